"""Shared by tests/test_gpu_fine_backward.py and tests/test_fine_backward_host.py: for the backward kernels of csrc/match_train.hip,
in the form of tests/train_ops_ref.py,
  (a) `*_ref64`  a float64 statement of the gradient, taking the fp32 inputs as given,
  (b) `*_bounds` a per-element first-order fp32 error bound for the arithmetic the kernel is documented to do (u = 2^-24),
  (c) `*_emul`   an fp32 NumPy emulation of that arithmetic (with `wrong=` switches: deliberately wrong formulae),
for the attention backward and the two loss backwards; for the head backward, which is float64 throughout, `head_bwd` is the unrolled
loop of include/t2p.h in a dtype of the caller's choice: np.longdouble is the reference, float64 the emulation, and the largest
distance between the two is the yardstick delta64 of a shape.  Plus the seeded inputs: random unit descriptors and entry lists.
Plain NumPy (torch only to draw the descriptors from torch.Generator).

Token rows are set-major: rows [0, B M) the object tokens (row b M + i), rows [B M, B (M + N)) the hint tokens."""
import functools

import numpy as np

from train_ops_ref import F32, U, U64

HEADS = 4
EXPF_ULPS = 4 * U           # device expf: 2 ulp = 4 u, twice what its documentation states


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def set_row(s, b, B, M, N):
    return b * M if s == 0 else B * M + b * N


# ---- attention backward -------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(1, 1, 1, 64), (2, 4, 2, 128), (3, 5, 7, 64), (2, 63, 1, 64), (2, 63, 63, 256)]     # (B, M, N, D)


@functools.lru_cache(maxsize=None)
def attn_inputs(B, M, N, D, seed=3):
    """qkv [B (M + N), 3 D] ~ N(0, 1) (scores of either sign, softmax rows from flat to peaked) and d_msg [B (M + N), D]."""
    rng = np.random.default_rng(seed)
    rows = B * (M + N)
    return _frozen(rng.standard_normal((rows, 3 * D)).astype(F32), rng.standard_normal((rows, D)).astype(F32))


def _attn_blocks(B, M, N, cross):
    """(target rows, source rows, head) of every workgroup."""
    for b in range(B):
        for ts in (0, 1):
            ss = 1 - ts if cross else ts
            nt, ns = (M, N)[ts], (M, N)[ss]
            t0, s0 = set_row(ts, b, B, M, N), set_row(ss, b, B, M, N)
            for h in range(HEADS):
                yield np.arange(t0, t0 + nt), np.arange(s0, s0 + ns), h


def _attn_apply(qkv, dmsg, B, M, N, D, cross, core, dtype, fill=np.nan, wrong=None):
    out = np.full((B * (M + N), 3 * D), fill, dtype=dtype)
    for tr, sr, h in _attn_blocks(B, M, N, cross):
        q, k, v = qkv[tr, h:D:HEADS], qkv[sr, D + h:2 * D:HEADS], qkv[sr, 2 * D + h:3 * D:HEADS]   # channel c = d * heads + h
        dq, dk, dv = core(q, k, v, dmsg[tr, h::HEADS])
        out[tr, h:D:HEADS] = dq
        if wrong == "dk_to_target":                      # dk written to the k columns of the TARGET rows
            r = min(len(tr), len(sr))
            out[tr[:r], D + h:2 * D:HEADS] = dk[:r]
        else:
            out[sr, D + h:2 * D:HEADS] = dk
        out[sr, 2 * D + h:3 * D:HEADS] = dv
    return out


def _attn_core64(q, k, v, do):
    q, k, v, do = (a.astype(np.float64) for a in (q, k, v, do))
    scale = 1.0 / np.sqrt(q.shape[1])
    s = scale * q @ k.T
    e = np.exp(s - s.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    dp = do @ v.T
    ds = p * (dp - (p * dp).sum(1, keepdims=True))
    return scale * ds @ k, scale * ds.T @ q, p.T @ do


def attn_bwd_ref64(qkv, dmsg, B, M, N, D, cross):
    return _attn_apply(qkv, dmsg, B, M, N, D, cross, _attn_core64, np.float64)


def attn_bwd_bounds(qkv, dmsg, B, M, N, D, cross):
    """The kernel: s = fl(scale fma-dot(q, k)); e = expf(s - max s); p = e / sum e; dP = fma-dot(dO, v); delta = fma-sum(p dP);
    dS = p (dP - delta); dq = scale fma-sum(dS k), dk = scale fma-sum(dS q), dv = fma-sum(p dO).  An n-term fma sum carries
    n u sum|terms|; every further operation one u of its result; the errors of the operands are carried along to first order.
    Softmax is invariant under a shift, so the error of the row maximum drops out: an error e_s of s is a relative error e_s of
    exp(s), on top of u |s - max| from the subtraction and expf's own error."""
    def core(q, k, v, do):
        q64, k64, v64, do64 = (a.astype(np.float64) for a in (q, k, v, do))
        aq, ak, av, ado = np.abs(q64), np.abs(k64), np.abs(v64), np.abs(do64)
        nt, dh = q.shape
        ns = k.shape[0]
        scale = 1.0 / np.sqrt(dh)
        s = scale * q64 @ k64.T
        e_s = (dh + 3) * U * scale * (aq @ ak.T)                        # dh fmas, the rounding of scale and of the product
        e = np.exp(s - s.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        r_e = e_s + U * np.abs(s - s.max(1, keepdims=True)) + EXPF_ULPS  # relative error of e
        r_p = r_e + (p * r_e).sum(1, keepdims=True) + (ns + 1) * U       # the sum of ns terms, the division
        e_p = p * r_p
        dp = do64 @ v64.T
        e_dp = dh * U * (ado @ av.T)
        delta = (p * dp).sum(1, keepdims=True)
        e_delta = (e_p * np.abs(dp) + p * e_dp).sum(1, keepdims=True) + (ns + 1) * U * (p * np.abs(dp)).sum(1, keepdims=True)
        diff = dp - delta
        ds = p * diff
        e_ds = e_p * np.abs(diff) + p * (e_dp + e_delta + U * np.abs(diff)) + U * np.abs(ds)
        e_dq = scale * (e_ds @ ak) + (ns + 3) * U * scale * (np.abs(ds) @ ak)
        e_dk = scale * (e_ds.T @ aq) + (nt + 3) * U * scale * (np.abs(ds).T @ aq)
        e_dv = e_p.T @ ado + (nt + 1) * U * (p.T @ ado)
        return e_dq, e_dk, e_dv
    return _attn_apply(qkv, dmsg, B, M, N, D, cross, core, np.float64)


def attn_bwd_emul(qkv, dmsg, B, M, N, D, cross, wrong=None):
    """fp32 throughout.  wrong: "no_rowsum" (dS = P o dP), "no_scale" (dq and dk without the factor scale), "dk_to_target"."""
    def core(q, k, v, do):
        scale = F32(1.0) / np.sqrt(F32(q.shape[1]))
        s = (q @ k.T) * scale
        e = np.exp(s - s.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True, dtype=F32)
        dp = do @ v.T
        delta = F32(0.0) if wrong == "no_rowsum" else (p * dp).sum(1, keepdims=True, dtype=F32)
        ds = p * (dp - delta)
        out_scale = F32(1.0) if wrong == "no_scale" else scale
        return (ds @ k) * out_scale, (ds.T @ q) * out_scale, p.T @ do
    return _attn_apply(qkv, dmsg, B, M, N, D, cross, core, F32, wrong=wrong)


# ---- loss backwards -----------------------------------------------------------------------------------------------------------------
def pack_entries(lists):
    """List of [M_b, 2] integer arrays -> (idx int32 [n, 2], entry_ptr int32 [B + 1]) as losses.MatchingLoss packs them."""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(a) for a in lists], out=ptr[1:])
    return np.concatenate(lists, axis=0).astype(np.int32).reshape(-1, 2), ptr.astype(np.int32)


def _entry_counts(shape, lists):
    c = np.zeros(shape, dtype=np.float64)
    for b, a in enumerate(lists):
        np.add.at(c[b], (np.asarray(a)[:, 0], np.asarray(a)[:, 1]), 1.0)      # a pair listed twice counts twice
    return c


def matching_loss_bwd_ref64(P, lists, g):
    """dP[b, i, j] = -g count / (B M_b P[b, i, j]) where the sample lists (i, j), exactly 0 elsewhere; P = 0 gives -inf."""
    c = _entry_counts(P.shape, lists)
    mb = np.array([len(a) for a in lists], dtype=np.float64)[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        val = -(float(g) * c) / (P.shape[0] * mb * P.astype(np.float64))
    return np.where(c > 0, val, 0.0)


def matching_loss_bwd_bounds(ref):
    """Float64 products and one quotient, rounded to fp32 once."""
    fin = np.where(np.isfinite(ref), np.abs(ref), 0.0)
    return (U + 8 * U64) * fin


def matching_loss_bwd_emul(P, lists, g, wrong=None):
    """wrong: "no_count" (a pair listed twice counted once), "no_batch" (the factor 1 / B missing)."""
    c = _entry_counts(P.shape, lists)
    if wrong == "no_count":
        c = np.minimum(c, 1.0)
    mb = np.array([len(a) for a in lists], dtype=np.float64)[:, None, None]
    denom = mb * (1.0 if wrong == "no_batch" else float(P.shape[0]))
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        val = (-(float(F32(g)) * c) / (denom * P.astype(np.float64))).astype(F32)
    return np.where(c > 0, val, F32(0.0)).astype(F32)


def mse_bwd_ref64(a, b, g):
    return 2.0 * float(g) * (a.astype(np.float64) - b.astype(np.float64)) / a.size


def mse_bwd_bounds(ref):
    return (U + 8 * U64) * np.abs(ref)


def mse_bwd_emul(a, b, g, wrong=None):
    """wrong: "no_two"."""
    f = (1.0 if wrong == "no_two" else 2.0) * float(F32(g)) / float(a.size)
    return (f * (a.astype(np.float64) - b.astype(np.float64))).astype(F32)


# ---- optimal-transport head ---------------------------------------------------------------------------------------------------------
def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.exp(x - m).sum(axis=axis))


def head_forward(md, B, M, N, D, alpha, iters, dtype):
    """The forward of t2p_match_head in `dtype`: per sample (Z0 [M + 1, N + 1], [(u_t, v_t) for t = 1 .. iters], log_mu, log_nu,
    norm)."""
    md = np.asarray(md).astype(dtype)
    one = dtype(1.0)
    norm = -np.log(dtype(M + N))
    log_mu = np.concatenate([np.full(M, norm, dtype), [np.log(dtype(N)) + norm]]).astype(dtype)
    log_nu = np.concatenate([np.full(N, norm, dtype), [np.log(dtype(M)) + norm]]).astype(dtype)
    out = []
    for b in range(B):
        m0 = md[set_row(0, b, B, M, N): set_row(0, b, B, M, N) + M]
        m1 = md[set_row(1, b, B, M, N): set_row(1, b, B, M, N) + N]
        z0 = np.full((M + 1, N + 1), dtype(alpha), dtype=dtype)
        z0[:M, :N] = (m0 @ m1.T) * (one / np.sqrt(dtype(D)))
        u, v = np.zeros(M + 1, dtype), np.zeros(N + 1, dtype)
        its = []
        for _ in range(iters):
            u = log_mu - _lse(z0 + v[None, :], 1)
            v = log_nu - _lse(z0 + u[:, None], 0)
            its.append((u, v))
        out.append((z0, its, log_mu, log_nu, norm))
    return out


def head_scores_fma(md, B, M, N, D, alpha):
    """Z0 [B, M + 1, N + 1] with the kernels' own bits (transport_scores of csrc/match_common.h): a = fma(x_k, y_k, a) over k in
    order in float64, times 1 / sqrt(D) once, alpha in the dustbin row and column.  The product of two fp32 values has 48
    significant bits and is exact in float64, so `a + x_k * y_k` rounds once, as the fma does: no tolerance is needed."""
    md = np.asarray(md)
    assert md.dtype == F32
    z0 = np.full((B, M + 1, N + 1), np.float64(F32(alpha)))
    for b in range(B):
        m0 = md[set_row(0, b, B, M, N): set_row(0, b, B, M, N) + M].astype(np.float64)
        m1 = md[set_row(1, b, B, M, N): set_row(1, b, B, M, N) + N].astype(np.float64)
        a = np.zeros((M, N))
        for k in range(D):
            a = a + m0[:, k, None] * m1[None, :, k]
        z0[b, :M, :N] = a * (1.0 / np.sqrt(np.float64(D)))
    return z0


def head_couplings(md, B, M, N, D, alpha, iters, dtype=np.float64):
    """P [B, M + 1, N + 1] in `dtype`."""
    p = []
    for z0, its, _, _, norm in head_forward(md, B, M, N, D, alpha, iters, dtype):
        u, v = its[-1] if its else (np.zeros(M + 1, dtype), np.zeros(N + 1, dtype))
        p.append(np.exp(z0 + u[:, None] + v[None, :] - norm))
    return np.stack(p)


def head_bwd(md, dP, B, M, N, D, alpha, iters, dtype=np.longdouble):
    """(d_mdesc [B (M + N), D], d_bin [B]) in `dtype`: G = dP exp(Z) and the unrolled iterations walked backwards, as include/t2p.h
    states them.  md and dP are taken as given (fp32)."""
    md_t = np.asarray(md).astype(dtype)
    dP = np.asarray(dP).astype(dtype)
    d_md = np.zeros(md_t.shape, dtype=dtype)
    d_bin = np.zeros(B, dtype=dtype)
    inv = dtype(1.0) / np.sqrt(dtype(D))
    for b, (z0, its, log_mu, log_nu, norm) in enumerate(head_forward(md, B, M, N, D, alpha, iters, dtype)):
        u, v = its[-1] if its else (np.zeros(M + 1, dtype), np.zeros(N + 1, dtype))
        gz = dP[b] * np.exp(z0 + u[:, None] + v[None, :] - norm)
        gu, gv = gz.sum(1), gz.sum(0)
        for t in range(iters - 1, -1, -1):
            u, v = its[t]
            vp = its[t - 1][1] if t > 0 else np.zeros(N + 1, dtype)
            w = np.exp(z0 + u[:, None] + v[None, :] - log_nu[None, :])        # columns sum to 1
            gz = gz - w * gv[None, :]
            gu = gu - w @ gv
            r = np.exp(z0 + vp[None, :] + u[:, None] - log_mu[:, None])       # rows sum to 1
            gz = gz - gu[:, None] * r
            gv = -(r.T @ gu)
            gu = np.zeros(M + 1, dtype)
        d_bin[b] = gz[:, N].sum() + gz[M, :N].sum()
        gs = gz[:M, :N]
        r0, r1 = set_row(0, b, B, M, N), set_row(1, b, B, M, N)
        d_md[r0: r0 + M] = (gs @ md_t[r1: r1 + N]) * inv
        d_md[r1: r1 + N] = (gs.T @ md_t[r0: r0 + M]) * inv
    return d_md, d_bin


# ---- inputs of the matcher tests ----------------------------------------------------------------------------------------------------
MATCHER_CASES = [dict(B=2, M=4, N=2, D=128, layers=1, seed=1), dict(B=4, M=16, N=6, D=128, layers=2, seed=3),
                 dict(B=2, M=63, N=63, D=64, layers=1, seed=5)]
MIN_COUPLING = 1e-30


def unit_descriptors(B, M, N, D, seed):
    """Random unit rows drawn in float64 from torch.Generator().manual_seed(seed): (desc0 [B, M, D], desc1 [B, N, D]) float64."""
    import torch
    g = torch.Generator().manual_seed(seed)
    d0 = torch.nn.functional.normalize(torch.randn(B, M, D, generator=g, dtype=torch.float64), dim=-1)
    d1 = torch.nn.functional.normalize(torch.randn(B, N, D, generator=g, dtype=torch.float64), dim=-1)
    return d0, d1


def entry_lists(B, M, N, seed):
    """Per sample: k ~ U{1 .. min(M, N)} pairs (o, h_o), o = 0 .. k - 1, h a sorted random subset of the hints; then every unmatched hint
    as (M, h), every unmatched object as (o, N) - the layout of synthetic.make_fine_batch's all_matches."""
    rng = np.random.default_rng(seed)
    lists = []
    for _ in range(B):
        k = int(rng.integers(1, min(M, N) + 1))
        h = np.sort(rng.choice(N, size=k, replace=False))
        rest_h = np.setdiff1d(np.arange(N), h)
        a = [(o, int(h[o])) for o in range(k)] + [(M, int(x)) for x in rest_h] + [(o, N) for o in range(k, M)]
        lists.append(np.asarray(a, dtype=np.int64).reshape(-1, 2))
    return lists


def keep_listed(lists, p64, floor=MIN_COUPLING):
    """The entries whose float64 coupling is at least `floor` (below fp32's range -log P is inf, in the reference as here).
    Returns (kept lists, entries kept, entries listed)."""
    p64 = np.asarray(p64)
    kept = [a[p64[b, a[:, 0], a[:, 1]] >= floor] for b, a in enumerate(lists)]
    return kept, sum(len(a) for a in kept), sum(len(a) for a in lists)
