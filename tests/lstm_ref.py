"""Shared by tests/test_gpu_text_recurrence.py and tests/test_lstm_ref_host.py: the persistent biLSTM of the inference text branch
(csrc/lstm.hip: k_bilstm<128|256|384> and k_bilstm_x3<128|256|384>, reached through t2p_encode_text), in the manner of gemm_ref.py:
  (a) `case_inputs`   seeded inputs in nn.LSTM's own parameter layout (computed once per case, handed out read-only),
  (b) `bilstm_ref64`  a float64 statement of LanguageEncoder.forward on the fp32 inputs as given, `normalized` its L2-normalised rows,
  (c) `bilstm_bound`  a running error bound carried beside the reference, per row and unit,
  (d) `bilstm_emul`   a NumPy emulation of each kernel's documented arithmetic and of the persistent schedule, with `wrong=`
                      switches that build one plausible defect each - in the emulation only, never in a kernel or the package.
Plain NumPy: no GPU, no torch.  The GPU tests assert |kernel - (b)| <= 2 (c) element by element; the host tests prove that (b) is
what torch's float64 LSTM computes, that (d) stays within 1 (c), that max (c) <= CAP on every bound-checked case, and that the
same check rejects every wrong variant.

Inputs.  The gate table  E W_ih^T + b_ih + b_hh  is EXACT: embedding entries are multiples of 1/4 in [-1, 1] (NNZ_EMB of them per
row, row 0 zero), W_ih entries multiples of 1/64 in [-1/8, 1/8], both biases multiples of 1/64: every partial sum is a multiple of
2^-8 far below 2^16, exact in fp32 in any summation order, and so is its product with w_hh_scale (a power of two).  The table adds
no error: the bounds are about the recurrence alone.  Only NNZ_EMB entries of an embedding row are non-zero because the
accumulator of a recurrent product STARTS at the table value, whose magnitude therefore enters every rounding of the chain
(gamma_n |table| below): a dense row makes |table| ~ 3 and the bound 1e-4 at D = 384 whatever the recurrence does.
W_hh families: `contractive` |w| <= C_CONTRACT / D;  `reference` 1.5 u / sqrt(D) as tests/golden/weights.py fills LSTM weights,
times `mult`;  `permuted` one entry of magnitude [1/2, 1] per gate column - the only family on which a dropped lo.hi product
(2^-12 relative on ONE product) is not hidden under gamma_(3D+2) of a D-term sum.

Bound - derived, not tuned; u, gamma_n, eta and the split terms as in gemm_ref.py's text.  Per direction and time step, with h, c
the float64 states, dh, dc the bounds carried so far, A = |h| + dh (a bound on the kernel's |h|), K the number of units with
A > 0 (the kernel's width, unless units of h are exactly 0: fma(0, w, acc) = acc does not round; K = 0 at the first step):
  pre-activations   dz = |W_hh|^T dh + prod             (the drain acc / s is a product with a power of two: exact, it adds nothing)
     fp32 kernel    prod = gamma_(K+2) (|table| + A |W_hh|)          (one chain from the table value, K products in MFMA order)
     f16x3 kernel   prod = (split + gamma_(3K+2) (s |table| + S3)) / s, split and S3 of gemm_ref.x3_bound with a = h, w' = s w;
                    split holds the planes' own error |hn - hi - lo| <= 2^-22 |hn| + (1 + 2^-11) eta, times |w'|
                    (prod = 0 where K = 0)
  gates             di, df, do = dz / 4 + EPS_GATE,  dg = dz + EPS_GATE   (sigmoid is 1/4-Lipschitz, tanh 1-Lipschitz); both forms
                    of tanh return 0 at an exact 0 (copysign of (1 - 1) r; tanhf(0) = 0): there dg = 0, and a unit whose h is
                    exactly 0 in the kernel too adds no product and no eta term to split and S3
  cell              c' = f c + i g:  dc' = |f| dc + |c| df + df dc + |i| dg + |g| di + di dg + 2 u (1 + u) (F + G),
                    F = (|f| + df)(|c| + dc), G = (|i| + di)(|g| + dg)   (two products and a sum, or one product and an fma)
  hidden            h' = o tanh(c'):  dt = dc' + EPS_GATE,  dh' = |o| dt + |t| do + do dt + u (|o| + do)(|t| + dt)
  output            raw = (h_fwd + h_bwd) / 2:  (dh_fwd + dh_bwd) / 2 + u |raw|
  normalised        y = x / |x|_2: the kernel's norm is a sum of K squares (K / 64 fma per lane, six butterfly adds), a square root
                    and a division: relative error rho = gamma_(K/64+8); with e = |dx|_2 and n_lo = (|x| - e)(1 - rho)
                    dy = dx / n_lo + |x| (e + rho (|x| + e)) / (|x| n_lo) + u (|y| + that)
EPS_GATE = 2e-7 for both kernels: the figure lstm.hip documents for its fast forms; the library forms of the fp32 kernel are taken
to be no worse.  test_gate_functions_in_isolation measures it."""
import functools
import zlib

import numpy as np

from gemm_ref import ETA, F32, FACTOR_GPU, U, bits_equal, gamma, split_f16, within, worst_ratio  # noqa: F401

EPS_GATE = 2e-7
CAP = 5e-5                      # half the suite's TOL = 1e-4
TOL = 1e-4
TOL_PRECISIONS = 2e-5
NUM_CUS = 256
C_CONTRACT = 0.5
NNZ_EMB = 16
PRECISIONS = ("fp32", "f16x3")
WIDTHS = [(128, 128), (256, 256), (384, 384), (300, 384), (64, 128)]        # (embed_dim, kernel width)
MULTS = [2.0 ** -6, 1.0, 2.0 ** 3, 2.0 ** 6]     # f16x3_scale clips at 2^15: x 2^-6 and x 1 share it, x 8 is the third value
WRONG = ["state_not_reset", "planes_not_cleared", "reverse_from_T", "finished_row_updated", "last_word_zero_row", "no_lo_hi",
         "table_not_scaled", "drain_no_inv_scale"]


def kernel_dim(d):
    return (d + 127) // 128 * 128


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

def _lengths(b, t, rng, layout):
    """layout: random (rows 0 and 1 at T and 1, the rest of group 0 random; the partial group behind row 32 has one row at T and
    the rest at 1) | equal (T for all) | equal_then_T (a full group at T - 3, then rows at T) | plain (T, 1, the rest random)."""
    if layout == "equal":
        return np.full(b, t, np.int32)
    ln = rng.integers(1, t + 1, b).astype(np.int32)
    if layout == "plain":                   # one row at T, one at 1, the rest random
        ln[0], ln[1] = t, 1
        return ln
    if layout == "equal_then_T":            # B = 33: a full group at one length below T, then a lone row at T
        ln[:] = max(t - 3, 1)
        ln[32:] = t
        return ln
    if b >= 2:
        ln[0], ln[1] = t, 1
    else:
        ln[0] = t
    if b > 32:                              # the partial last group: one row at T, the rest at 1
        ln[32:] = 1
        ln[b - 1 if b - 1 > 32 else 32] = t
    return ln


def _tokens(ln, t, vocab, rng):
    """[B][T] int32, 0 behind each length; every id of [0, vocab) occurs as a word where there is room, vocab - 1 and 0 always."""
    b = len(ln)
    tok = rng.integers(0, vocab, (b, t)).astype(np.int32)
    valid = np.arange(t)[None, :] < ln[:, None]
    pos = np.argwhere(valid)
    pos = pos[rng.permutation(len(pos))]
    ids = list(range(vocab))
    ids = [vocab - 1, 0] + ids[1:-1]
    for (r, c), v in zip(pos, ids):
        tok[r, c] = v
    tok[~valid] = 0
    return tok


def _weights(d, vocab, family, mult, live, rng):
    emb = np.zeros((vocab, d), np.float64)
    for v in range(1, vocab):
        cols = rng.choice(d, min(NNZ_EMB, d), replace=False)
        emb[v, cols] = rng.integers(-4, 5, len(cols)) / 4.0
    w_ih = rng.integers(-8, 9, (2, 4 * d, d)) / 64.0
    b_ih = rng.integers(-8, 9, (2, 4 * d)) / 64.0
    b_hh = rng.integers(-8, 9, (2, 4 * d)) / 64.0
    if live:                                # the cell input g = tanh(0) = 0 at step 1 in all but `live` units: h_1 is exactly 0 there
        dead = np.ones(d, bool)
        dead[rng.choice(d, min(live, d), replace=False)] = False
        for arr in (w_ih, b_ih, b_hh):
            arr[:, 2 * d: 3 * d][:, dead] = 0.0
    if family == "contractive":
        w_hh = rng.uniform(-1.0, 1.0, (2, 4 * d, d)) * (C_CONTRACT / d)
    elif family == "reference":
        w_hh = rng.uniform(-1.0, 1.0, (2, 4 * d, d)) * (1.5 / np.sqrt(d)) * mult
    elif family == "permuted":
        w_hh = np.zeros((2, 4 * d, d))
        for i in range(2):
            for q in range(4):
                w_hh[i, q * d + np.arange(d), rng.permutation(d)] = rng.uniform(0.5, 1.0, d) * rng.choice([-1.0, 1.0], d)
    else:
        raise ValueError(family)
    return dict(emb=emb.astype(F32), w_ih=w_ih.astype(F32), w_hh=w_hh.astype(F32), b_ih=b_ih.astype(F32), b_hh=b_hh.astype(F32))


@functools.lru_cache(maxsize=None)
def case_inputs(d, b, t, vocab, family="contractive", mult=1.0, layout="random", live=0, seed=0):
    """dict(d, vocab, emb [V][d], w_ih, w_hh [2][4d][d] (nn.LSTM layout, direction 1 = reverse), b_ih, b_hh [2][4d],
    tokens [B][T] int32, lengths [B] int32).  live > 0: only that many units have a non-zero cell input from the table (LIVE_UNITS)."""
    rng = np.random.default_rng([seed, d, b, t, vocab, int(np.log2(mult)) + 64, live, zlib.crc32(family.encode()), zlib.crc32(layout.encode())])
    p = _weights(d, vocab, family, mult, live, rng)
    ln = _lengths(b, t, rng, layout)
    p.update(d=d, vocab=vocab, tokens=_tokens(ln, t, vocab, rng), lengths=ln)
    return _frozen(p)


# Reference-like W_hh times 8 or 64 makes sum |h||w| ~ 10 .. 10^2 per pre-activation when every unit of h_1 is alive, and
# gamma_(3K+2) of that is 7e-5 .. 5e-3 after ONE step (times 1 stays below CAP with every unit alive, and runs so).  Those cases keep h_1 exactly 0 (g = tanh(0), exact in both kernels) in all but a
# few units, so that the recurrent term of step 2 is a sum of that many products of ordinary size and the bound stays below CAP.
LIVE_UNITS = {8.0: 4, 64.0: 1}


def width_cases():
    """(label, inputs) of GPU check 2: every width, B = 37 (one-and-a-bit groups), T = 7, vocab 11; B = 1, 32, 33 at D = 256."""
    out = [(f"contractive d={d} B=37 T=7", case_inputs(d, 37, 7, 11)) for d, _ in WIDTHS]
    out += [(f"contractive d=256 B={b} T=7", case_inputs(256, b, 7, 11, layout=lay))
            for b, lay in ((1, "random"), (32, "equal"), (33, "equal_then_T"))]
    return out


def scale_cases():
    """GPU check 3: reference-like W_hh times 2^-6, 1, 8, 2^6 at T = 2 on every width (every unit alive up to x 1), and two extra
    cases at D = 128 for the dropped lo.hi product: x 1 with 64 live units, and the permuted family at T = 3."""
    out = [(f"reference x{m:g} d={d} B=37 T=2", case_inputs(d, 37, 2, 11, "reference", m, live=LIVE_UNITS.get(m, 0)))
           for d, _ in WIDTHS for m in MULTS]
    return out + [("reference x1 (64 live) d=128 B=37 T=2", case_inputs(128, 37, 2, 11, "reference", 1.0, live=64)),
                  ("permuted d=128 B=37 T=3", case_inputs(128, 37, 3, 11, "permuted"))]


LONG_T = 162


def long_cases(family):
    return [(f"{family} d={d} B=40 T={LONG_T}", case_inputs(d, 40, LONG_T, 11, family, layout="plain")) for d in (128, 256, 384)]


def group_lengths(b, t, per_dir, rng):
    """The group loop's lengths: a workgroup's first pass is short (<= 2) on even groups and T on odd ones, its second pass the
    reverse, the third as the first: stale state and a stale max_len both show."""
    grp = np.arange(b) // 32
    long_ = ((grp // per_dir) % 2 == 1) ^ (grp % 2 == 1)
    ln = np.where(long_, t, rng.integers(1, 3, b)).astype(np.int32)
    return ln


@functools.lru_cache(maxsize=None)
def group_inputs(d, per_dir, passes, t=5, vocab=11, seed=5):
    """B = 32 per_dir (passes - 1) + 1 rows: the last pass holds one lone row.  Contractive family, exact table."""
    b = 32 * per_dir * (passes - 1) + 1
    rng = np.random.default_rng([seed, d, per_dir, passes, t])
    p = _weights(d, vocab, "contractive", 1.0, 0, rng)
    ln = group_lengths(b, t, per_dir, rng)
    p.update(d=d, vocab=vocab, tokens=_tokens(ln, t, vocab, rng), lengths=ln)
    return _frozen(p)


def group_rows(b, per_dir, n_random=100, seed=6):
    """First and last row of groups 0, per_dir - 1, per_dir, 2 per_dir - 1, 2 per_dir and the last, plus n_random seeded rows."""
    n_groups = (b + 31) // 32
    rows = set()
    for g in (0, per_dir - 1, per_dir, 2 * per_dir - 1, 2 * per_dir, n_groups - 1):
        if 0 <= g < n_groups:
            rows.update((32 * g, min(32 * g + 31, b - 1)))
    rng = np.random.default_rng([seed, b, per_dir])
    rows.update(int(r) for r in rng.choice(b, min(n_random, b), replace=False))
    return np.array(sorted(rows), np.int64)


GATE_SPECIALS = [0.0, 2.0 ** -20, 20.0, 88.0, 90.0, 104.0]
GATE_HELD = dict(i=2.0, f=2.0, g=1.0, o=1.0)


@functools.lru_cache(maxsize=None)
def gate_inputs(d=128, seed=7):
    """T = 1 sentences of one word each; word v's embedding is x_v in column 0 and W_ih's column 0 is 1 for the swept gate of a
    unit, so the swept pre-activation is exactly x_v (its bias is 0) and the other gates sit at GATE_HELD (their biases).  Units
    [0, d/4) sweep i, the next quarter f, then g, then o.  x_v: the multiples of 13/256 in [-104, 104] (4,097 values) and
    +-GATE_SPECIALS.  With h_0 = c_0 = 0 the forget gate reaches the output only through 0 f: its sweep shows non-finite values."""
    xs = np.concatenate([np.arange(-2048, 2049) * (13.0 / 256.0), np.array(GATE_SPECIALS), -np.array(GATE_SPECIALS)])
    vocab = len(xs) + 1
    emb = np.zeros((vocab, d), F32)
    emb[1:, 0] = xs
    assert np.array_equal(emb[1:, 0].astype(np.float64), xs)
    w_ih = np.zeros((2, 4 * d, d), F32)
    b_ih = np.zeros((2, 4 * d), F32)
    q4 = d // 4
    for q, name in enumerate("ifgo"):
        swept = np.arange(q * q4, (q + 1) * q4)
        w_ih[:, q * d + swept, 0] = 1.0
        held = np.setdiff1d(np.arange(d), swept)
        b_ih[:, q * d + held] = GATE_HELD[name]
    rng = np.random.default_rng([seed, d])
    w_hh = (rng.uniform(-1.0, 1.0, (2, 4 * d, d)) * (C_CONTRACT / d)).astype(F32)
    tokens = np.arange(1, vocab, dtype=np.int32)[:, None].copy()
    return _frozen(dict(d=d, vocab=vocab, emb=emb, w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=np.zeros((2, 4 * d), F32), tokens=tokens,
                        lengths=np.ones(vocab - 1, np.int32), xs=xs))


# ---- the kernel's view of the weights (packing.pack_text_weights restated) ---------------------------------------------------------------

def w_hh_scale(inp):
    """packing.f16x3_scale of the recurrent matrices: the largest power of two s with max |s w| <= 2^14, clipped to [2^-8, 2^15]."""
    m = float(np.abs(inp["w_hh"]).max())
    if m == 0.0:
        return 1.0
    return float(2.0 ** max(-8, min(15, int(np.floor(np.log2(2.0 ** 14 / m))))))


def _gates_kmajor(w, d, dk):
    out = np.zeros((dk, 4 * dk), np.float64)
    for q in range(4):
        out[:d, q * dk: q * dk + d] = w[q * d: (q + 1) * d, :].astype(np.float64).T
    return out


def _gates_vec(b, d, dk):
    out = np.zeros(4 * dk, np.float64)
    for q in range(4):
        out[q * dk: q * dk + d] = b[q * d: (q + 1) * d]
    return out


def kernel_view(inp, dk=None):
    """dict(table [2][V + 1][4 dk] float64 with the zero row at V, w_hh [2][dk][4 dk] k-major float64 of the fp32 values)."""
    d, v = inp["d"], inp["vocab"]
    dk = kernel_dim(d) if dk is None else dk
    emb = np.zeros((v, dk), np.float64)
    emb[:, :d] = inp["emb"]
    table = np.zeros((2, v + 1, 4 * dk), np.float64)
    w_hh = np.zeros((2, dk, 4 * dk), np.float64)
    for i in range(2):
        bias = _gates_vec(inp["b_ih"][i].astype(np.float64), d, dk) + _gates_vec(inp["b_hh"][i].astype(np.float64), d, dk)
        table[i, :v] = emb @ _gates_kmajor(inp["w_ih"][i], d, dk) + bias.astype(F32).astype(np.float64)
        w_hh[i] = _gates_kmajor(inp["w_hh"][i], d, dk)
    return dict(table=table, w_hh=w_hh, dk=dk)


def table_is_exact(inp):
    """The fp32 gate table, formed by an fp32 fma chain over k in order (k_gemm), equals the float64 one bit for bit - and its
    partial sums in the reverse order too."""
    d, v = inp["d"], inp["vocab"]
    kv = kernel_view(inp, d)
    for i in range(2):
        w = _gates_kmajor(inp["w_ih"][i], d, d).astype(F32)
        for order in (range(d), range(d - 1, -1, -1)):
            acc = np.zeros((v, 4 * d), F32)
            for k in order:
                acc = (acc.astype(np.float64) + inp["emb"][:, k: k + 1].astype(np.float64) * w[k: k + 1].astype(np.float64)).astype(F32)
            bias = (inp["b_ih"][i].astype(F32) + inp["b_hh"][i].astype(F32)).astype(F32)
            acc = (acc + bias[None, :]).astype(F32)
            if not np.array_equal(acc.astype(np.float64), kv["table"][i, :v]):
                return False
    return True


# ---- float64 statement -----------------------------------------------------------------------------------------------------------------

def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _step_index(ln, step, reverse):
    return np.clip(ln - 1 - step, 0, None) if reverse else np.minimum(step, np.maximum(ln - 1, 0))


def bilstm_ref64(inp, rows=None):
    """[n][d] float64: embedding, packed-sequence semantics (forward reads tokens 0 .. len - 1, reverse len - 1 .. 0), gates
    i, f, g, o, the mean of the two final hidden states.  rows: only these rows (rows are independent)."""
    d = inp["d"]
    tok, ln = inp["tokens"], inp["lengths"]
    if rows is not None:
        tok, ln = tok[rows], ln[rows]
    n = len(ln)
    emb = inp["emb"].astype(np.float64)
    total = np.zeros((n, d))
    for i in range(2):
        w_ih, w_hh = inp["w_ih"][i].astype(np.float64), inp["w_hh"][i].astype(np.float64)
        b = inp["b_ih"][i].astype(np.float64) + inp["b_hh"][i].astype(np.float64)
        h, c = np.zeros((n, d)), np.zeros((n, d))
        for step in range(int(ln.max()) if n else 0):
            act = (step < ln)[:, None]
            x = emb[tok[np.arange(n), _step_index(ln, step, i == 1)]]
            z = x @ w_ih.T + h @ w_hh.T + b
            ig, fg, gg, og = sigmoid64(z[:, :d]), sigmoid64(z[:, d: 2 * d]), np.tanh(z[:, 2 * d: 3 * d]), sigmoid64(z[:, 3 * d:])
            cn = fg * c + ig * gg
            hn = og * np.tanh(cn)
            c, h = np.where(act, cn, c), np.where(act, hn, h)
        total += h
    return total / 2.0


def normalized(raw):
    """F.normalize(raw, dim=-1) in float64."""
    n = np.sqrt((raw * raw).sum(1, keepdims=True))
    return raw / np.maximum(n, 1e-12)


def pad_cols(x, dk):
    out = np.zeros((x.shape[0], dk), x.dtype)
    out[:, : x.shape[1]] = x
    return out


# ---- bound -------------------------------------------------------------------------------------------------------------------------------

def bilstm_bound(inp, precision, rows=None, dk=None):
    """dict(raw, out): [n][dk] bounds on |kernel - float64| of the encoder output and of its normalised rows (module text)."""
    kv = kernel_view(inp, dk)
    dk = kv["dk"]
    tok, ln = inp["tokens"], inp["lengths"]
    if rows is not None:
        tok, ln = tok[rows], ln[rows]
    n = len(ln)
    s = w_hh_scale(inp)
    k = dk
    total, dtotal = np.zeros((n, dk)), np.zeros((n, dk))
    for i in range(2):
        w, table = kv["w_hh"][i], kv["table"][i]
        wa = np.abs(w)
        h, c, dh, dc = (np.zeros((n, dk)) for _ in range(4))
        for step in range(int(ln.max()) if n else 0):
            act = (step < ln)[:, None]
            tab = table[tok[np.arange(n), _step_index(ln, step, i == 1)]]
            z = tab + h @ w
            a = np.abs(h) + dh
            nz = (a > 0.0).astype(np.float64)                   # a unit that is exactly 0 in the kernel too adds no product,
            kk = nz.sum(1)[:, None]                             # and fma(0, w, acc) = acc: only kk products round
            if precision == "fp32":
                prod = np.where(kk > 0, gamma(kk + 2), 0.0) * (np.abs(tab) + a @ wa)
            else:
                ws = wa * s
                sm = a @ ws
                lin = a.sum(1)[:, None] + nz @ ws
                split = 3 * 2.0 ** -22 * (1 + 2.0 ** -10) * sm + (1 + 2.0 ** -9) * ETA * lin + 6 * ETA * ETA * kk
                s3 = (1 + 2.0 ** -8) * sm + 4 * ETA * lin + 6 * ETA * ETA * kk
                prod = (split + np.where(kk > 0, gamma(3 * kk + 2), 0.0) * (s * np.abs(tab) + s3)) / s
            dz = dh @ wa + prod
            zi, zf, zg, zo = (z[:, q * dk: (q + 1) * dk] for q in range(4))
            di, df, dg, do = (dz[:, q * dk: (q + 1) * dk] * (1.0 if q == 2 else 0.25) + EPS_GATE for q in range(4))
            dg = np.where((zg == 0.0) & (dz[:, 2 * dk: 3 * dk] == 0.0), 0.0, dg)        # tanh(0) = 0 exactly
            ig, fg, gg, og = sigmoid64(zi), sigmoid64(zf), np.tanh(zg), sigmoid64(zo)
            cn = fg * c + ig * gg
            f_, g_ = (fg + df) * (np.abs(c) + dc), (ig + di) * (np.abs(gg) + dg)
            dcn = fg * dc + np.abs(c) * df + df * dc + ig * dg + np.abs(gg) * di + di * dg + 2 * U * (1 + U) * (f_ + g_)
            t = np.tanh(cn)
            dt = np.where((cn == 0.0) & (dcn == 0.0), 0.0, dcn + EPS_GATE)
            hn = og * t
            dhn = og * dt + np.abs(t) * do + do * dt + U * (og + do) * (np.abs(t) + dt)
            c, h, dc, dh = np.where(act, cn, c), np.where(act, hn, h), np.where(act, dcn, dc), np.where(act, dhn, dh)
        total += h
        dtotal += dh
    raw = total / 2.0
    b_raw = dtotal / 2.0 + U * np.abs(raw)
    nrm = np.sqrt((raw * raw).sum(1, keepdims=True))
    e = np.sqrt((b_raw * b_raw).sum(1, keepdims=True))
    rho = gamma(k // 64 + 8)
    n_lo = (nrm - e) * (1.0 - rho)
    assert np.all(n_lo > 1e-9), "a reference row too close to zero for the normalised bound"
    y = np.abs(raw) / nrm
    dy = b_raw / n_lo + np.abs(raw) * (e + rho * (nrm + e)) / (nrm * n_lo)
    return dict(raw=b_raw, out=dy + U * (y + dy))


# ---- emulation ---------------------------------------------------------------------------------------------------------------------------

def _f32(x):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.asarray(x, np.float64).astype(F32)


def _gate_sigmoid(x, fast):
    x = x.astype(np.float64)
    if not fast:                                        # library expf, then 1 / (1 + e)
        return _f32(1.0 / _f32(1.0 + _f32(np.exp(np.clip(-x, -745, 745))).astype(np.float64)).astype(np.float64))
    with np.errstate(over="ignore"):
        e = _f32(np.exp(-x))                            # v_exp_f32: inf past fp32's range, and rcp(inf) = 0
        return _f32(1.0 / _f32(1.0 + e.astype(np.float64)).astype(np.float64))


def _gate_tanh(x, fast):
    x = x.astype(np.float64)
    if not fast:
        return _f32(np.tanh(x))
    t = _f32(np.exp(_f32(-2.0 * np.abs(x)).astype(np.float64))).astype(np.float64)
    r = _f32(_f32(1.0 - t).astype(np.float64) * _f32(1.0 / _f32(1.0 + t).astype(np.float64)).astype(np.float64))
    return np.copysign(r, x).astype(F32)


def schedule(b, precision, num_cus=NUM_CUS):
    """(grid.x, [groups of workgroup 0, of workgroup 1, ...]): the fp32 kernel has one workgroup per group of 32 rows, the f16x3
    kernel at most num_cus / 2 per direction, each taking the groups blockIdx.x, blockIdx.x + grid.x, ..."""
    n_groups = (b + 31) // 32
    grid = n_groups
    if precision == "f16x3":
        grid = min(n_groups, max(1, num_cus // 2))
    return grid, [list(range(w, n_groups, grid)) for w in range(grid)]


def bilstm_emul(inp, precision, num_cus=NUM_CUS, wrong=None, dk=None, rows=None):
    """[B][dk] fp32: what the kernel of `precision` computes, in its order of products.
    fp32: the accumulator starts at the table value; MFMA s adds h[s] w[s] and h[K/2 + s] w[K/2 + s] (the two lane halves), s in
    order; library gate functions.  f16x3: the accumulator starts at s x table; per k-step of 16 (k = 8 j .. 8 j + 7 of both
    halves of K) three MFMAs hi.hi, hi.lo, lo.hi add their 16 exact products and round once each; z = acc / s; the fast gate
    functions; hn goes to the planes as hi = fp16(hn), lo = fp16(hn - hi).  A row is updated while step < len; the rows of one
    group run max(len) steps; a workgroup's groups follow one another (`schedule`).
    wrong (f16x3 unless noted): state_not_reset (c and the output registers carry over to a workgroup's next group) |
    planes_not_cleared | reverse_from_T (both kernels: token T - 1 - step) | finished_row_updated (both: a row past its length
    takes steps on the zero row until its group ends) | last_word_zero_row (both: id vocab - 1 reads the zero row) | no_lo_hi |
    table_not_scaled | drain_no_inv_scale.  rows: only these rows, as a batch of their own (a row's arithmetic does not depend
    on its neighbours; not with the two switches that carry state from group to group)."""
    kv = kernel_view(inp, dk)
    dk = kv["dk"]
    tok, ln = inp["tokens"], inp["lengths"]
    if rows is not None:
        assert wrong not in ("state_not_reset", "planes_not_cleared")
        tok, ln = tok[rows], ln[rows]
    b, t_buf = tok.shape
    v = inp["vocab"]
    x3 = precision == "f16x3"
    s = w_hh_scale(inp) if x3 else 1.0
    grid, per_wg = schedule(b, precision, num_cus)
    n_groups = (b + 31) // 32
    bp = n_groups * 32
    tokp = np.zeros((bp, t_buf), np.int64)
    tokp[:b] = tok
    lnp = np.zeros(bp, np.int64)
    lnp[:b] = ln
    hout = np.zeros((2, bp, dk), F32)
    half = dk // 2
    for i in range(2):
        table = kv["table"][i].astype(F32)
        w = kv["w_hh"][i]
        if x3:
            wh, wl = split_f16(w * s)
            blocks = [np.r_[8 * j: 8 * j + 8, half + 8 * j: half + 8 * j + 8] for j in range(dk // 16)]
        prev = None                                              # state the previous pass of the same workgroups left behind
        for p in range(max(len(g) for g in per_wg)):
            groups = [g[p] for g in per_wg if len(g) > p]
            rows = np.concatenate([np.arange(32 * g, 32 * g + 32) for g in groups])
            lens = lnp[rows]
            gmax = np.repeat(lens.reshape(-1, 32).max(1), 32)
            if wrong not in ("state_not_reset", "planes_not_cleared"):     # (the rows that pad the last group compute nothing kept)
                keep = rows < b
                rows, lens, gmax = rows[keep], lens[keep], gmax[keep]
            m = len(rows)
            c, hreg = np.zeros((m, dk), F32), np.zeros((m, dk), F32)
            hi, lo = np.zeros((m, dk)), np.zeros((m, dk))
            if prev is not None and x3:
                if wrong == "state_not_reset":
                    c, hreg = prev[0][:m].copy(), prev[1][:m].copy()
                if wrong == "planes_not_cleared":
                    hi, lo = prev[2][:m].copy(), prev[3][:m].copy()
            hfull = np.zeros((m, dk), F32)                       # the fp32 kernel's h in LDS
            for step in range(int(gmax.max())):
                act = step < lens
                upd = (step < gmax) if wrong == "finished_row_updated" else act
                col = (t_buf - 1 - step) if (i == 1 and wrong == "reverse_from_T") else _step_index(lens, step, i == 1)
                tk = np.where(act, tokp[rows, np.clip(col, 0, t_buf - 1)], v)
                if wrong == "last_word_zero_row":
                    tk = np.where(tk == v - 1, v, tk)
                tab = table[tk]
                if x3:
                    acc = tab if wrong == "table_not_scaled" else _f32(tab.astype(np.float64) * s)
                    pairs = [(hi, wh), (hi, wl)] + ([] if wrong == "no_lo_hi" else [(lo, wh)])
                    for blk in blocks:
                        for x, y in pairs:
                            acc = _f32(acc.astype(np.float64) + x[:, blk] @ y[blk, :])
                    z = acc if wrong == "drain_no_inv_scale" else _f32(acc.astype(np.float64) / s)
                else:
                    acc, a64 = tab.copy(), tab.astype(np.float64)          # fp32 fma: the exact product and sum in float64, one
                    h64, tmp = hfull.astype(np.float64), np.empty_like(a64)  # rounding to fp32 (buffers reused: 2 K steps per call)
                    for j in range(half):
                        for kk in (j, half + j):
                            np.multiply(h64[:, kk: kk + 1], w[kk: kk + 1, :], out=tmp)
                            np.add(tmp, a64, out=tmp)
                            acc[...] = tmp
                            a64[...] = acc
                    z = acc
                ig, fg, og = (_gate_sigmoid(z[:, q * dk: (q + 1) * dk], x3) for q in (0, 1, 3))
                gg = _gate_tanh(z[:, 2 * dk: 3 * dk], x3)
                cn = _f32(fg.astype(np.float64) * c.astype(np.float64) + _f32(ig.astype(np.float64) * gg.astype(np.float64)).astype(np.float64))
                hn = _f32(og.astype(np.float64) * _gate_tanh(cn, x3).astype(np.float64))
                u_ = upd[:, None]
                c, hreg = np.where(u_, cn, c), np.where(u_, hn, hreg)
                if x3:
                    nh, nl = split_f16(hn.astype(np.float64))
                    hi, lo = np.where(u_, nh, hi), np.where(u_, nl, lo)
                else:
                    hfull = np.where(u_, hn, hfull)
            hout[i, rows] = hreg
            prev = (c, hreg, hi, lo)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((hout[0, :b] + hout[1, :b]).astype(F32) / F32(2.0)).astype(F32)


def rownorm_emul(raw):
    """k_rownorm in fp32: x / max(sqrt(sum x^2), 1e-12)."""
    raw = raw.astype(F32)
    ss = (raw.astype(np.float64) ** 2).sum(1, keepdims=True).astype(F32)
    den = np.maximum(np.sqrt(ss).astype(F32), F32(1e-12))
    with np.errstate(invalid="ignore", over="ignore"):
        return (raw / den).astype(F32)
