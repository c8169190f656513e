"""Shared by tests/test_gpu_train_ops.py and tests/test_train_ops_ref_host.py: for every kernel of csrc/train_ops.hip on the cell
branch's training path
  (a) `*_ref64`  a float64 statement of the operation and of its gradient, taking the fp32 inputs as given,
  (b) `*_bounds` a per-element first-order fp32 error bound for the arithmetic the kernel is documented to do (u = 2^-24),
  (c) `*_emul`   an fp32 NumPy emulation of that arithmetic: float64 sums where the kernel sums in float64, fp32 elsewhere,
plus the shapes and the seeded inputs of the tests (computed once per case and handed out read-only).  Plain NumPy: no GPU, no
torch.  The GPU tests assert |kernel - (a)| <= 2 (b) element by element (the 2 covers second-order terms and nothing else); the
host tests prove that (c) stays within 1 (b) of (a) and that `within` rejects deliberately wrong emulations (the `wrong=` switches).

Where a bound is first-order: a result computed as fl(a op b) carries (1 + d), |d| <= u; the bounds below add |d| times the
magnitude of every intermediate value, and the rounding of every float64 quantity that the kernel stores as fp32."""
import functools

import numpy as np

U = 2.0 ** -24          # unit round-off of fp32
U64 = 2.0 ** -53        # of float64
F32 = np.float32
EPS_BN = 1e-5

BN_CHUNK_ROWS = 512     # T2P_BN_CHUNK_ROWS of csrc/train_ops.hip


def bn_chunks(rows, n_seg):
    """Row chunks per segment, as csrc/train_ops.hip's bn_chunks."""
    r = (rows // max(n_seg, 1) + BN_CHUNK_ROWS - 1) // BN_CHUNK_ROWS
    return int(min(max(r, 1), 256))


# (segment sizes, C): what each one reaches is listed in tests/test_gpu_train_ops.py
BN_SHAPES = [([1300, 2, 700], 32), ([1100], 8), ([900, 3, 700], 100), ([2100, 2], 256), ([37, 2, 5], 67), ([1200, 2], 6)]
BN_SEED = 1             # np.random.default_rng: the ReLU margin (bn_relu_margin >= 8) holds for all six shapes, see the host test
SEG_SIZES = [5, 1, 0, 33, 8, 4, 259]
SEG_CHANNELS = [128, 67, 3]
EDGE_SHAPE = dict(E=5000, rows=300, cent=150, hub=3000, silent=100)
EDGE_CHANNELS = [3, 64, 128]
PAIR_SHAPE = dict(E=4000, rows=260, hub_targets=500)
PAIR_DIMS = [256, 300, 64]
ROWNORM_SHAPES = [(1, 64), (7, 256), (130, 300), (5, 3)]


def seg_ptr_of(sizes, first=0):
    return np.concatenate([[first], first + np.cumsum(sizes)]).astype(np.int32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def within(got, ref, bound, factor):
    """Every element of got within factor * bound of ref; where ref is NaN, got must be NaN, where ref is infinite, equal."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    fin = np.isfinite(ref)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return False
    if not np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]):
        return False
    return bool(np.all(np.abs(got[fin] - ref[fin]) <= factor * bound[fin]))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the finite elements of ref (0 / 0 counts as 0)."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound[fin])
    return float(r.max()) if r.size else 0.0


# ---- batch-statistics BatchNorm (+ReLU) over row segments ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bn_inputs(case, seed=BN_SEED):
    """x ~ 2 N(0,1) + 0.5, gamma / beta ~ N(0,1) (negative scales included), dy ~ N(0,1) of BN_SHAPES[case]."""
    sizes, c = BN_SHAPES[case]
    rng = np.random.default_rng(seed)
    m = int(sum(sizes))
    x = (rng.standard_normal((m, c)) * 2.0 + 0.5).astype(F32)
    gamma = rng.standard_normal(c).astype(F32)
    beta = rng.standard_normal(c).astype(F32)
    dy = rng.standard_normal((m, c)).astype(F32)
    return _frozen(x, gamma, beta, dy)


def bn_ref64(x, sizes, gamma, beta, relu, dy=None, eps=EPS_BN):
    """dict of float64 arrays: mean / invstd / var_unbiased [S, C], xhat / pre / y [M, C] and, with dy, dz / dx [M, C],
    dgamma_seg / dbeta_seg [S + 1, C] (row S: the sum over the segments).  NaN and inf propagate as in IEEE arithmetic."""
    x64, g, b = x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    eps = float(F32(eps))
    s, c = len(sizes), x.shape[1]
    o = dict(mean=np.zeros((s, c)), invstd=np.zeros((s, c)), var_unbiased=np.zeros((s, c)), xhat=np.zeros_like(x64),
             n=np.repeat(np.asarray(sizes, np.float64), sizes)[:, None])
    ptr = seg_ptr_of(sizes)
    with np.errstate(invalid="ignore"):
        for i, n in enumerate(sizes):
            xs = x64[ptr[i]: ptr[i + 1]]
            m = xs.mean(0)
            ss = ((xs - m) ** 2).sum(0)
            o["mean"][i], o["invstd"][i] = m, 1.0 / np.sqrt(ss / n + eps)
            o["var_unbiased"][i] = ss / (n - 1) if n > 1 else ss / n
            o["xhat"][ptr[i]: ptr[i + 1]] = (xs - m) * o["invstd"][i]
        o["pre"] = g * o["xhat"] + b
        o["y"] = np.where(o["pre"] <= 0.0, 0.0, o["pre"]) if relu else o["pre"]     # keeps NaN, as torch.relu
        if dy is not None:
            dz = np.where(o["pre"] > 0.0, dy.astype(np.float64), 0.0) if relu else dy.astype(np.float64)
            dgs, dbs, dx = np.zeros((s + 1, c)), np.zeros((s + 1, c)), np.zeros_like(x64)
            for i, n in enumerate(sizes):
                sl = slice(ptr[i], ptr[i + 1])
                dbs[i], dgs[i] = dz[sl].sum(0), (dz[sl] * o["xhat"][sl]).sum(0)
                dx[sl] = g * o["invstd"][i] * (dz[sl] - dbs[i] / n - o["xhat"][sl] * dgs[i] / n)
            dbs[s], dgs[s] = dbs[:s].sum(0), dgs[:s].sum(0)
            o.update(dz=dz, dx=dx, dgamma_seg=dgs, dbeta_seg=dbs)
    return o


def bn_bounds(x, sizes, gamma, beta, ref, dy=None):
    """First-order bounds for the kernels' arithmetic, same keys as bn_ref64 (statistics, y, and with dy: dx, dgamma_seg, dbeta_seg).

    Statistics: s0 = sum x and s1 = sum x^2 are float64 sums of n terms (error <= U64 n sum|term|); m = s0 / n, ss = s1 - s0 m
    (|s0 m| <= s1), var = ss / n: e_mean = U64 sum|x|, e_ss = U64 (2 n + 4) sum x^2; each statistic is then rounded to fp32 once.
    y = fl(fl(fl(fl(x - mean) invstd) gamma) + beta) with t = |gamma| |xhat|:  u (5 t + |beta| + (|mean| + |x|) invstd |gamma|).
    xhat as the backward recomputes it: e_xhat = u (2 |xhat| + (|mean| + |x|) invstd).
    dbeta = fl32(float64 sum of dz): u sum|dz|;  dgamma = fl32(float64 sum of dz xhat_fp32): u sum(|dz| |xhat|) + sum(|dz| e_xhat).
    dx = fl(gamma invstd) (dz - dbeta/n - xhat dgamma/n): six roundings on the three terms, the stored sums' own errors
    (b_dbeta, b_dgamma) and the two roundings of sum * fl(1/n), and e_xhat on the third term.
    Row S of the two tables is a float64 sum of the fp32 rows, rounded once: the rows' bounds added, plus u |total|."""
    x64, g, b = np.abs(x.astype(np.float64)), np.abs(gamma.astype(np.float64)), np.abs(beta.astype(np.float64))
    s = len(sizes)
    ptr = seg_ptr_of(sizes)
    rep = np.repeat(np.arange(s), sizes)
    n_s = np.asarray(sizes, np.float64)[:, None]
    sum_x = np.add.reduceat(x64, ptr[:-1].astype(np.int64), 0) if s else np.zeros((0, x.shape[1]))
    sum_x2 = np.add.reduceat(x64 * x64, ptr[:-1].astype(np.int64), 0) if s else np.zeros((0, x.shape[1]))
    e_mean = U64 * sum_x
    e_var = U64 * (2 * n_s + 4) * sum_x2 / n_s
    o = dict(mean=U * np.abs(ref["mean"]) + e_mean,
             invstd=U * ref["invstd"] + 0.5 * ref["invstd"] ** 3 * e_var,
             var_unbiased=U * ref["var_unbiased"] + e_var * n_s / np.maximum(n_s - 1, 1))
    mean_r, is_r = np.abs(ref["mean"])[rep], ref["invstd"][rep]
    xhat = np.abs(ref["xhat"])
    o["y"] = U * (5 * g * xhat + b + (mean_r + x64) * is_r * g)
    if dy is not None:
        dz, n = np.abs(ref["dz"]), ref["n"]
        e_xhat = U * (2 * xhat + (mean_r + x64) * is_r)
        seg_sum = lambda a: np.add.reduceat(a, ptr[:-1].astype(np.int64), 0)    # noqa: E731  (no empty segments here)
        b_db = U * seg_sum(dz)
        b_dg = U * seg_sum(dz * xhat) + seg_sum(dz * e_xhat)
        dbeta, dgamma = np.abs(ref["dbeta_seg"][:s]), np.abs(ref["dgamma_seg"][:s])
        o["dx"] = g * is_r * (6 * U * (dz + dbeta[rep] / n + xhat * dgamma[rep] / n) + (b_db + 2 * U * dbeta)[rep] / n
                              + xhat * (b_dg + 2 * U * dgamma)[rep] / n + e_xhat * dgamma[rep] / n)
        o["dbeta_seg"] = np.concatenate([b_db, b_db.sum(0, keepdims=True) + U * np.abs(ref["dbeta_seg"][s:])])
        o["dgamma_seg"] = np.concatenate([b_dg, b_dg.sum(0, keepdims=True) + U * np.abs(ref["dgamma_seg"][s:])])
    return o


def bn_relu_margin(ref, bounds):
    """Smallest |float64 pre-activation| / bound_y: the ReLU masks of two fp32 evaluations agree when this is well above 1."""
    with np.errstate(divide="ignore"):
        return float((np.abs(ref["pre"]) / bounds["y"]).min())


def bn_emul(x, sizes, gamma, beta, relu, dy=None, eps=EPS_BN, wrong=None):
    """The kernels' arithmetic in NumPy: float64 chunk sums combined in chunk order, everything else fp32 in the kernels' order.
    wrong: None | "unbiased_var" | "drop_last_chunk" | "mask_ge" | "no_xhat_term" - the deliberately wrong variants."""
    s, c, rows = len(sizes), x.shape[1], x.shape[0]
    chunks = bn_chunks(rows, s)
    ptr = seg_ptr_of(sizes)
    mean, invstd, var_u = (np.zeros((s, c), F32) for _ in range(3))
    for i, n in enumerate(sizes):
        per = (n + chunks - 1) // chunks
        s0, s1 = np.zeros(c), np.zeros(c)
        for z in range(chunks):
            lo = ptr[i] + z * per
            hi = min(lo + per, ptr[i + 1])
            if wrong == "drop_last_chunk" and chunks > 1 and z == chunks - 1:
                continue
            xs = x[lo: max(hi, lo)].astype(np.float64)
            s0 += xs.sum(0)
            s1 += (xs * xs).sum(0)
        with np.errstate(invalid="ignore"):
            m = s0 / n
            ss = np.maximum(s1 - s0 * m, 0.0)                   # (NaN stays NaN, as the kernel's `if (ss < 0) ss = 0`)
            var = ss / n
            mean[i] = m
            invstd[i] = 1.0 / np.sqrt((ss / (n - 1) if wrong == "unbiased_var" and n > 1 else var) + float(F32(eps)))
            var_u[i] = ss / (n - 1) if n > 1 else var
    rep = np.repeat(np.arange(s), sizes)
    with np.errstate(invalid="ignore"):
        xhat = (x - mean[rep]) * invstd[rep]                    # fp32: two roundings
        v = xhat * gamma + beta                                 # two more (-ffp-contract=off)
    o = dict(mean=mean, invstd=invstd, var_unbiased=var_u, y=np.where(v <= 0, F32(0), v) if relu else v)
    if dy is not None:
        keep = (v >= 0 if wrong == "mask_ge" else v > 0) if relu else np.ones(v.shape, bool)
        dz = np.where(keep, dy, F32(0))
        dgs, dbs, dx = np.zeros((s + 1, c), F32), np.zeros((s + 1, c), F32), np.zeros_like(x)
        for i, n in enumerate(sizes):
            sl = slice(ptr[i], ptr[i + 1])
            dbs[i] = dz[sl].astype(np.float64).sum(0)
            dgs[i] = (dz[sl].astype(np.float64) * xhat[sl].astype(np.float64)).sum(0)
            inv_n = F32(1) / F32(n)
            sdz, sdx = dbs[i] * inv_n, dgs[i] * inv_n
            third = F32(0) if wrong == "no_xhat_term" else xhat[sl] * sdx
            dx[sl] = (gamma * invstd[i]) * ((dz[sl] - sdz) - third)
        dbs[s], dgs[s] = dbs[:s].astype(np.float64).sum(0), dgs[:s].astype(np.float64).sum(0)
        o.update(dx=dx, dgamma_seg=dgs, dbeta_seg=dbs)
    return o


def bn_running_ref64(mean, var_unbiased, running_mean, running_var, tracked, momentum):
    """nn.BatchNorm1d's update of the running estimates applied segment by segment in float64: (mean, var, num_batches_tracked)."""
    rm, rv = running_mean.astype(np.float64), running_var.astype(np.float64)
    for i in range(mean.shape[0]):
        tracked += 1
        f = 1.0 / tracked if momentum is None else float(momentum)
        rm, rv = (1 - f) * rm + f * mean[i], (1 - f) * rv + f * var_unbiased[i]
    return rm, rv, tracked


def bn_running_bounds(stat, b_stat, running, tracked, momentum):
    """Bound for one running estimate: the recurrence is linear, r = keep r0 + sum_k w_k stat_k with positive weights, so the
    statistics' own bounds enter with w_k; the closed form is evaluated in fp32 (weights from a power, <= 4 u; one product and up to
    three additions per term, one product and one addition for r0): 8 u on the magnitudes."""
    s = stat.shape[0]
    k = np.arange(s)
    if momentum is None:
        w, keep = np.full(s, 1.0 / (tracked + s)), tracked / (tracked + s)
    else:
        w, keep = momentum * (1 - momentum) ** (s - 1 - k), (1 - momentum) ** s
    return (w[:, None] * b_stat).sum(0) + 8 * U * (keep * np.abs(running) + (w[:, None] * np.abs(stat)).sum(0))


# ---- segment max / segment mean ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def seg_inputs(c, first=0, tail=0):
    """x drawn from the 17 multiples of 0.25 in [-2, 2] (exact ties: the columns of the 259-row segment tie across row lanes) and dout; `first`
    rows before the first segment and `tail` rows behind the last one belong to no segment."""
    rng = np.random.default_rng(100 + c)
    m = first + int(sum(SEG_SIZES)) + tail
    x = (rng.integers(-8, 9, (m, c)) * 0.25).astype(F32)
    dout = rng.standard_normal((len(SEG_SIZES), c)).astype(F32)
    return _frozen(x, dout, seg_ptr_of(SEG_SIZES, first))


def segment_max_ref(x, ptr, wrong=None):
    """(out, arg): NumPy argmax per segment - the first row wins ties, a NaN wins over every number (the first one), an all -inf
    column names its first row; an empty segment gives out = 0, arg = -1.  wrong="last_tie": ties go to the last row."""
    s, c = len(ptr) - 1, x.shape[1]
    out, arg = np.zeros((s, c), F32), np.full((s, c), -1, np.int32)
    for i in range(s):
        xs = x[ptr[i]: ptr[i + 1]]
        if len(xs):
            a = len(xs) - 1 - np.argmax(xs[::-1], 0) if wrong == "last_tie" else np.argmax(xs, 0)
            arg[i], out[i] = ptr[i] + a, xs[a, np.arange(c)]
    return out, arg


def segment_max_backward_ref(dout, arg, rows):
    dx = np.zeros((rows, dout.shape[1]), F32)
    s, c = np.nonzero(arg >= 0)
    dx[arg[s, c], c] = dout[s, c]
    return dx


def segment_mean_ref64(x, ptr, dout=None):
    """(mean [S, C], dx [M, C] or None) in float64; empty segment: 0; rows of no segment: dx = 0."""
    s = len(ptr) - 1
    out, dx = np.zeros((s, x.shape[1])), None if dout is None else np.zeros(x.shape)
    for i in range(s):
        n = ptr[i + 1] - ptr[i]
        if n:
            out[i] = x[ptr[i]: ptr[i + 1]].astype(np.float64).mean(0)
            if dout is not None:
                dx[ptr[i]: ptr[i + 1]] = dout[i].astype(np.float64) / n
    return out, dx


def segment_mean_bounds(x, ptr, dout=None):
    """forward: fl32 of a float64 sum of n terms divided by n: u |mean| + U64 n sum|x| / n;  backward: one fp32 division: 2 u |dout| / n."""
    s = len(ptr) - 1
    ref, _ = segment_mean_ref64(x, ptr)
    b, bdx = np.zeros((s, x.shape[1])), None if dout is None else np.zeros(x.shape)
    for i in range(s):
        n = ptr[i + 1] - ptr[i]
        if n:
            b[i] = U * np.abs(ref[i]) + U64 * n * np.abs(x[ptr[i]: ptr[i + 1]].astype(np.float64)).sum(0) / n
            if dout is not None:
                bdx[ptr[i]: ptr[i + 1]] = 2 * U * np.abs(dout[i].astype(np.float64)) / n
    return b, bdx


def segment_mean_emul(x, ptr, dout=None, wrong=None):
    """wrong="n_minus_1": divides by n - 1."""
    s = len(ptr) - 1
    out, dx = np.zeros((s, x.shape[1]), F32), None if dout is None else np.zeros(x.shape, F32)
    for i in range(s):
        n = int(ptr[i + 1] - ptr[i])
        d = n - 1 if wrong == "n_minus_1" else n
        if n:
            with np.errstate(divide="ignore", invalid="ignore"):
                out[i] = x[ptr[i]: ptr[i + 1]].astype(np.float64).sum(0) / np.float64(d)
                if dout is not None:
                    dx[ptr[i]: ptr[i + 1]] = dout[i] / F32(d)
    return out, dx


# ---- the two message gathers ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_inputs(c):
    """x [300, C], pos [300, 3], pos_c [150, 3], src / dst [5000], d_out [5000, W] with NaN in its pad columns.  Row 7 is the
    source of 3,000 edges, rows 200 .. 299 of none, rows 0 .. 199 share the other 2,000."""
    sh = EDGE_SHAPE
    rng = np.random.default_rng(200 + c)
    e, rows = sh["E"], sh["rows"]
    w = (c + 3 + 7) // 8 * 8
    src = np.concatenate([np.full(sh["hub"], 7), rng.integers(0, rows - sh["silent"], e - sh["hub"])]).astype(np.int32)
    rng.shuffle(src)
    dst = np.sort(rng.integers(0, sh["cent"], e)).astype(np.int32)
    x = rng.standard_normal((rows, c)).astype(F32)
    pos = rng.standard_normal((rows, 3)).astype(F32)
    pos_c = rng.standard_normal((sh["cent"], 3)).astype(F32)
    d_out = rng.standard_normal((e, w)).astype(F32)
    d_out[:, c:] = np.nan                                       # never read: only the first C columns carry a gradient to x
    return _frozen(x, pos, pos_c, src, dst, d_out) + (w,)


def edge_features_forward_ref(x, pos, pos_c, src, dst, w):
    """fp32, exact: a gather and one subtraction."""
    c = x.shape[1]
    out = np.zeros((len(src), w), F32)
    out[:, :c] = x[src]
    out[:, c: c + 3] = pos[src] - pos_c[dst]
    return out


def edge_features_backward_ref64(d_out, src, rows, c):
    """(dx, bound): dx[src[e]] += d_out[e, :C] in float64; fp32 atomics in any order: deg u sum|terms| per element."""
    dx, mag, deg = np.zeros((rows, c)), np.zeros((rows, c)), np.zeros((rows, 1))
    np.add.at(dx, src, d_out[:, :c].astype(np.float64))
    np.add.at(mag, src, np.abs(d_out[:, :c].astype(np.float64)))
    np.add.at(deg, src, 1.0)
    return dx, deg * U * mag


def edge_features_backward_emul(d_out, src, rows, c, wrong=None):
    """fp32 additions in edge order.  wrong="pitch_c": reads d_out with row pitch C instead of W."""
    dx = np.zeros((rows, c), F32)
    terms = d_out.reshape(-1)[: len(src) * c].reshape(len(src), c) if wrong == "pitch_c" else d_out[:, :c]
    np.add.at(dx, src, terms)
    return dx


@functools.lru_cache(maxsize=None)
def pair_inputs(d):
    """x [260, D], tgt / src [4000], d_out [4000, 2 D].  tgt is sorted and made of runs of 1 .. 8 edges, one run per target (as
    train_cell._host_plan builds it; 4,000 edges over 260 rows need about 900 runs, so a row is the target of several runs); the
    first edge of every run is the self edge src == tgt; row 3 is the source of one edge of each of 500 targets."""
    sh = PAIR_SHAPE
    rng = np.random.default_rng(300 + d)
    e, rows = sh["E"], sh["rows"]
    per = rng.integers(1, 9, e)
    cut = int(np.searchsorted(np.cumsum(per), e))               # the first run that reaches E edges: cut short to end there
    per = per[: cut + 1]
    per[-1] -= per.sum() - e
    tgt_rows = rng.integers(0, rows, len(per))
    tgt_rows.sort()
    tgt = np.repeat(tgt_rows, per).astype(np.int32)
    src = rng.integers(0, rows, e).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(per)[:-1]])
    src[first] = tgt[first]
    multi = np.nonzero(per >= 2)[0]
    src[first[multi[: sh["hub_targets"]]] + 1] = 3
    x = rng.standard_normal((rows, d)).astype(F32)
    d_out = rng.standard_normal((e, 2 * d)).astype(F32)
    return _frozen(x, tgt, src, d_out)


def pair_features_forward_ref(x, tgt, src):
    return np.concatenate([x[tgt], x[src] - x[tgt]], 1)


def pair_features_backward_ref64(d_out, tgt, src, rows):
    """(dx, bound): dx[tgt] += dA - dB, dx[src] += dB in float64; deg u sum|terms| per element plus u |dA - dB| per subtraction."""
    d = d_out.shape[1] // 2
    da, db = d_out[:, :d].astype(np.float64), d_out[:, d:].astype(np.float64)
    dx, mag, sub, deg = np.zeros((rows, d)), np.zeros((rows, d)), np.zeros((rows, d)), np.zeros((rows, 1))
    np.add.at(dx, tgt, da - db)
    np.add.at(dx, src, db)
    np.add.at(mag, tgt, np.abs(da - db))
    np.add.at(mag, src, np.abs(db))
    np.add.at(sub, tgt, np.abs(da - db))
    np.add.at(deg, tgt, 1.0)
    np.add.at(deg, src, 1.0)
    return dx, deg * U * mag + U * sub


def pair_features_backward_emul(d_out, tgt, src, rows, wrong=None):
    """wrong="sum_to_target": adds dA + dB to the target."""
    d = d_out.shape[1] // 2
    da, db = d_out[:, :d], d_out[:, d:]
    dx = np.zeros((rows, d), F32)
    np.add.at(dx, tgt, da + db if wrong == "sum_to_target" else da - db)
    np.add.at(dx, src, db)
    return dx


# ---- backward of F.normalize ---------------------------------------------------------------------------------------------------------

ROWNORM_EPS = float(F32(1e-12))


@functools.lru_cache(maxsize=None)
def rownorm_inputs(n_rows, dim):
    """x, dy [n_rows, dim] with row norms from 1e-3 to 1e3 and, from three rows on, the special rows
    (row n-1: x = 0; row n-2: dy = 3 x, pure cancellation; row n-3: dy orthogonal to x up to its fp32 rounding)."""
    rng = np.random.default_rng(400 + 7 * n_rows + dim)
    x = rng.standard_normal((n_rows, dim))
    norms = np.ones(n_rows)
    if n_rows >= 3:
        norms[: n_rows - 1] = 10.0 ** np.linspace(-3, 3, n_rows - 1)      # (the last row becomes the all-zero one)
    x *= norms[:, None] / np.linalg.norm(x, axis=1, keepdims=True)
    x = x.astype(F32)
    dy = rng.standard_normal((n_rows, dim)).astype(F32)
    special = {}
    if n_rows >= 3:
        special = dict(zero=n_rows - 1, cancel=n_rows - 2, orthogonal=n_rows - 3)
        x[special["zero"]] = 0
        dy[special["cancel"]] = F32(3) * x[special["cancel"]]
        xo, do = x[special["orthogonal"]].astype(np.float64), dy[special["orthogonal"]].astype(np.float64)
        dy[special["orthogonal"]] = do - xo * (xo @ do) / (xo @ xo)
    return _frozen(x, dy) + (special,)


def rownorm_backward_ref64(x, dy):
    """(dx, bound) of dx = (dy - x proj) inv, inv = 1 / max(|x|, eps), proj = <x, dy> inv^2, eps = fl32(1e-12).

    The kernel sums x^2 and x dy in fp32: ceil(dim / 64) terms per lane, then six butterfly stages; with the products' own
    rounding, k = ceil(dim / 64) + 6 + 1 roundings, each at most u sum|products|:  e_ss = k u sum x^2, e_dot = k u sum|x dy|.
    nrm = fl(sqrt(ss)), inv = fl(1 / nrm): relative error r_inv = e_ss / (2 ss) + 2 u (an all-zero row takes the clamp: u).
    proj = fl(fl(dot inv) inv): e_proj = e_dot inv^2 + |proj| (2 r_inv + 2 u).
    dx = fl(fl(dy - fl(x proj)) inv): |x| e_proj + u |x proj| from the product, then (r_inv + 2 u) on (|dy| + |x| |proj|) - not on
    the cancelled difference -, all times inv: an absolute bound in units of (|dy| + |x| |proj|) / |x|."""
    x64, d64 = x.astype(np.float64), dy.astype(np.float64)
    dim = x.shape[1]
    k = (dim + 63) // 64 + 7
    ss, dot = (x64 * x64).sum(1, keepdims=True), (x64 * d64).sum(1, keepdims=True)
    nrm = np.maximum(np.sqrt(ss), ROWNORM_EPS)
    inv = 1.0 / nrm
    proj = dot * inv * inv
    dx = (d64 - x64 * proj) * inv
    r_inv = np.where(ss > 0, k * U / 2, 0.0) + 2 * U
    e_proj = k * U * np.abs(x64 * d64).sum(1, keepdims=True) * inv * inv + np.abs(proj) * (2 * r_inv + 2 * U)
    ax, scale = np.abs(x64), np.abs(d64) + np.abs(x64) * np.abs(proj)
    bound = inv * (ax * e_proj + U * ax * np.abs(proj) + (r_inv + 2 * U) * scale)
    return dx, bound


def rownorm_backward_emul(x, dy, wrong=None):
    """One wavefront per row: lane l adds columns l, l + 64, .. in fp32, six xor-butterfly stages (fp32 addition commutes, so every
    lane ends with the same bits), then fp32 throughout.  wrong="no_projection": dx = dy inv."""
    n, dim = x.shape
    pad = (-dim) % 64

    def wave_sum(p):
        p = np.concatenate([p, np.zeros((n, pad), F32)], 1).reshape(n, -1, 64)
        acc = np.zeros((n, 64), F32)
        for j in range(p.shape[1]):
            acc = acc + p[:, j]
        w = 64
        while w > 1:
            w //= 2
            acc = acc[:, :w] + acc[:, w: 2 * w]
        return acc
    ss, dot = wave_sum(x * x), wave_sum(x * dy)
    nrm = np.maximum(np.sqrt(ss), F32(1e-12))
    inv = F32(1) / nrm
    proj = F32(0) * dot if wrong == "no_projection" else dot * inv * inv
    return (dy - x * proj) * inv
