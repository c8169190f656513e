"""Shared by tests/test_gpu_text_train.py and tests/test_text_train_ref_host.py: the two pieces of the coarse training step that
the other yardsticks leave out, in the manner of lstm_ref.py, train_ops_ref.py and gemm_ref.py (whose gamma, U, within,
worst_ratio, bits_equal, FACTOR_GPU and skinny_emul are used here, not restated):
  A  the ranking losses  t2p_pairwise_ranking / t2p_hardest_ranking  (csrc/small_kernels.hip: k_rank_rows, k_rank_diag,
     k_hardest_scan, k_hardest_grad),
  B  the per-step training LSTM kernels  t2p_lstm_cell_forward / _backward  (csrc/lstm.hip: k_lstm_cell_fwd, k_lstm_cell_bwd),
  C  the in-library time loops  t2p_lstm_train_forward / _backward  (csrc/api.hip; products on tg_gemm.hip::k_gemm_skinny),
  D  modules._LstmTrainFn end to end at a width the loops refuse (products on the tiled t2p_gemm through ops.matmul).
For each: seeded inputs (computed once per case, read-only), a float64 statement on the fp32 inputs as given, a per-element bound
carried beside it, an fp32 emulation of the kernel's documented order with `wrong=` switches (one plausible defect each - in the
emulation only), and ONE check function that the GPU test applies to the kernel and the host test to the emulations.
Plain NumPy: no GPU, no torch.

A.  margin is the fp32 value the ABI receives.  With d = the diagonal, cost_s[i][j] = max(0, (margin - S[j][j]) + S[i][j]) and
cost_im[i][j] = max(0, (margin - S[i][i]) + S[i][j]) off the diagonal; the hardest loss forms (margin + S) - d.  Each hinge x is
two fp32 roundings: e = u (|first sum| + |x|); max(0, .) and a maximum over candidates are 1-Lipschitz.  A row loss adds
2 (B - 1) hinges in some order: sum e + gamma_(2(B-1)) sum|hinge|.  A gradient entry off the diagonal is count fl(1 / B) with
count in {0, 1, 2}, the pairwise diagonal one correctly rounded division -(count) / B: both equal the float64 value rounded once
unless 1 / B sits on a rounding boundary (the host test rules that out for every B used), so gradients, counts and positions are
compared EXACTLY.  That means something only where no hinge lies within FACTOR_GPU bounds of zero (and, for the hardest loss, the
winner within FACTOR_GPU bounds of the runner-up): `near` counts such entries, and the seeds are chosen so that it is 0.
Rules pinned (include/t2p.h): a hinge counts only where it is > 0 (gradient 0 at an exact hinge, where the reference's
element-wise torch.max(zeros, x) has 1/2); the first of equal maxima wins; a NaN hinge stays NaN (best = NaN, where = the first
position that holds one); values of d_scores where a NaN took part are free, but written.
Exact family: scores multiples of 2^-10 in [-1, 1], margin 0.375 = 384 2^-10: every hinge is a multiple of 2^-10 of magnitude
<= 2.375 and a row sum of 2 (B - 1) of them stays below 2^24 2^-10 = 2^14 while 4.75 (B - 1) < 2^14, B <= 3,450: every fp32
operation is exact in any order and every output must equal the float64 one rounded once, bit for bit.

B, C.  One step, float64 z = pre + table[token] with bound dz (u |z| for the sum; in C also the recurrent product's
|W|^T dh + gamma_(K+2) (|h| + dh) |W| + u |pre| of gemm_ref.gemm_bound, any order):
  gates   di, df, do = dz / 4 + EPS_GATE,  dg = dz + EPS_GATE                                   (lstm_ref.py's header)
  cell    dc' = |f| dc + |c| df + df dc + |i| dg + |g| di + di dg + 2 u (1 + u) (F + G)
  hidden  dt = dc' + EPS_GATE,  dh' = |o| dt + |t| do + do dt + u (|o| + do)(|t| + dt)
Backward of a step: every output is a product of factors x_k known to e_k, rounded n times:
  |fl(prod) - prod| <= sum_k e_k prod_(j<k) |x_j| prod_(j>k) (|x_j| + e_j) + gamma_n prod (|x_j| + e_j)       (`_pb`)
with dh = dh_gemm + carry (one rounding; dh_gemm = d_pre W_hh on the few-rows kernel, K = 4 D), tc = tanhf(c) to EPS_GATE,
1 - tc^2 and 1 - g to their own roundings, dct = dc + dh o (1 - tc^2).  The build keeps products and sums apart
(-ffp-contract=off), which the emulations follow.  EPS_GATE is lstm_ref's 2e-7: the training kernels use 1 / (1 + expf(-x)) and the
library tanhf; test_gate_functions_in_isolation measures both through the ABI (docs/notebook.md records it).
In C the backward takes gates, cs, dh_last and W_hh as exact fp32 arrays (made from the float64 forward, rounded).

D composes these (`fallback_ref64`): the gate table carries gemm_bound of E W_ih^T plus the roundings of the bias sum, the backward
step takes the gates and cell states to their forward bounds, and each weight-gradient product adds gemm_ref.tn_bound on the
magnitudes to the parts its operands carry (`_tn`); the bias gradient is an fp32 sum of V rows in some order."""
import functools

import numpy as np

import lstm_ref as LR
from gemm_ref import F32, FACTOR_GPU, U, bits_equal, gamma, skinny_emul, within, worst_ratio  # noqa: F401
from lstm_ref import CAP, EPS_GATE, sigmoid64  # noqa: F401

SENTINEL = F32(-12345.671875)       # what the tests prefill every output with: no kernel result equals it
SENTINEL_I = np.int32(-777)
MARGIN = F32(0.35)
MARGIN_EXACT = F32(0.375)
RANK_SIZES = [1, 2, 255, 256, 257, 513]
RANK_SEEDS = {1: 0, 2: 0, 255: 0, 256: 0, 257: 0, 513: 0}     # near == 0 for both losses: test_near_hinge_share_is_zero
RANK_NAN_SIZES = [2, 257]
RANK_NAN_KINDS = ["off_diagonal", "diagonal", "row_and_column"]
RANK_WRONG = ["hinge_ge", "diag_counted", "both_costs_use_row_diag", "mean_over_pairs", "nan_dropped"]
HARDEST_WRONG = ["hardest_tie_to_last", "hardest_diag_included", "hardest_col_as_row", "hardest_grad_no_diag", "nan_dropped"]
LSTM_WRONG = ["finished_row_updated", "reverse_from_T", "gates_not_zeroed_past_end", "carry_dropped", "dc_not_carried",
              "g_and_o_swapped", "tanh_of_c_prev", "forget_grad_uses_c", "dh_gemm_read_at_last_step", "initial_state_overwritten"]


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _same(got, want, free=None):
    """NaN where want is NaN and nowhere else, the same bits elsewhere; elements under `free` are not looked at."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    keep = np.ones(want.shape, bool) if free is None else ~free
    g, w = got[keep], want[keep]
    if g.dtype.kind != "f":
        return bool(np.array_equal(g, w))
    ng, nw = np.isnan(g), np.isnan(w)
    return bool(np.array_equal(ng, nw) and np.array_equal(g[~nw].view(np.int32), w[~nw].astype(F32).view(np.int32)))


def _written(*arrays):
    return all(not np.any(np.asarray(a) == (SENTINEL_I if np.asarray(a).dtype.kind == "i" else SENTINEL)) for a in arrays)


# ---- A: ranking losses, inputs -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rank_scores(b, seed=None, dim=8):
    """[B][B] fp32: products of L2-normalised random rows, the positives correlated with their anchors.  dim = 8 spreads the
    off-diagonal scores (sigma 0.35) so that about one hinge in eight is above 0 and the row sums have many terms."""
    rng = np.random.default_rng([RANK_SEEDS[b] if seed is None else seed, b])
    im = rng.standard_normal((b, dim))
    s = 0.7 * im + 0.6 * rng.standard_normal((b, dim))
    im /= np.sqrt((im * im).sum(1, keepdims=True))
    s /= np.sqrt((s * s).sum(1, keepdims=True))
    out = (im @ s.T).astype(F32)
    out.setflags(write=False)
    return out


# rows / columns / positions of rank_exact_scores' plants (B >= 255)
X_ROW_NONE, X_COL_NONE = 3, 5                   # no positive hinge: best = 0, where = -1
X_ROW_TIE, X_COL_TIE = 11, 17                   # equal maxima in different lanes, at X_TIE
X_TIE = (40, 200)
X_ROW_STRIDE, X_COL_STRIDE = 13, 19             # equal maxima in one lane's stride, at 0 and 256 (B >= 257)
X_ZERO_S, X_ZERO_IM = (21, 23), (25, 27)        # cost_s / cost_im exactly 0 there


@functools.lru_cache(maxsize=None)
def rank_exact_scores(b, seed=0):
    """[B][B] fp32, multiples of 2^-10 in [-1, 1], diagonal in [1/4, 1], with the plants listed above (B = 2: both off-diagonal
    entries are exact hinges: S[0][1] = S[1][1] - margin, S[1][0] = S[1][1] - margin)."""
    rng = np.random.default_rng([seed, b, 1])
    s = rng.integers(-1024, 1025, (b, b)) / 1024.0
    s[np.arange(b), np.arange(b)] = rng.integers(256, 1025, b) / 1024.0
    m = float(MARGIN_EXACT)
    if b == 2:
        s[0, 1] = s[1, 1] - m
        s[1, 0] = s[1, 1] - m
    elif b >= 255:
        off = ~np.eye(b, dtype=bool)
        for r, cols in ((X_ROW_TIE, X_TIE), (X_ROW_STRIDE, (0, 256))):
            if max(cols) < b:
                s[r, off[r]] = np.minimum(s[r, off[r]], 0.875)
                s[r, list(cols)] = 0.9375
        for c, rows in ((X_COL_TIE, X_TIE), (X_COL_STRIDE, (0, 256))):
            if max(rows) < b:
                s[off[:, c], c] = np.minimum(s[off[:, c], c], 0.875)
                s[list(rows), c] = 0.9375
        s[X_ROW_NONE, off[X_ROW_NONE]] = np.minimum(s[X_ROW_NONE, off[X_ROW_NONE]], 0.5)
        s[off[:, X_COL_NONE], X_COL_NONE] = np.minimum(s[off[:, X_COL_NONE], X_COL_NONE], 0.5)
        s[X_ROW_NONE, X_ROW_NONE] = s[X_COL_NONE, X_COL_NONE] = 1.0
        s[X_ROW_NONE, 7] = s[9, X_COL_NONE] = 0.625             # an exact hinge in the row / column that has none above 0
        (i, j), (k, l) = X_ZERO_S, X_ZERO_IM
        s[i, j] = s[j, j] - m
        s[k, l] = s[k, k] - m
    out = s.astype(F32)
    assert np.array_equal(out.astype(np.float64), s)
    out.setflags(write=False)
    return out


def exact_headroom(b):
    """The largest magnitude a row's partial sum can reach, in units of the exact family's 2^-10: must stay below 2^24."""
    return 2 * (b - 1) * (float(MARGIN_EXACT) + 2.0) * 1024.0


@functools.lru_cache(maxsize=None)
def rank_nan_scores(b, kind):
    """rank_exact_scores(b) with NaN planted: one off the diagonal, one on it, or a whole row and column."""
    s = rank_exact_scores(b).copy()
    r = 1 if b == 2 else 130
    if kind == "off_diagonal":
        s[r, 0] = np.nan
    elif kind == "diagonal":
        s[r, r] = np.nan
    else:
        s[r, :] = np.nan
        s[:, r] = np.nan
    s.setflags(write=False)
    return s


# ---- A: float64 statements and bounds ---------------------------------------------------------------------------------------------------

def _hinge(x):
    with np.errstate(invalid="ignore"):
        return np.where(x <= 0.0, 0.0, x)       # keeps NaN, as torch.max(zeros, x) and torch.relu


def rank_ref64(s, margin):
    """PairwiseRankingLoss (training/losses.py:139-164) on the fp32 scores as given.  dict(row_loss [B] (loss = sum / B), row_count
    [B] = the row's cost_im terms above 0, d_scores [B][B] diagonal included, b_row_loss the bound, near = off-diagonal entries
    with a hinge within FACTOR_GPU bounds of 0, free_d / free_count = where a NaN took part)."""
    s64, m = s.astype(np.float64), float(F32(margin))
    b = len(s64)
    d = np.diag(s64)
    eye = np.eye(b, dtype=bool)
    with np.errstate(invalid="ignore"):
        fs, fi = np.broadcast_to((m - d)[None, :], (b, b)), np.broadcast_to((m - d)[:, None], (b, b))
        cs, ci = fs + s64, fi + s64
        hs, hi = np.where(eye, 0.0, _hinge(cs)), np.where(eye, 0.0, _hinge(ci))
        act_s, act_i = (cs > 0.0) & ~eye, (ci > 0.0) & ~eye
        es, ei = np.where(eye, 0.0, U * (np.abs(fs) + np.abs(cs))), np.where(eye, 0.0, U * (np.abs(fi) + np.abs(ci)))
        near = int((((np.abs(cs) <= FACTOR_GPU * es) | (np.abs(ci) <= FACTOR_GPU * ei)) & ~eye).sum())
        es, ei = np.where(cs < -FACTOR_GPU * es, 0.0, es), np.where(ci < -FACTOR_GPU * ei, 0.0, ei)    # 0 on both sides: no error
        row_loss = hs.sum(1) + hi.sum(1)
        bound = es.sum(1) + ei.sum(1) + gamma(max(2 * (b - 1), 1)) * (np.abs(hs).sum(1) + np.abs(hi).sum(1))
    ds = (act_s.astype(np.float64) + act_i) / b
    ds[eye] = -(act_s.sum(0) + act_i.sum(1)).astype(np.float64) / b
    nan_s, nan_i = np.isnan(cs) & ~eye, np.isnan(ci) & ~eye
    free_d = nan_s | nan_i
    free_d[eye] = nan_s.any(0) | nan_i.any(1)
    return dict(row_loss=row_loss, row_count=act_i.sum(1).astype(np.float64), d_scores=ds, b_row_loss=bound, near=near,
                free_d=free_d, free_count=nan_i.any(1))


def hardest_ref64(s, margin):
    """HardestRankingLoss (training/losses.py:173-200).  dict(best [2B] rows then columns, where [2B] int32 (-1: nothing above 0),
    d_scores [B][B], b_best, near = rows / columns whose winner is within FACTOR_GPU bounds of the runner-up or of 0, free_d)."""
    s64, m = s.astype(np.float64), float(F32(margin))
    b = len(s64)
    d = np.diag(s64)
    eye2 = np.concatenate([np.eye(b, dtype=bool)] * 2)
    with np.errstate(invalid="ignore"):
        first = np.concatenate([m + s64, m + s64.T])                        # [2B][B]: row a, then column a, over k
        h = first - np.concatenate([d, d])[:, None]
        e = np.where(eye2, 0.0, U * (np.abs(first) + np.abs(h)))
        hg = np.where(eye2, 0.0, _hinge(h))
        e_all, e = e, np.where(h < -FACTOR_GPU * e, 0.0, e)                 # a hinge that is 0 on both sides carries no error
    isn = np.isnan(hg)
    has_nan = isn.any(1)
    clean = np.where(isn, 0.0, hg)
    best = clean.max(1) if b else np.zeros(0)
    where = np.where(best > 0.0, clean.argmax(1), -1).astype(np.int32) if b else np.zeros(0, np.int32)
    where = np.where(has_nan, isn.argmax(1), where).astype(np.int32)
    best = np.where(has_nan, np.nan, best)
    emax = np.where(isn, 0.0, e).max(1) if b else np.zeros(0)
    second = np.sort(clean, 1)[:, -2] if b >= 2 else np.zeros(2 * b)        # (0 if there is one candidate: the diagonal's 0)
    with np.errstate(invalid="ignore"):
        at_zero = ((np.abs(h) <= FACTOR_GPU * e_all) & ~eye2).any(1)            # matters only where nothing is clearly above 0
        near = int((~has_nan & np.where(best > 0.0, best - second <= 2 * FACTOR_GPU * emax, at_zero)).sum())
    ds = np.zeros((b, b))
    for blk in range(2 * b):
        a, w = blk % b, int(where[blk])
        if w >= 0:
            ds[(a, w) if blk < b else (w, a)] += 1.0
            ds[a, a] -= 1.0
    free_d = has_nan[:b, None] | has_nan[None, b:]
    return dict(best=best, where=where, d_scores=ds / max(b, 1), b_best=emax, near=near, free_d=free_d)


def rank_check(got, ref, exact, factor):
    """got: dict(row_loss, row_count, d_scores) of a kernel or an emulation.  (ok, why)."""
    if not _written(got["row_loss"], got["row_count"], got["d_scores"]):
        return False, "an output element was not written"
    if exact:
        if not _same(got["row_loss"], ref["row_loss"]):
            return False, "row_loss is not the float64 value rounded once"
    elif not within(got["row_loss"], ref["row_loss"], ref["b_row_loss"], factor):
        return False, "row_loss beyond %g x bound (worst ratio %.3g)" % (factor, worst_ratio(got["row_loss"], ref["row_loss"], ref["b_row_loss"]))
    if not _same(got["row_count"], ref["row_count"], ref["free_count"]):
        return False, "row_count"
    if not _same(got["d_scores"], ref["d_scores"], ref["free_d"]):
        return False, "d_scores is not count / B rounded once"
    return True, ""


def hardest_check(got, ref, exact, factor):
    """got: dict(best, where, d_scores).  (ok, why)."""
    if not _written(got["best"], got["where"], got["d_scores"]):
        return False, "an output element was not written"
    if exact:
        if not _same(got["best"], ref["best"]):
            return False, "best is not the float64 value rounded once"
    elif not within(got["best"], ref["best"], ref["b_best"], factor):
        return False, "best beyond %g x bound (worst ratio %.3g)" % (factor, worst_ratio(got["best"], ref["best"], ref["b_best"]))
    if not np.array_equal(np.asarray(got["where"]), ref["where"]):
        return False, "where"
    if not _same(got["d_scores"], ref["d_scores"], ref["free_d"]):
        return False, "d_scores is not count / B rounded once"
    return True, ""


# ---- A: emulations -------------------------------------------------------------------------------------------------------------------------

def _f32(x):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.asarray(x, np.float64).astype(F32)


def _add(x, y):
    with np.errstate(invalid="ignore", over="ignore"):
        return _f32(np.asarray(x, F32).astype(np.float64) + np.asarray(y, F32).astype(np.float64))


def _mul(x, y):
    with np.errstate(invalid="ignore", over="ignore"):
        return _f32(np.asarray(x, F32).astype(np.float64) * np.asarray(y, F32).astype(np.float64))


def _block_sum(terms):
    """[rows][n] fp32 -> [rows]: thread t adds elements t, t + 256, .. in order from 0, then the LDS tree 128, 64, .. 1."""
    rows, n = terms.shape
    pad = (-n) % 256
    t = np.concatenate([terms, np.zeros((rows, pad), F32)], 1).reshape(rows, -1, 256)
    acc = np.zeros((rows, 256), F32)
    for c in range(t.shape[1]):
        acc = _add(acc, t[:, c])
    s = 128
    while s > 0:
        acc[:, :s] = _add(acc[:, :s], acc[:, s: 2 * s])
        s //= 2
    return acc[:, 0]


def rank_emul(s, margin, wrong=None):
    """k_rank_rows + k_rank_diag in fp32: cs = (margin - S[j][j]) + S[i][j], ci = (margin - S[i][i]) + S[i][j], a thread's sum takes
    fl(hinge(cs) + hinge(ci)) per column, inv = fl(1 / B), the diagonal -(column count + row count) / B.
    wrong: hinge_ge | diag_counted | both_costs_use_row_diag | mean_over_pairs | nan_dropped."""
    s = np.asarray(s, F32)
    b = len(s)
    m = F32(margin)
    d = np.diag(s).copy()
    skip = np.zeros((b, b), bool) if wrong == "diag_counted" else np.eye(b, dtype=bool)
    dj = np.broadcast_to(d[:, None] if wrong == "both_costs_use_row_diag" else d[None, :], (b, b))
    cs, ci = _add(_add(m, -dj), s), _add(_add(m, -np.broadcast_to(d[:, None], (b, b))), s)
    with np.errstate(invalid="ignore"):
        if wrong == "nan_dropped":
            hs, hi = np.fmax(cs, F32(0)), np.fmax(ci, F32(0))
        else:
            hs, hi = np.where(cs <= 0, F32(0), cs), np.where(ci <= 0, F32(0), ci)
        act_s, act_i = ((cs >= 0) if wrong == "hinge_ge" else (cs > 0)) & ~skip, ((ci >= 0) if wrong == "hinge_ge" else (ci > 0)) & ~skip
    row_loss = _block_sum(np.where(skip, F32(0), _add(hs, hi)))
    row_cnt = _block_sum(act_i.astype(F32))
    n = F32(b) * F32(b) if wrong == "mean_over_pairs" else F32(b)
    ds = _mul(act_s.astype(F32) + act_i.astype(F32), F32(1.0) / n) if b else np.zeros((0, 0), F32)
    col_cnt = _block_sum(act_s.T.astype(F32))
    if b:
        ds[np.arange(b), np.arange(b)] = -(col_cnt + row_cnt) / n
    return dict(row_loss=row_loss, row_count=row_cnt, d_scores=ds)


def hardest_emul(s, margin, wrong=None):
    """k_hardest_scan + k_hardest_grad in fp32: h = (margin + S) - d; a candidate replaces the kept one only if it is larger (the
    lanes' and the tree's tie rule together: the lowest index among equal maxima), a NaN replaces every number and stays.
    wrong: hardest_tie_to_last | hardest_diag_included | hardest_col_as_row | hardest_grad_no_diag | nan_dropped."""
    s = np.asarray(s, F32)
    b = len(s)
    m = F32(margin)
    d = np.diag(s).copy()
    cols = s if wrong == "hardest_col_as_row" else s.T
    h = _add(_add(m, np.concatenate([s, cols])), -np.concatenate([d, d])[:, None])
    skip = np.zeros((2 * b, b), bool) if wrong == "hardest_diag_included" else np.concatenate([np.eye(b, dtype=bool)] * 2)
    isn = np.isnan(h) & ~skip
    if wrong == "nan_dropped":
        isn[:] = False
    with np.errstate(invalid="ignore"):
        cand = np.where(skip | np.isnan(h) | ~(h > 0), F32(0), h)
    best = cand.max(1)
    arg = (b - 1 - cand[:, ::-1].argmax(1)) if wrong == "hardest_tie_to_last" else cand.argmax(1)
    where = np.where(best > 0, arg, -1)
    where = np.where(isn.any(1), isn.argmax(1), where).astype(np.int32)
    best = np.where(isn.any(1), F32(np.nan), best).astype(F32)
    cnt = np.zeros((b, b), F32)
    for blk in range(2 * b):
        a, w = blk % b, int(where[blk])
        if w >= 0:
            cnt[(a, w) if blk < b else (w, a)] += 1
            if wrong != "hardest_grad_no_diag":
                cnt[a, a] -= 1
    return dict(best=best, where=where, d_scores=_mul(cnt, F32(1.0) / F32(max(b, 1))))


# ---- B: one step of the training LSTM ----------------------------------------------------------------------------------------------------

CELL_DIMS = [1, 3, 6, 64, 300]
CELL_BATCHES = [1, 5, 130]
CELL_T = 4
CELL_VOCAB = 9


def _fwd_step(z, dz, c, dc, d):
    """float64 gates [n][4d], c', h' and their bounds from the pre-activations z known to dz and the cell state c known to dc."""
    zi, zf, zg, zo = (z[:, q * d: (q + 1) * d] for q in range(4))
    di, df, dg, do = (dz[:, q * d: (q + 1) * d] * (1.0 if q == 2 else 0.25) + EPS_GATE for q in range(4))
    ig, fg, gg, og = sigmoid64(zi), sigmoid64(zf), np.tanh(zg), sigmoid64(zo)
    cn = fg * c + ig * gg
    f_, g_ = (fg + df) * (np.abs(c) + dc), (ig + di) * (np.abs(gg) + dg)
    dcn = fg * dc + np.abs(c) * df + df * dc + ig * dg + np.abs(gg) * di + di * dg + 2 * U * (1 + U) * (f_ + g_)
    t = np.tanh(cn)
    dt = dcn + EPS_GATE
    hn = og * t
    dhn = og * dt + np.abs(t) * do + do * dt + U * (og + do) * (np.abs(t) + dt)
    return (np.concatenate([ig, fg, gg, og], 1), np.concatenate([di, df, dg, do], 1), cn, dcn, hn, dhn)


def _token_col(ln, step, reverse, t_buf, wrong=None):
    if reverse and wrong == "reverse_from_T":
        return np.full(len(ln), t_buf - 1 - step)
    return np.clip(ln - 1 - step, 0, t_buf - 1) if reverse else np.minimum(step, t_buf - 1) + 0 * ln


def cell_fwd_ref64(pre, table, tokens, lengths, step, reverse, c_prev, h_prev):
    """dict(gates [B][4D], c, h [B][D]) float64 and b_gates, b_c, b_h.  Rows with step >= length: the state as given, zero gates,
    zero bounds (bit for bit)."""
    b, d = c_prev.shape
    live = (step < lengths)[:, None]
    tok = tokens[np.arange(b), _token_col(lengths, step, reverse, tokens.shape[1])]
    z = pre.astype(np.float64) + table.astype(np.float64)[tok]
    g, dg, c, dc, h, dh = _fwd_step(z, U * np.abs(z), c_prev.astype(np.float64), np.zeros((b, d)), d)
    return dict(gates=np.where(live, g, 0.0), b_gates=np.where(live, dg, 0.0), c=np.where(live, c, c_prev), b_c=np.where(live, dc, 0.0),
                h=np.where(live, h, h_prev), b_h=np.where(live, dh, 0.0), live=live[:, 0])


def cell_fwd_emul(pre, table, tokens, lengths, step, reverse, c_prev, h_prev, wrong=None):
    """k_lstm_cell_fwd in fp32: z = pre + table[token]; 1 / (1 + expf(-z)), tanhf; c' = fl(fl(f c) + fl(i g)); h' = fl(o tanhf(c')).
    wrong: finished_row_updated | reverse_from_T | gates_not_zeroed_past_end | g_and_o_swapped."""
    b, d = c_prev.shape
    live = (step < lengths)[:, None]
    tok = tokens[np.arange(b), _token_col(lengths, step, reverse, tokens.shape[1], wrong)]
    z = _add(pre, table[tok])
    gi, gf, go = (LR._gate_sigmoid(z[:, q * d: (q + 1) * d], False) for q in (0, 1, 3))
    gg = LR._gate_tanh(z[:, 2 * d: 3 * d], False)
    cn = _add(_mul(gf, c_prev), _mul(gi, gg))
    hn = _mul(go, LR._gate_tanh(cn, False))
    gates = np.concatenate([gi, gf, go, gg] if wrong == "g_and_o_swapped" else [gi, gf, gg, go], 1)
    upd = np.ones_like(live) if wrong == "finished_row_updated" else live
    keep_g = np.ones_like(live) if wrong == "gates_not_zeroed_past_end" else live
    return dict(gates=np.where(keep_g, gates, F32(0)), c=np.where(upd, cn, c_prev), h=np.where(upd, hn, h_prev))


def _pb(xs, es, n):
    """Bound on |fl(prod x~_k) - prod x_k| with |x~_k - x_k| <= es[k] and n roundings (module text)."""
    a = [np.abs(x) for x in xs]
    tot = 0.0
    for k in range(len(xs)):
        term = es[k]
        for j in range(len(xs)):
            if j < k:
                term = term * a[j]
            elif j > k:
                term = term * (a[j] + es[j])
        tot = tot + term
    full = 1.0
    for j in range(len(xs)):
        full = full * (a[j] + es[j])
    return tot + gamma(n) * full


def _bwd_step(dh, e_dh, dc, e_dc, gates, c_prev, c, live, d, e_gates=None, e_cp=0.0, e_c=0.0):
    """float64 d_pre [n][4d], dc_out, dh_carry_out with bounds; gates / c_prev / c are exact inputs unless their bounds are given."""
    gi, gf, gg, go = (gates[:, q * d: (q + 1) * d] for q in range(4))
    e_i, e_f, e_g, e_o = (0.0, 0.0, 0.0, 0.0) if e_gates is None else (e_gates[:, q * d: (q + 1) * d] for q in range(4))
    tc = np.tanh(c)
    e_tc = EPS_GATE + e_c + 0.0 * tc

    def one_minus(x, e):                        # fl(1 - x~): the operand's error and one rounding
        return 1.0 - x, e + U * (np.abs(1.0 - x) + e)

    def square(x, e):                           # fl(x~ x~)
        err = 2 * np.abs(x) * e + e * e
        return x * x, err + U * (x * x + err)

    one, e_one = one_minus(*square(tc, e_tc))
    q = dh * go * one
    e_q = _pb([dh, go, one], [e_dh, e_o, e_one], 2)
    dct = dc + q
    e_dct = e_dc + e_q + U * (np.abs(dct) + e_dc + e_q)
    (og_i, e_og_i), (og_f, e_og_f), (og_o, e_og_o) = one_minus(gi, e_i), one_minus(gf, e_f), one_minus(go, e_o)
    og_g, e_og_g = one_minus(*square(gg, e_g))
    dp = [dct * gg * gi * og_i, dct * c_prev * gf * og_f, dct * gi * og_g, dh * tc * go * og_o]
    e_dp = [_pb([dct, gg, gi, og_i], [e_dct, e_g, e_i, e_og_i], 3), _pb([dct, c_prev, gf, og_f], [e_dct, e_cp, e_f, e_og_f], 3),
            _pb([dct, gi, og_g], [e_dct, e_i, e_og_g], 2), _pb([dh, tc, go, og_o], [e_dh, e_tc, e_o, e_og_o], 3)]
    dc_out, e_dc_out = dct * gf, _pb([dct, gf], [e_dct, e_f], 1)
    z = np.zeros_like(dh)
    return (np.where(live, np.concatenate(dp, 1), 0.0), np.where(live, np.concatenate(e_dp, 1), 0.0), np.where(live, dc_out, dc),
            np.where(live, e_dc_out, e_dc), np.where(live, z, dh), np.where(live, z, e_dh))


def cell_bwd_ref64(dh_gemm, dh_carry_in, dc_in, gates, c_prev, c, lengths, step):
    """dict(d_pre [B][4D], dc_out, dh_carry_out) float64 with b_*; dh_gemm None = the last step.  Finished rows: d_pre 0, dc_out =
    dc_in, dh_carry_out = fl(dh_gemm + dh_carry_in), the one rounding that sum has (bound u |dh|)."""
    b, d = c.shape
    live = (step < lengths)[:, None]
    dh = dh_carry_in.astype(np.float64) + (0.0 if dh_gemm is None else dh_gemm.astype(np.float64))
    e_dh = np.zeros((b, d)) if dh_gemm is None else U * np.abs(dh)
    dp, e_dp, dco, e_dco, car, e_car = _bwd_step(dh, e_dh, dc_in.astype(np.float64), np.zeros((b, d)), gates.astype(np.float64),
                                                 c_prev.astype(np.float64), c.astype(np.float64), live, d)
    return dict(d_pre=dp, b_d_pre=e_dp, dc_out=dco, b_dc_out=e_dco, dh_carry_out=car, b_dh_carry_out=e_car, live=live[:, 0])


def cell_bwd_emul(dh_gemm, dh_carry_in, dc_in, gates, c_prev, c, lengths, step, wrong=None):
    """k_lstm_cell_bwd in fp32, products from the left as written.  wrong: carry_dropped | dc_not_carried | tanh_of_c_prev |
    forget_grad_uses_c."""
    b, d = c.shape
    live = (step < lengths)[:, None]
    dh = _add(np.zeros((b, d), F32) if dh_gemm is None else dh_gemm, dh_carry_in)
    gi, gf, gg, go = (np.asarray(gates[:, q * d: (q + 1) * d], F32) for q in range(4))
    one = F32(1.0)
    tc = LR._gate_tanh(np.asarray(c_prev if wrong == "tanh_of_c_prev" else c, F32), False)
    dct = _add(dc_in, _mul(_mul(dh, go), _add(one, -_mul(tc, tc))))
    dp = [_mul(_mul(_mul(dct, gg), gi), _add(one, -gi)), _mul(_mul(_mul(dct, c if wrong == "forget_grad_uses_c" else c_prev), gf), _add(one, -gf)),
          _mul(_mul(dct, gi), _add(one, -_mul(gg, gg))), _mul(_mul(_mul(dh, tc), go), _add(one, -go))]
    z = np.zeros((b, d), F32)
    return dict(d_pre=np.where(live, np.concatenate(dp, 1), F32(0)),
                dc_out=np.where(live, _mul(dct, gf), z if wrong == "dc_not_carried" else np.asarray(dc_in, F32)),
                dh_carry_out=np.where(live, z, z if wrong == "carry_dropped" else dh))


@functools.lru_cache(maxsize=None)
def cell_inputs(b, d, seed=0):
    """One step's arguments for both kernels, N(0, 1)-sized fp32 (any width is legal here).  lengths: rows 0 and 1 (where they
    exist) at CELL_T and 1, the rest random in [1, CELL_T]; token 0 sits inside every sentence of three words or more."""
    rng = np.random.default_rng([seed, b, d, 7])
    t, v = CELL_T, CELL_VOCAB
    ln = rng.integers(1, t + 1, b).astype(np.int32)
    ln[0] = t
    if b > 1:
        ln[1] = 1
    tok = rng.integers(1, v, (b, t)).astype(np.int32)
    tok[ln >= 3, 1] = 0
    n = lambda *s: rng.standard_normal(s).astype(F32)      # noqa: E731
    p = dict(b=b, d=d, tokens=tok, lengths=ln, pre=n(b, 4 * d), table=n(v, 4 * d), c_prev=n(b, d), h_prev=n(b, d),
             dh_gemm=n(b, d), dh_carry_in=n(b, d), dc_in=n(b, d), c=n(b, d))
    g = rng.uniform(0.02, 0.98, (b, 4 * d))
    g[:, 2 * d: 3 * d] = rng.uniform(-0.98, 0.98, (b, d))
    p["gates"] = g.astype(F32)
    return _frozen(p)


def cell_steps():
    """(step, reverse) of the forward cases: the first step, one in the middle (rows past their end, token 0 inside a sentence),
    step = max_len - 1, each in both directions."""
    return [(s, r) for s in (0, 1, CELL_T - 1) for r in (0, 1)]


def cell_fwd_check(got, ref, factor):
    """got: dict(gates, c, h), each [B + guard rows][..] prefilled with SENTINEL: rows [0, B) within factor x bound of ref (bit-equal
    where the bound is 0: the carried state and the zero gates of finished rows), the guard rows untouched.  (ok, why)."""
    for k in ("gates", "c", "h"):
        n = ref[k].shape[0]
        if not np.all(np.asarray(got[k])[n:] == SENTINEL):
            return False, k + ": written past the last row"
        if not _written(np.asarray(got[k])[:n]):
            return False, k + ": an element was not written"
        if not within(np.asarray(got[k])[:n], ref[k], ref["b_" + k], factor):
            return False, "%s beyond %g x bound (worst ratio %.3g)" % (k, factor, worst_ratio(np.asarray(got[k])[:n], ref[k], ref["b_" + k]))
    return True, ""


def cell_bwd_check(got, ref, factor):
    for k in ("d_pre", "dc_out", "dh_carry_out"):
        n = ref[k].shape[0]
        if not np.all(np.asarray(got[k])[n:] == SENTINEL):
            return False, k + ": written past the last row"
        if not _written(np.asarray(got[k])[:n]):
            return False, k + ": an element was not written"
        if not within(np.asarray(got[k])[:n], ref[k], ref["b_" + k], factor):
            return False, "%s beyond %g x bound (worst ratio %.3g)" % (k, factor, worst_ratio(np.asarray(got[k])[:n], ref[k], ref["b_" + k]))
    return True, ""


GATE_SWEEP_D = 64


@functools.lru_cache(maxsize=None)
def gate_sweep():
    """Arguments of the isolated gate-function measurement, as a table [V][4 * GATE_SWEEP_D] with one one-word sentence per row:
    [-30, 30] in steps of 2^-8, +-2^-k and +-1.5 2^-k for k = 0 .. 40, +-0; padded with zeros to whole rows."""
    k = np.arange(0, 41)
    x = np.concatenate([np.arange(-30 * 256, 30 * 256 + 1) / 256.0, 2.0 ** -k, -(2.0 ** -k), 1.5 * 2.0 ** -k, -1.5 * 2.0 ** -k, [0.0, -0.0]])
    w = 4 * GATE_SWEEP_D
    x = np.concatenate([x, np.zeros((-len(x)) % w)]).astype(F32).reshape(-1, w)
    x.setflags(write=False)
    return x


def gate_functions64(x):
    """What the gates output of the sweep must hold, float64: sigmoid in slices i, f, o and tanh in slice g."""
    d = x.shape[1] // 4
    x64 = x.astype(np.float64)
    out = sigmoid64(x64)
    out[:, 2 * d: 3 * d] = np.tanh(x64[:, 2 * d: 3 * d])
    return out


# ---- C: the in-library loops --------------------------------------------------------------------------------------------------------------

LOOP_VOCAB = 11
# (B, D, T, W_hh family, length layout, non-zero initial state): every B of {1, 33, 64, 65, 130} (the few-rows kernel owns 64-row
# tiles), every D of {4, 12, 64, 100} (K / 8 splits unevenly at 4, 12, 100) and 300, every T of {1, 2, 7} (no product in the
# backward at T = 1), every layout.  The reference family (1.5 u / sqrt(D), rows of |W_hh| summing to 0.75 sqrt(D)) multiplies
# the carried bound by about that per step: it runs at T <= 2, or at T = 7 where D = 4; at D = 300 its backward product (K = 1,200)
# alone passes the cap of d_pre, so that width runs the contractive family.
LOOP_CASES = [(1, 4, 1, "contractive", "equal", False), (33, 12, 2, "reference", "one_long", False),
              (64, 64, 7, "contractive", "random", False), (65, 100, 7, "contractive", "random", False),
              (130, 4, 7, "reference", "random", False), (130, 64, 2, "reference", "one_long", False),
              (33, 100, 1, "reference", "equal", False), (65, 12, 7, "contractive", "equal", False),
              (5, 300, 2, "contractive", "random", False), (33, 64, 2, "reference", "random", True)]


@functools.lru_cache(maxsize=None)
def loop_inputs(b, d, t, family, layout, init, seed=0):
    """dict(table [2][V][4D] fp32 - lstm_ref's exact gate table -, w_hh_k [2][D][4D] = W_hh^T, tokens [B][T], lengths, c0, h0 [B][D]
    (zeros unless init), dh_last [B][D]).  Tokens fill the whole buffer: what lies behind a length must not be read."""
    base = LR.case_inputs(d, b, t, LOOP_VOCAB, family, 1.0, "equal", 0, seed)
    kv = LR.kernel_view(base, d)
    rng = np.random.default_rng([seed, b, d, t, 11])
    if layout == "equal":
        ln = np.full(b, t, np.int32)
    elif layout == "one_long":
        ln = np.ones(b, np.int32)
        ln[b // 2] = t
    else:
        ln = rng.integers(1, t + 1, b).astype(np.int32)
        ln[0] = t
        if b > 1:
            ln[b - 1] = 1
    c0 = (rng.uniform(-1, 1, (b, d)) if init else np.zeros((b, d))).astype(F32)
    h0 = (rng.uniform(-0.5, 0.5, (b, d)) if init else np.zeros((b, d))).astype(F32)
    table = kv["table"][:, :LOOP_VOCAB].astype(F32)
    assert np.array_equal(table.astype(np.float64), kv["table"][:, :LOOP_VOCAB])
    return _frozen(dict(b=b, d=d, t=t, base=base, table=table, w_hh_k=kv["w_hh"].astype(F32), tokens=base["tokens"], lengths=ln, c0=c0, h0=h0,
                        dh_last=rng.standard_normal((b, d)).astype(F32)))


def _prod_bound(a, da, w_abs, ref):
    """|skinny(a~ w) - a w| with |a~ - a| <= da: gemm_ref.gemm_bound's any-order term on |a| + da, plus the carried part."""
    k = a.shape[1]
    return da @ w_abs + gamma(k + 2) * ((np.abs(a) + da) @ w_abs) + U * np.abs(ref)


def train_fwd_ref64(table, w_hh_k, tokens, lengths, reverse, c0, h0, e_table=None):
    """One direction of t2p_lstm_train_forward: dict(gates [T][B][4D], cs, hs [T+1][B][D]) float64 with b_* carried beside them.
    table: fp32 taken as exact, or (D) float64 known to e_table."""
    b, t = tokens.shape
    d = w_hh_k.shape[0]
    w, tab = w_hh_k.astype(np.float64), table.astype(np.float64)
    wa = np.abs(w)
    gates, b_gates = np.zeros((t, b, 4 * d)), np.zeros((t, b, 4 * d))
    cs, hs, b_cs, b_hs = (np.zeros((t + 1, b, d)) for _ in range(4))
    cs[0], hs[0] = c0, h0
    for s in range(t):
        live = (s < lengths)[:, None]
        tok = tokens[np.arange(b), _token_col(lengths, s, reverse, t)]
        pre = hs[s] @ w
        d_pre = _prod_bound(hs[s], b_hs[s], wa, pre)
        z = pre + tab[tok]
        d_in = d_pre if e_table is None else d_pre + e_table[tok]
        g, dg, c, dc, h, dh = _fwd_step(z, d_in + U * (np.abs(z) + d_in), cs[s], b_cs[s], d)
        gates[s], b_gates[s] = np.where(live, g, 0.0), np.where(live, dg, 0.0)
        cs[s + 1], b_cs[s + 1] = np.where(live, c, cs[s]), np.where(live, dc, b_cs[s])
        hs[s + 1], b_hs[s + 1] = np.where(live, h, hs[s]), np.where(live, dh, b_hs[s])
    return dict(gates=gates, cs=cs, hs=hs, b_gates=b_gates, b_cs=b_cs, b_hs=b_hs)


def train_fwd_emul(table, w_hh_k, tokens, lengths, reverse, c0, h0, wrong=None):
    """The loop of t2p_lstm_train_forward in fp32: pre = skinny_emul(hs[s] W), then cell_fwd_emul.  wrong: the forward switches of
    cell_fwd_emul | initial_state_overwritten (slice 0 of cs / hs zeroed)."""
    b, t = tokens.shape
    d = w_hh_k.shape[0]
    gates = np.zeros((t, b, 4 * d), F32)
    cs, hs = np.zeros((t + 1, b, d), F32), np.zeros((t + 1, b, d), F32)
    if wrong != "initial_state_overwritten":
        cs[0], hs[0] = c0, h0
    for s in range(t):
        pre = skinny_emul(hs[s], d, np.asarray(w_hh_k, F32), np.zeros((b, 4 * d), F32), 4 * d, b, d, 4 * d)
        o = cell_fwd_emul(pre, table, tokens, lengths, s, reverse, cs[s], hs[s], wrong)
        gates[s], cs[s + 1], hs[s + 1] = o["gates"], o["c"], o["h"]
    return dict(gates=gates, cs=cs, hs=hs)


def train_bwd_ref64(dh_last, w_hh_t, gates, cs, lengths):
    """t2p_lstm_train_backward on exact fp32 inputs: dict(d_pre [T][B][4D], b_d_pre)."""
    t, b, d4 = gates.shape
    d = d4 // 4
    w = w_hh_t.astype(np.float64)
    wa = np.abs(w)
    d_pre, b_d_pre = np.zeros((t, b, d4)), np.zeros((t, b, d4))
    carry, e_carry = dh_last.astype(np.float64), np.zeros((b, d))
    dc, e_dc = np.zeros((b, d)), np.zeros((b, d))
    for s in range(t - 1, -1, -1):
        live = (s < lengths)[:, None]
        if s == t - 1:
            dh, e_dh = carry, e_carry
        else:
            dg = d_pre[s + 1] @ w
            e_dg = _prod_bound(d_pre[s + 1], b_d_pre[s + 1], wa, dg)
            dh = dg + carry
            e_dh = e_dg + e_carry + U * (np.abs(dh) + e_dg + e_carry)
        d_pre[s], b_d_pre[s], dc, e_dc, carry, e_carry = _bwd_step(dh, e_dh, dc, e_dc, gates[s].astype(np.float64), cs[s].astype(np.float64),
                                                                  cs[s + 1].astype(np.float64), live, d)
    return dict(d_pre=d_pre, b_d_pre=b_d_pre)


def train_bwd_emul(dh_last, w_hh_t, gates, cs, lengths, wrong=None, ws_fill=np.nan):
    """The loop of t2p_lstm_train_backward in fp32.  wrong: the backward switches of cell_bwd_emul | dh_gemm_read_at_last_step (the
    scratch slot, holding ws_fill, is added at step T - 1)."""
    t, b, d4 = gates.shape
    d = d4 // 4
    d_pre = np.zeros((t, b, d4), F32)
    carry, dc = np.asarray(dh_last, F32), np.zeros((b, d), F32)
    dh_gemm = np.full((b, d), ws_fill, F32)
    for s in range(t - 1, -1, -1):
        first = s == t - 1 and wrong != "dh_gemm_read_at_last_step"
        o = cell_bwd_emul(None if first else dh_gemm, carry, dc, gates[s], cs[s], cs[s + 1], lengths, s, wrong)
        d_pre[s], dc, carry = o["d_pre"], o["dc_out"], o["dh_carry_out"]
        if s > 0:
            dh_gemm = skinny_emul(d_pre[s], d4, np.asarray(w_hh_t, F32), np.zeros((b, d), F32), d, b, d4, d)
    return dict(d_pre=d_pre)


@functools.lru_cache(maxsize=None)
def loop_reference(case, reverse):
    """(inputs, forward ref, backward inputs (gates, cs fp32 of the float64 forward), backward ref) of LOOP_CASES[case]."""
    inp = loop_inputs(*LOOP_CASES[case])
    i = 1 if reverse else 0
    fwd = train_fwd_ref64(inp["table"][i], inp["w_hh_k"][i], inp["tokens"], inp["lengths"], reverse, inp["c0"], inp["h0"])
    g32, c32 = fwd["gates"].astype(F32), fwd["cs"].astype(F32)
    w_t = np.ascontiguousarray(inp["w_hh_k"][i].T)
    bwd = train_bwd_ref64(inp["dh_last"], w_t, g32, c32, inp["lengths"])
    for dct in (fwd, bwd):
        _frozen(dct)
    g32.setflags(write=False)
    c32.setflags(write=False)
    return inp, fwd, dict(gates=g32, cs=c32, w_hh_t=w_t), bwd


def loop_fwd_check(got, ref, factor):
    for k in ("gates", "cs", "hs"):
        if not _written(got[k]):
            return False, k + ": an element was not written"
        if not within(got[k], ref[k], ref["b_" + k], factor):
            return False, "%s beyond %g x bound (worst ratio %.3g)" % (k, factor, worst_ratio(got[k], ref[k], ref["b_" + k]))
    return True, ""


def loop_bwd_check(got, ref, factor):
    if not _written(got["d_pre"]):
        return False, "d_pre: an element was not written"
    if not within(got["d_pre"], ref["d_pre"], ref["b_d_pre"], factor):
        return False, "d_pre beyond %g x bound (worst ratio %.3g)" % (factor, worst_ratio(got["d_pre"], ref["d_pre"], ref["b_d_pre"]))
    return True, ""


# ---- D: modules._LstmTrainFn at a width the loops refuse ---------------------------------------------------------------------------------

FALLBACK_DIMS = [6, 10]
FALLBACK_B, FALLBACK_T, FALLBACK_V = 5, 4, 9
GRAD_NAMES = ["emb", "w_ih", "w_hh", "b_ih", "b_hh", "w_ih_r", "w_hh_r", "b_ih_r", "b_hh_r"]


@functools.lru_cache(maxsize=None)
def fallback_inputs(d, seed=0):
    """nn.LSTM's own layout: emb [V][d] (row 0 zero), w_ih, w_hh [2][4d][d], b_ih, b_hh [2][4d] (direction 1 = reverse), tokens
    [B][T] (0 = an unknown word inside a sentence), lengths (row 0 at T, row 1 at 1), coef [B][d]: the loss is sum(out coef).
    N(0, 1) entries times 1.5 / sqrt(d) as the autograd test of the loops fills them, W_hh times 0.5 / sqrt(d): the composed bound
    grows with the row sums of |W_hh| at every step in both passes, and with the larger W_hh it passes 1e-4 per element (the host
    test asserts <= 1e-4 for every gradient and <= 1e-5 for the output)."""
    rng = np.random.default_rng([seed, d, 13])
    b, t, v = FALLBACK_B, FALLBACK_T, FALLBACK_V
    n = lambda *s: rng.standard_normal(s)       # noqa: E731
    emb = n(v, d) * 1.5 / np.sqrt(d)
    emb[0] = 0.0
    ln = rng.integers(1, t + 1, b).astype(np.int32)
    ln[0], ln[1] = t, 1
    tok = rng.integers(0, v, (b, t)).astype(np.int32)
    tok[0, 1] = 0
    return _frozen(dict(d=d, emb=emb.astype(F32), w_ih=(n(2, 4 * d, d) * 1.5 / np.sqrt(d)).astype(F32),
                        w_hh=(n(2, 4 * d, d) * 0.5 / np.sqrt(d)).astype(F32), b_ih=(n(2, 4 * d) * 0.5).astype(F32),
                        b_hh=(n(2, 4 * d) * 0.5).astype(F32), tokens=tok, lengths=ln, coef=n(b, d).astype(F32)))


def _tn(a, ea, b_, eb):
    """a^T b of t2p_gemm_tn with a, b known to ea, eb: gemm_ref.tn_bound on the magnitudes plus the carried parts."""
    ref = a.T @ b_
    aa, bb = np.abs(a) + ea, np.abs(b_) + eb
    return ref, gamma(a.shape[0] + 2) * (aa.T @ bb) + U * np.abs(ref) + np.abs(a).T @ (eb + 0.0 * bb) + (ea + 0.0 * aa).T @ bb


def fallback_ref64(p):
    """The step-by-step path of _LstmTrainFn (products on ops.matmul = the tiled t2p_gemm with K zero-padded: padding adds no
    rounding) in float64 with the bounds of B and C composed: dict(out [B][d], b_out, grads = the nine gradients in GRAD_NAMES'
    order, b_grads)."""
    d, tok, ln = p["d"], p["tokens"], p["lengths"]
    b, t = tok.shape
    v = p["emb"].shape[0]
    emb = p["emb"].astype(np.float64)
    out, b_out = np.zeros((b, d)), np.zeros((b, d))
    d_emb, e_emb, grads, b_grads = [], [], [], []
    fw = []
    for i in range(2):
        wih_k, whh_k = p["w_ih"][i].astype(np.float64).T, p["w_hh"][i].astype(np.float64).T        # [d][4d]
        bias32 = (p["b_ih"][i] + p["b_hh"][i]).astype(F32).astype(np.float64)
        e_bias = U * np.abs(p["b_ih"][i].astype(np.float64) + p["b_hh"][i].astype(np.float64))
        prod = emb @ wih_k
        table = prod + p["b_ih"][i].astype(np.float64) + p["b_hh"][i].astype(np.float64)
        e_table = _prod_bound(emb, 0.0 * emb, np.abs(wih_k), prod) + e_bias + U * (np.abs(prod + bias32) + e_bias)
        f = train_fwd_ref64(table, whh_k, tok, ln, i == 1, np.zeros((b, d)), np.zeros((b, d)), e_table=e_table)
        fw.append((f, wih_k, whh_k))
        out += f["hs"][t]
        b_out += f["b_hs"][t]
    sum_h = out
    out = 0.5 * sum_h
    b_out = 0.5 * (b_out + U * (np.abs(sum_h) + b_out)) + U * np.abs(out)
    steps = np.arange(t)[:, None]
    active = (steps < ln[None, :]).reshape(t * b)
    for i, (f, wih_k, whh_k) in enumerate(fw):
        w_t, wa_t = whh_k.T, np.abs(whh_k.T)                                                       # [4d][d]
        d_pre, e_pre = np.zeros((t, b, 4 * d)), np.zeros((t, b, 4 * d))
        carry, e_carry = 0.5 * p["coef"].astype(np.float64), np.zeros((b, d))
        dc, e_dc = np.zeros((b, d)), np.zeros((b, d))
        for s in range(t - 1, -1, -1):
            live = (s < ln)[:, None]
            if s == t - 1:
                dh, e_dh = carry, e_carry
            else:
                dg = d_pre[s + 1] @ w_t
                e_dg = _prod_bound(d_pre[s + 1], e_pre[s + 1], wa_t, dg)
                dh = dg + carry
                e_dh = e_dg + e_carry + U * (np.abs(dh) + e_dg + e_carry)
            d_pre[s], e_pre[s], dc, e_dc, carry, e_carry = _bwd_step(dh, e_dh, dc, e_dc, f["gates"][s], f["cs"][s], f["cs"][s + 1], live, d,
                                                                     f["b_gates"][s], f["b_cs"][s], f["b_cs"][s + 1])
        flat, e_flat = d_pre.reshape(t * b, 4 * d), e_pre.reshape(t * b, 4 * d)
        d_whh_k, e_whh_k = _tn(f["hs"][:t].reshape(t * b, d), f["b_hs"][:t].reshape(t * b, d), flat, e_flat)
        pos = steps if i == 0 else np.clip(ln[None, :] - 1 - steps, 0, None)
        tk = tok.T[pos, np.arange(b)[None, :]].reshape(t * b)
        onehot = np.zeros((t * b, v))
        onehot[np.arange(t * b), tk] = active
        d_table, e_dtable = _tn(onehot, 0.0 * onehot, flat, e_flat)
        d_bias = d_table.sum(0)
        e_dbias = e_dtable.sum(0) + gamma(v) * (np.abs(d_table) + e_dtable).sum(0) + U * np.abs(d_bias)
        d_wih_k, e_wih_k = _tn(emb, 0.0 * emb, d_table, e_dtable)
        part = d_table @ wih_k.T
        d_emb.append(part)
        e_emb.append(_prod_bound(d_table, e_dtable, np.abs(wih_k.T), part))
        grads += [d_wih_k.T, d_whh_k.T, d_bias, d_bias]
        b_grads += [e_wih_k.T, e_whh_k.T, e_dbias, e_dbias]
    de = d_emb[0] + d_emb[1]
    e_de = e_emb[0] + e_emb[1] + U * (np.abs(de) + e_emb[0] + e_emb[1])
    de[0], e_de[0] = 0.0, 0.0
    return dict(out=out, b_out=b_out, grads=[de] + grads, b_grads=[e_de] + b_grads)
