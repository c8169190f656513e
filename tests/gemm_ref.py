"""Shared by tests/test_gpu_gemm_family.py and tests/test_gemm_ref_host.py: for every dense product of the path
(csrc/tg_gemm.hip: k_gemm<64|128> and k_gemm_skinny, tg_gemm_x3.hip, tg_gemm_tn.hip, train_gemm.hip)
  (a) `*_inputs`  seeded inputs (computed once per case, handed out read-only) and `*_exact_inputs`, whose result carries no rounding,
  (b) `*_ref64`   a float64 statement of the operation, taking the fp32 inputs as given,
  (c) `*_bound`   a per-element error bound for the arithmetic the kernel is documented to do,
  (d) `*_emul`    a NumPy emulation of that arithmetic on the pitched buffers the C ABI sees, with a `wrong=` switch that
                  builds one deliberately wrong kernel,
plus the launchers' dispatch rules restated (tile side, row splits, the weight-gradient plan).  Plain NumPy: no GPU, no torch.
The GPU tests assert |kernel - (b)| <= 2 (c) element by element (the factor of tests/train_ops_ref.py), bit equality on the exact
inputs, and that nothing outside the output window changes; the host tests prove that (d) stays within 1 (c), that the exact
inputs are exact, and that `check_window` rejects every wrong kernel.

Bounds - derived, not tuned.  u = 2^-24, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, Lemma 3.1).
 * fp32 kernels.  A sum of L products formed by fp32 fma or by rounded products and additions in ANY order (tiles, splits,
   butterflies) differs from the exact sum by at most gamma_L sum|a||w|; the bias addition and one more rounding (the second
   reduction of the split kernels, the conversion of the reference) make it
       gamma_(L+2) (sum|a||w| + |bias|) + u |result|.
   ReLU is 1-Lipschitz: it never enlarges the error.  A residual is added with one more rounding: + u |result + resid|.
 * f16x3 (tg_gemm_x3.hip).  With w' = s w (s a power of two: exact), the kernel splits a = ah + al + ea and w' = wh + wl + ew
   (hi = fp16 to nearest, lo = fp16(x - hi), the difference exact in fp32) and accumulates ah wh + ah wl + al wh in fp32.
   fp16 has 11 significant bits and a subnormal spacing of 2^-24; eta = 2^-25 is half of that.  For |x| <= 65504:
       |x - hi| <= 2^-11 |x| + eta,  |lo| <= (1 + 2^-11)(2^-11 |x| + eta) + eta,  |e| = |x - hi - lo| <= 2^-22 |x| + (1 + 2^-11) eta.
   a w' - (ah wh + ah wl + al wh) = al wl + ea w' + (a - ea) ew, so per product
       |.| <= 3 2^-22 (1 + 2^-10) |a||w'| + (1 + 2^-9) eta (|a| + |w'|) + 6 eta^2                                    (split)
   (2^-22 |a||w'| each for the two split errors and for the dropped lo.lo product; the eta terms cover pieces below fp16's
   subnormal spacing).  Products of two fp16 values are exact in fp32; 3 K of them are summed in some order:
       gamma_(3K) S3,  S3 = sum(|ah wh| + |ah wl| + |al wh|) <= (1 + 2^-8) sum|a||w'| + 4 eta sum(|a| + |w'|) + 6 eta^2 K.
   The epilogue is one fma (acc / s + bias), then the residual as above:
       bound = (split + gamma_(3K+2) S3) / s + gamma_(3K+2) |bias| + u |result| (+ u |result + resid|).

Exact inputs.  A in {-8..8}, W, bias and the residual in {-64..64} / 64: every product and every partial sum is an integer
multiple of 2^-6 below 2^24 2^-6 in magnitude as long as sum|a||w| + |bias| + |resid| < 2^18 (L < 32,768), so every fp32
operation is exact in any order, and the f16x3 lo planes are zero (|64 s w| <= 64 has 7 bits).  Two-plane inputs for f16x3 (K = 32):
a = p + q 2^-13, w = r + t 2^-13 with q, t in {-8..8} and p, r integers with 4 <= |p|, |r| <= 8: there fp16's spacing is at least
2^-8, so |q| 2^-13 <= 2^-10 is below half of it and hi = p, lo = q 2^-13 exactly.  (With |p| < 4 the sum p + q 2^-13 can be an
fp16 number itself - p = 1, q = 8 - and the split would be hi = a, lo = 0.)  The kernel must return
sum(p r + (p t + q r) 2^-13) bit for bit: all multiples of 2^-13 whose magnitudes sum to less than 2^11, hence exact."""
import functools

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -25
F32 = np.float32
FACTOR_GPU = 2.0
NUM_CUS = 256                      # MI355X; the GPU tests pass the device's own multi_processor_count

# M x K x N of t2p_gemm / t2p_gemm_residual / t2p_gemm_x3
GEMM_SHAPES = [(1, 4, 8), (65, 20, 40), (129, 64, 256), (300, 1024, 512)]
TILE_SHAPE = (2100, 64, 1024)      # 17 x 8 tiles of 128: the 128 tile below 272 CUs; its first TILE_SMALL_ROWS rows take the 64 tile
TILE_SMALL_ROWS = 300
X3_SCALES = [1.0, 1024.0]
# t2p_gemm_skinny: K in {4, 12, 20, 128, 260} x N in {1, 32, 40, 1024} x M in {1, 33, 64, 130}, every value at least once, with
# the LSTM's own (64, 256, 1024) and (64, 1024, 256)
SKINNY_SHAPES = [(1, 4, 1), (33, 4, 40), (64, 4, 32), (130, 12, 32), (64, 12, 1), (130, 20, 40), (33, 20, 32), (33, 128, 40),
                 (1, 260, 1024), (130, 260, 40), (64, 256, 1024), (64, 1024, 256)]
TN_SHAPES = [(1, 4, 8), (37, 67, 128), (3001, 100, 72), (5000, 256, 1024), (0, 8, 8)]         # M x K1 x N
# (K1, N) -> what wgrad_plan must select: (tpw, ktp, ntp, n_phase)
WGRAD_WIDTHS = {(160, 96): (3, 8, 1, 1), (160, 128): (4, 8, 1, 1), (160, 160): (5, 8, 1, 1), (160, 192): (6, 8, 1, 1),
                (160, 200): (7, 8, 1, 1), (100, 160): (3, 4, 1, 1), (20, 40): (1, 1, 2, 4), (32, 72): (1, 1, 4, 2),
                (48, 72): (1, 2, 4, 1), (67, 128): (2, 4, 1, 1), (300, 256): (8, 8, 1, 1), (256, 300): (8, 8, 1, 1),
                (32, 6): (1, 1, 1, 8)}
WGRAD_ROWS = [1, 33, 3001]
WGRAD_WAVE_SHAPE = (20000, 32, 8)  # total <= 16384 outputs and >= 128 slots: k_wgrad_reduce_wave


def gamma(n):
    return n * U / (1.0 - n * U)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ---- pitched buffers ----------------------------------------------------------------------------------------------------------------

def poison(rows, pitch):
    """[rows][pitch] fp32 of NaN and 1e30 in alternation: whatever reads it shows in a sum."""
    p = np.empty((rows, pitch), F32)
    p.reshape(-1)[0::2] = np.nan
    p.reshape(-1)[1::2] = 1e30
    return p


def pitched(x, pitch, extra_rows=0, first=0):
    """x [M][W] in columns [first, first + W) of a poisoned [M + extra_rows][pitch] buffer."""
    m, w = x.shape
    buf = poison(m + extra_rows, pitch)
    buf[:m, first: first + w] = x
    return buf


def nan_buffer(rows, pitch):
    return np.full((rows, pitch), np.nan, F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def within(got, ref, bound, factor):
    """Every element of got within factor * bound of ref; where ref is NaN, got must be NaN, where ref is infinite, equal."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    fin = np.isfinite(ref)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return False
    inf = ~fin & ~np.isnan(ref)
    if not np.array_equal(got[inf], ref[inf]):
        return False
    return bool(np.all(np.abs(got[fin] - ref[fin]) <= factor * bound[fin]))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the finite elements of ref (0 / 0 counts as 0, x / 0 as inf)."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound[fin])
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def check_window(after, before, m, n, c0, ref, bound, factor, exact=False):
    """The contract of an output buffer: rows [0, m) x columns [c0, c0 + n) of `after` within factor * bound of ref (bit-equal
    to fp32(ref) with exact=True), every other element - columns outside the window, rows at and beyond m - bit-equal to `before`.
    Returns (ok, reason)."""
    after, before = np.asarray(after, F32), np.asarray(before, F32)
    if after.shape != before.shape:
        return False, "shape"
    keep = np.ones(after.shape, bool)
    keep[:m, c0: c0 + n] = False
    if not np.array_equal(bits(after)[keep], bits(before)[keep]):
        return False, "an element outside the window changed"
    got = after[:m, c0: c0 + n]
    if exact:
        return (True, "") if bits_equal(got, np.asarray(ref, np.float64).astype(F32)) else (False, "not bit-equal to the exact result")
    if not within(got, ref, bound, factor):
        return False, "beyond %g x bound (worst ratio %.3g)" % (factor, worst_ratio(got, ref, bound))
    return True, ""


# ---- dispatch rules of the launchers, restated -------------------------------------------------------------------------------------

def gemm_tile(m, n, num_cus=NUM_CUS):
    """launch_gemm / launch_gemm_x3: the 64 tile while twice the number of 128 x 128 tiles fits the CUs."""
    tiles128 = ((m + 127) // 128) * ((n + 127) // 128)
    return 64 if tiles128 * 2 <= num_cus else 128


def tn_splits(m, k1, n, num_cus=NUM_CUS):
    tiles = ((k1 + 63) // 64) * ((n + 63) // 64)
    want = (4 * num_cus + tiles - 1) // tiles
    want = min(want, (m + 63) // 64, 4096)
    return max(want, 1)


def wgrad_plan(m, k1, n, num_cus=NUM_CUS):
    """wgrad_plan of csrc/train_gemm.hip."""
    p = dict(blocks_k=(k1 + 255) // 256, blocks_n=(n + 255) // 256)
    kw, nw = min(k1, 256), min(n, 256)
    kt_n, nt_n = (kw + 31) // 32, (nw + 31) // 32
    p["ktp"] = 1 if kt_n <= 1 else 2 if kt_n <= 2 else 4 if kt_n <= 4 else 8
    g = 8 // p["ktp"]
    p["n_phase"], p["ntp"] = 1, 1
    if nt_n >= g:
        p["tpw"] = (nt_n + g - 1) // g
    else:
        p["tpw"] = 1
        p["ntp"] = 1 if nt_n <= 1 else 2 if nt_n <= 2 else 4
        p["n_phase"] = g // p["ntp"]
    ldl = ((kw + 3) & ~3) + ((nw + 3) & ~3)
    p["rows_chunk"] = min(max((16384 // ldl) // 32 * 32, 32), 512)
    blocks = p["blocks_k"] * p["blocks_n"]
    want = (num_cus + blocks - 1) // blocks
    want = max(min(want, (m + 2 * p["rows_chunk"] - 1) // (2 * p["rows_chunk"])), 1)
    p["rows_per_split"] = max(((m + want - 1) // want + 31) // 32 * 32, 32)
    p["splits"] = max((m + p["rows_per_split"] - 1) // p["rows_per_split"], 1)
    p["slots"] = p["splits"] * p["n_phase"] if m > 0 else 0
    p["wave_reduce"] = k1 * n + k1 <= 16384 and p["slots"] >= 128
    return p


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gemm_inputs(m, k, n, seed=0):
    """A [m][k], W [k][n], bias [n], resid [m][n] ~ N(0, 1) fp32."""
    rng = np.random.default_rng([seed, m, k, n])
    return _frozen(rng.standard_normal((m, k)).astype(F32), rng.standard_normal((k, n)).astype(F32),
                   rng.standard_normal(n).astype(F32), rng.standard_normal((m, n)).astype(F32))


@functools.lru_cache(maxsize=None)
def gemm_exact_inputs(m, k, n, seed=1):
    """A in {-8..8}, W, bias, resid in {-64..64} / 64 (see the module text)."""
    rng = np.random.default_rng([seed, m, k, n])
    return _frozen(rng.integers(-8, 9, (m, k)).astype(F32), (rng.integers(-64, 65, (k, n)) / 64.0).astype(F32),
                   (rng.integers(-64, 65, n) / 64.0).astype(F32), (rng.integers(-64, 65, (m, n)) / 64.0).astype(F32))


@functools.lru_cache(maxsize=None)
def two_plane_inputs(m, n, seed=2, k=32):
    """(A, W, exact result, sum of the magnitudes of its terms) of the two-plane f16x3 case: a = p + q 2^-13, w = r + t 2^-13."""
    rng = np.random.default_rng([seed, m, k, n])

    def big(shape):
        return rng.integers(4, 9, shape) * rng.choice([-1, 1], shape)
    p, q, r, t = big((m, k)), rng.integers(-8, 9, (m, k)), big((k, n)), rng.integers(-8, 9, (k, n))
    a, w = (p + q * 2.0 ** -13).astype(F32), (r + t * 2.0 ** -13).astype(F32)
    want = (p @ r).astype(np.float64) + (p @ t + q @ r) * 2.0 ** -13
    return _frozen(a, w, want, np.abs(p) @ np.abs(r) + (np.abs(p) @ np.abs(t) + np.abs(q) @ np.abs(r)) * 2.0 ** -13)


@functools.lru_cache(maxsize=None)
def tn_inputs(m, k1, n, seed=3):
    """A [m][k1] (dY), B [m][n] (X) ~ N(0, 1) fp32."""
    rng = np.random.default_rng([seed, m, k1, n])
    return _frozen(rng.standard_normal((m, k1)).astype(F32), rng.standard_normal((m, n)).astype(F32))


@functools.lru_cache(maxsize=None)
def tn_exact_inputs(m, k1, n, seed=4):
    rng = np.random.default_rng([seed, m, k1, n])
    return _frozen(rng.integers(-8, 9, (m, k1)).astype(F32), (rng.integers(-64, 65, (m, n)) / 64.0).astype(F32))


# ---- float64 statements and bounds ---------------------------------------------------------------------------------------------------

def relu64(x):
    return np.where(x <= 0.0, 0.0, x)      # keeps NaN, as torch.relu


def gemm_ref64(a, w, bias=None, relu=False, resid=None):
    """dict(act = act(a w + bias), out = act + resid), float64; NaN and inf propagate as in IEEE arithmetic."""
    with np.errstate(invalid="ignore", over="ignore"):
        pre = a.astype(np.float64) @ w.astype(np.float64)
        bad = ~np.isfinite(a).all(1)
        for r in np.nonzero(bad)[0]:       # BLAS makes no promise about inf / NaN: state those rows term by term
            pre[r] = (a[r].astype(np.float64)[:, None] * w.astype(np.float64)).sum(0)
        if bias is not None:
            pre = pre + bias.astype(np.float64)
        act = relu64(pre) if relu else pre
        return dict(act=act, out=act if resid is None else act + resid.astype(np.float64))


def gemm_bound(a, w, bias, ref, resid=None, reduction=None):
    """fp32 kernels: gamma_(L+2) (sum|a||w| + |bias|) + u |act| (+ u |act + resid|)."""
    L = a.shape[1] if reduction is None else reduction
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64))
        if bias is not None:
            s = s + np.abs(bias.astype(np.float64))
        b = gamma(L + 2) * s + U * np.abs(ref["act"])
        return b if resid is None else b + U * np.abs(ref["out"])


def x3_bound(a, w, scale, bias, ref, resid=None):
    """f16x3: (split + gamma_(3K+2) S3) / s + gamma_(3K+2) |bias| + u |act| (+ u |act + resid|), see the module text."""
    k = a.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        aa, ww = np.abs(a.astype(np.float64)), np.abs(w.astype(np.float64)) * scale
        s = aa @ ww
        lin = aa.sum(1)[:, None] + ww.sum(0)[None, :]
        split = 3 * 2.0 ** -22 * (1 + 2.0 ** -10) * s + (1 + 2.0 ** -9) * ETA * lin + 6 * ETA * ETA * k
        s3 = (1 + 2.0 ** -8) * s + 4 * ETA * lin + 6 * ETA * ETA * k
        g = gamma(3 * k + 2)
        b = (split + g * s3) / scale + U * np.abs(ref["act"])
        if bias is not None:
            b = b + g * np.abs(bias.astype(np.float64))
        return b if resid is None else b + U * np.abs(ref["out"])


def tn_ref64(a, b):
    return a.astype(np.float64).T @ b.astype(np.float64)


def tn_bound(a, b, ref):
    """gamma_(M+2) sum|a||b| + u |result|: M products in any order, the second reduction's roundings included."""
    return gamma(a.shape[0] + 2) * (np.abs(a.astype(np.float64)).T @ np.abs(b.astype(np.float64))) + U * np.abs(ref)


def colsum_ref64(dy):
    return dy.astype(np.float64).sum(0)


def colsum_bound(dy, ref):
    return gamma(dy.shape[0] + 2) * np.abs(dy.astype(np.float64)).sum(0) + U * np.abs(ref)


def exact_headroom(a, w, bias=None, resid=None):
    """max over the outputs of sum|a||w| + |bias| + |resid|: below 2^18 every fp32 sum of the integer inputs is exact in any order."""
    s = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64))
    if bias is not None:
        s = s + np.abs(bias.astype(np.float64))
    if resid is not None:
        s = s + np.abs(resid.astype(np.float64))
    return float(s.max()) if s.size else 0.0


# ---- emulations -----------------------------------------------------------------------------------------------------------------------

def _fma(acc, x, y):
    """fp32 fma, elementwise: the product of two fp32 values is exact in float64."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc.astype(np.float64) + x.astype(np.float64) * y.astype(np.float64)).astype(F32)


def _add32(x, y):
    with np.errstate(invalid="ignore", over="ignore"):
        return (x.astype(F32) + y.astype(F32)).astype(F32)


def _epilogue(v, c_buf, ldc, c0, m, n, relu, r_buf, ldr, r_first, wrong):
    """relu, residual, store into a copy of c_buf; the wrong switches of the epilogue."""
    out = c_buf.copy()
    if relu:
        v = np.where(v <= 0, F32(0), v).astype(F32)
    if r_buf is not None:
        flat = np.ascontiguousarray(r_buf).reshape(-1)          # read before anything is written (the residual may be c_buf)
        pitch = ldc if wrong == "resid_ldc" else ldr
        idx = (np.arange(m)[:, None] * pitch + r_first + np.arange(n)[None, :]) % flat.size
        v = _add32(v, flat[idx])
    rows = m - 1 if (wrong == "last_row_pair" and m % 2) else m
    col = 0 if wrong == "c0_ignored" else c0
    out[:rows, col: col + n] = v[:rows]
    return out


def gemm_emul(a_buf, lda, w, bias, c_buf, ldc, c0, m, k, n, relu, r_buf=None, ldr=0, r_first=0, tile=64, wrong=None):
    """k_gemm<tile>: one fp32 fma chain over k = 0 .. K - 1 per output from 0 (tiles of 16 k, two per MFMA, in order), + bias,
    ReLU, + residual.  a_buf [>= m][lda], c_buf [rows][ldc] (returned as a modified copy), r_buf any buffer read at pitch ldr from
    element r_first.  wrong: last_k_chunk | last_row_pair | bias_no_n0 | c0_ignored | resid_ldc."""
    assert a_buf.shape[1] == lda and c_buf.shape[1] == ldc
    acc = np.zeros((m, n), F32)
    k_end = k // 16 * 16 if (wrong == "last_k_chunk" and k % 16) else k
    for kk in range(k_end):
        acc = _fma(acc, a_buf[:m, kk: kk + 1], w[kk: kk + 1, :])
    if bias is not None:
        bv = bias[np.arange(n) % tile] if wrong == "bias_no_n0" else bias
        acc = _add32(acc, bv[None, :])
    return _epilogue(acc, c_buf, ldc, c0, m, n, relu, r_buf, ldr, r_first, wrong)


def split_f16(x64):
    """(hi, lo) fp16 pieces of the f16x3 split, as float64 arrays: hi = fp16(x) to nearest even, lo = fp16(x - hi)."""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x64.astype(np.float16).astype(np.float64)
        return hi, (x64 - hi).astype(np.float16).astype(np.float64)


def x3_emul(a_buf, lda, w, scale, bias, c_buf, ldc, c0, m, k, n, relu, r_buf=None, ldr=0, r_first=0, wrong=None):
    """k_gemm_x3: per 16 k, three MFMAs (hi.hi, hi.lo, lo.hi) add their 16 exact products to one fp32 accumulator, rounding once
    each; v = fma(acc, 1 / s, bias).  Also returns the guard word: the bit pattern of max |a[:m, :k]|.
    wrong: no_lo_hi | no_hi_lo | lolo | no_scale (and the epilogue's)."""
    ah, al = split_f16(a_buf[:m, :k].astype(np.float64))
    wh, wl = split_f16(w.astype(np.float64) * scale)
    acc = np.zeros((m, n), F32)
    pairs = [(ah, wh), (ah, wl), (al, wh)]
    if wrong == "no_lo_hi":
        pairs = [(ah, wh), (ah, wl)]
    elif wrong == "no_hi_lo":
        pairs = [(ah, wh), (al, wh)]
    elif wrong == "lolo":
        pairs = pairs + [(al, wl)]
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, k, 16):
            for x, y in pairs:
                acc = (acc.astype(np.float64) + x[:, k0: k0 + 16] @ y[k0: k0 + 16, :]).astype(F32)
        inv = 1.0 if wrong == "no_scale" else 1.0 / scale
        v = (acc.astype(np.float64) * inv + (0.0 if bias is None else bias.astype(np.float64)[None, :])).astype(F32)
    amax = np.abs(a_buf[:m, :k]).max().astype(F32).view(np.int32) if m and k else np.int32(0)
    return _epilogue(v, c_buf, ldc, c0, m, n, relu, r_buf, ldr, r_first, wrong), int(amax)


def skinny_emul(a_buf, lda, w, c_buf, ldc, m, k, n, wrong=None):
    """k_gemm_skinny: K is cut into eight ranges of `per` (a multiple of 8); inside a range, per group of 8 k, MFMA j adds
    a[k + j] w[k + j] (lane half 0) and a[k + 4 + j] w[k + 4 + j] (lane half 1, masked past K); range 0's sum then takes the
    other seven in order.  wrong: upper_half (the half past K of a K = 8 i + 4 group is not masked: it reads A's padding)."""
    per = (((k + 7) // 8 + 7) // 8) * 8
    w_pad = np.concatenate([w, np.ones((8, n), F32)], 0)
    total = None
    for ks in range(8):
        acc = np.zeros((m, n), F32)
        for k0 in range(min(ks * per, k), min(ks * per + per, k), 8):
            for j in range(4):
                for kk in (k0 + j, k0 + 4 + j):
                    if kk < k or (wrong == "upper_half" and kk < lda):
                        acc = _fma(acc, a_buf[:m, kk: kk + 1], w_pad[kk: kk + 1, :])
        total = acc if total is None else _add32(total, acc)
    out = c_buf.copy()
    out[:m, :n] = total
    return out


def tn_emul(a_buf, lda, b_buf, ldb, c_buf, ldc, m, k1, n, num_cus=NUM_CUS, wrong=None, cols=None):
    """k_gemm_tn + k_gemm_tn_reduce: the rows are cut into `splits` ranges of `per` (a multiple of 16); each range is one fma chain
    over its rows per output, the ranges' sums are added in order from 0.  cols: emulate only these output columns (each output
    has its own chain; used for the largest shape).  wrong: split_missing (the last range's partial is left out)."""
    splits = tn_splits(m, k1, n, num_cus)
    per = ((m + splits - 1) // splits + 15) // 16 * 16
    cols = np.arange(n) if cols is None else np.asarray(cols)
    a, b = a_buf[:m, :k1], b_buf[:m][:, cols]
    acc = np.zeros((splits, k1, len(cols)), F32)
    for i in range(per):
        rows = np.arange(splits) * per + i
        ok = rows < m
        if not ok.any():
            break
        acc[ok] = _fma(acc[ok], a[rows[ok]][:, :, None], b[rows[ok]][:, None, :])
    total = np.zeros((k1, len(cols)), F32)
    for s in range(splits - 1 if (wrong == "split_missing" and splits > 1) else splits):
        total = _add32(total, acc[s])
    out = c_buf.copy()
    out[:k1, cols] = total
    return out


def _wave_sum(parts):
    """k_wgrad_reduce_wave: lane l adds the slots l, l + 64, ... in order from 0, then the xor butterfly 32, 16, .. 1."""
    lanes = np.zeros((64,) + parts.shape[1:], F32)
    for s in range(parts.shape[0]):
        lanes[s % 64] = _add32(lanes[s % 64], parts[s])
    for off in (32, 16, 8, 4, 2, 1):
        lanes = _add32(lanes, lanes[np.arange(64) ^ off])
    return lanes[0]


def wgrad_emul(dy_buf, lda, x_buf, ldb, c_buf, ldc, m, k1, n, want_colsum=True, num_cus=NUM_CUS, wrong=None):
    """k_wgrad_f32 + its reduce kernel.  Rows are cut into `splits` ranges; inside a range the rows are staged rows_chunk at a time
    and the row PAIRS of a chunk go round-robin to n_phase phases; (split, phase) is one slot: one fma chain per output over its
    rows in order, and two column sums of dY (even and odd rows of the pairs: the two lane halves).  The slots are added in
    order from 0 (k_wgrad_reduce) or per lane and through a butterfly (k_wgrad_reduce_wave).  Returns (dW buffer, colsum).
    wrong: split_missing (the last slot's block left out of dW) | colsum_lda (the column sums run over the whole pitch: column j
    of the lda columns of dY is added into sum j % K1); both may be named in one string."""
    p = wgrad_plan(m, k1, n, num_cus)
    slots, nph, rc, rps = max(p["slots"], 0), p["n_phase"], p["rows_chunk"], p["rows_per_split"]
    row = np.arange(m)
    local = row % rps if m else row
    slot = (row // rps) * nph + ((local % rc) // 2) % nph
    order = [row[slot == s] for s in range(slots)]
    depth = max((len(o) for o in order), default=0)
    idx = np.full((slots, depth), -1, np.int64)
    for s, o in enumerate(order):
        idx[s, : len(o)] = o
    dy, x = dy_buf[:m, :k1], x_buf[:m, :n]
    dyc = dy
    wrong = wrong or ""
    if "colsum_lda" in wrong:
        dyc = np.zeros((m, k1), F32)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(lda):
                dyc[:, j % k1] += dy_buf[:m, j]
    acc = np.zeros((slots, k1, n), F32)
    cs = np.zeros((slots, 2, k1), F32)
    for t in range(depth):
        rows = idx[:, t]
        ok = rows >= 0
        r = rows[ok]
        acc[ok] = _fma(acc[ok], dy[r][:, :, None], x[r][:, None, :])
        h = ((r % rps) % rc) % 2
        cs[np.nonzero(ok)[0], h] = _add32(cs[np.nonzero(ok)[0], h], dyc[r])
    used = slots - 1 if ("split_missing" in wrong and slots > 1) else slots
    parts, cparts = acc[:used], cs.reshape(2 * slots, k1)
    if p["wave_reduce"]:
        total, csum = _wave_sum(parts), _wave_sum(cparts)
    else:
        total, csum = np.zeros((k1, n), F32), np.zeros(k1, F32)
        for s in range(used):
            total = _add32(total, parts[s])
        for s in range(2 * slots):
            csum = _add32(csum, cparts[s])
    out = c_buf.copy()
    out[:k1, :n] = total
    return out, (csum if want_colsum else None)
