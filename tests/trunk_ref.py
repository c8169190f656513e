"""Shared by tests/test_gpu_trunk_stages.py and tests/test_trunk_ref_host.py: the cell encoder's trunk (PointNet++ of the object
encoder: grouping, SA levels 1-3, GA, lin1, lin2) and the object head behind it, ONE STAGE AT A TIME.  Every stage is stated on the
stage's own inputs - on the GPU those are the kernel's traced upstream outputs (t2p_cell_trace), so errors do not compound and no
discrete choice (FPS pick, ball-query hit) stands between the kernel and its reference.  Per stage:
  (a) `*_ref64`   float64 on the fp32 inputs as given,
  (b) `*_bound`   a per-element bound for the arithmetic the kernel is documented to do (include/t2p.h, DESIGN 4, the kernel headers),
  (c) `*_emul`    a NumPy emulation of that arithmetic with an `order=` of summation and a `wrong=` switch that builds one
                  deliberately wrong kernel.
Plain NumPy: no GPU, no torch (oracle_groups loads oracle/primitives.c through ctypes).

The GPU tests assert, per stage, precision and case,
  (A) |kernel - ref64| <= 2 bound for every element (gemm_ref.FACTOR_GPU, gemm_ref.within),
  (B) max|kernel - ref64| <= R max(max|emul - ref64|, u max|ref64|): a worst-case bound is blind to a lost fp16 plane (a kernel
      without its lo.hi products sits at 0.89 of it at SA2, K = 128, and at 0.10 at GA, K = 512), the emulation's own error is not.  R = R_SHARP below: 4 x the largest
      ratio between the maxima of the correct emulation under five summation orders (sequential, pairwise, 16-k tiles, reversed,
      random), rounded up to a power of two; the host test re-derives it and measures by how much every arithmetic wrong= variant
      exceeds it at its stage (8 x and more, except a lost plane at GA and lin1: 4 x, where tier (C) carries it).
  (C) bit equality with fp32(ref64) on the exact inputs at the end of this file: the single-plane set (hi.hi, lo.hi and, through its
      probe channel, a split by truncation) and one two-plane set per MFMA stage (hi.lo).
The host tests prove that the correct emulation stays within 1 x bound under every order, that the row sets below are the edge
lists of oracle/pyg_restated.py, and that every wrong= variant is rejected, naming the tier.

Row sets.  A level's edge rows come from the traced nbr / cnt tables plus PyG's self-loop rule as DESIGN 2 pins it: with
self_loops, a hit whose two CELL-local indices agree (rank n_dense + j == rank n_cent + c, rank = the object's position in its cell)
is removed, and dense row i of the cell's flattened batch feeds centroid row i of the cell for every centroid row - the source of
object o's loop row c is global dense row first(o) n_dense + rank n_cent + c, in general a point of ANOTHER object.  (The kernels'
lists keep the removed hit: it names the same dense row as the loop, so the maximum is the same.)

Documented arithmetic, u = 2^-24, gamma_n as in gemm_ref (whose f16x3 split model and bounds are reused; eta = 2^-25).
 * Layer 1 at levels 2, 3 and, off the 256-point shapes or in fp32, level 1: the algebraic split A_j = W1 [x_j | pos_j] + b1 per dense
   point (k_ws DENSE_STORE), B_i = W1p pos_i per centroid (((x w0) + y w1) + z w2, fp32 fma), h = relu(fp32(A_j - B_i)) per edge.
   f16x3 table: both operands split hi = fp16(x), lo' = fp16(2048 (x - hi)) (pack_f16x3: "hi + lo / 2048"), TWO accumulators
   acc = b1 + sum hi.hi, accx = sum (hi.lo' + lo'.hi), A = fma(accx, 2^-11, acc).  Scaling lo by 2048 only lowers its absolute
   (subnormal) error, so gemm_ref's split model covers it at scale 1: err_A = x3_bound(x, W1, 1, b1).  fp32: err_A = gemm_bound.
   err_B = gamma_4 sum|W1p||pos_i| + u|B|.  The edge row inherits BOTH tables' errors - the bound carries |A| + |B| terms, not
   |A - B|, which cancels:  e1 = err_A[j] + err_B[i] + u (|A - B| + err_A[j] + err_B[i]).
 * Layer 1 of k_sa_points (f16x3, 256 points): x = [rgb_j | fp32(pos_j - pos_i) | 1 | 0] per edge, the bias rides on the constant 1;
   W1 and b1 split UNSCALED (hi = fp16(w), lo = fp16(w - hi)); three v_mfma_f32_32x32x8_f16 (hi.hi, w_lo.x_hi, w_hi.x_lo) into one
   accumulator:  e1 = x3_bound([x | 1], [W1; b1], 1) + (u |pos_j - pos_i|) |W1p|   (the reference subtracts in float64).
 * Layer 2 of every SA level, f16x3: the scaled single-accumulator form w' = s w (s = packing.f16x3_scale, a power of two),
   hi = fp16(w'), lo = fp16(w' - hi); h split the same way; per 16 k hi.hi, hi.lo, lo.hi into ONE fp32 accumulator; max over the
   centroid's rows; r = max(fp32(raw + s b2), 0); out = r / s (exact).  (k_sa_stream starts the accumulator at s b2 instead: the same
   bound.)  Per row: x3_bound(|h| + e1, W2, s, b2) + e1 |W2|; the max over rows is 1-Lipschitz in the sup norm:
       bound[i] = max over the rows r of centroid i of (e1[r] |W2| + x3_bound[r]) + u |out[i]|.
   fp32: gemm_bound in place of x3_bound (fma chains of v_mfma_f32_32x32x2_f32, any order).
 * GA: layer 1 on [F | xyz] as the tables above (with ReLU), the hidden row stored as two fp16 planes (hi, lo' = fp16(2048 (h - hi))) -
   the split GA layer 2 would do itself, so no further term; layer 2 with the unscaled pack_f16x3 image and two accumulators per k
   half, the halves added, + b2, ReLU, max over the object's rows: the SA formula with s = 1.
 * lin1, lin2, mlp_pointnet, mlp_merge: k_gemm_x3 / k_gemm - gemm_ref's x3_bound / gemm_bound as they are.
 * Object head: F.normalize(v) = v / max(||v||, 1e-12) with the norm summed in fp32:
       |d(v / n)| <= (|dv| + |v| (||dv|| / n + gamma_(D+4))) / n + 2 u |v| / n
   and the colour / position encoders 3 -> 64 -> D in fp32 fma.  object_head_emul chains dense_emul, those fma chains and an fp32
   normalize, so the head's two GEMMs are held by (B) as well.

Exact inputs (C): exact_objects / exact_weights at the end of this file - one chain from the points to features2 without a rounding."""
import ctypes
import hashlib

import numpy as np

import gemm_ref as G

U, ETA, F32 = G.U, G.ETA, G.F32
FACTOR_GPU = G.FACTOR_GPU
gamma = G.gamma

H = (32, 128, 256)          # hidden width of the SA levels
C = (64, 128, 256)          # output width
LD = (96, 160, 288)         # pitch of a traced sa_out row: [C | xyz 0 | 28 pad]
RADIUS = (0.2, 0.3, 0.4)
ORDERS = ("seq", "pairwise", "tile", "reversed", "random")
# (B): 4 x the largest ratio between the five orders' maxima, rounded up to a power of two (derived by derive_r, asserted by the host test)
R_SHARP = {"f16x3": dict(sa1=8.0, sa2=16.0, sa3=32.0, ga=64.0, lin1=64.0, lin2=16.0, head=32.0),
           "fp32": dict(sa1=16.0, sa2=32.0, sa3=32.0, ga=64.0, lin1=32.0, lin2=32.0, head=32.0)}
ARITH_WRONG = ("no_lo_hi", "no_hi_lo", "trunc_split", "no_drain_scale", "bias_unscaled", "max_from_zero")
ROW_WRONG = ("self_own", "drop33")
GA_WRONG = ("no_lo_hi", "no_hi_lo", "trunc_split", "ga_one_plane", "max_from_zero")


def level_geometry(n_pts):
    """[(n_dense, n_cent)] of the three SA levels (ops._level_geometry)."""
    out, nd = [], n_pts
    for _ in range(3):
        out.append((nd, (nd + 1) // 2))
        nd = out[-1][1]
    return out


def specialised(n_pts):
    """f16x3: the 256-point level shapes run k_sa_points / k_sa_rows / k_sa3 (LDS centroid tables); every other size, and fp32 at
    every size, runs k_sa_stream on HBM tables (cell_encoder.hip: Geo::specialised)."""
    return n_pts == 256


def ga_group(n_pts):
    """k_ga2<GP>: rows per max group = the next power of two >= n_cent of level 3."""
    nc, gp = level_geometry(n_pts)[2][1], 1
    while gp < nc:
        gp *= 2
    return gp


def kernels_reached(n_pts, precision, self_loops, tuning, want_nbr=True):
    """Which kernel and template each stage of a case reaches.  A HAND restatement of Chunk::group / sa_levels (cell_encoder.hip),
    sa_shares_tail_rows (t2p_common.h), launch_ws_sa (ws_sa.hip) and launch_ga2 (ga2.hip), as gemm_ref restates the tile rules:
    nothing ties it to the library, so it changes with those launchers."""
    x3, sp = precision == "f16x3", specialised(n_pts)
    prune_l0 = not (tuning & 1) and n_pts == 256
    mask_l0 = prune_l0 and not (tuning & 8) and not want_nbr
    return dict(
        scan="mask" if mask_l0 else "list",
        sa1_rows="k_build_rows" if mask_l0 else ("k_dedup_rows" if prune_l0 else "full"),
        prune_dup=bool(mask_l0 and not (tuning & 4) and not self_loops),
        share_tail=bool(x3 and sp and not (tuning & 4)),
        sa1="k_sa_points" if (x3 and sp) else "k_sa_stream<32,64,%s>" % ("x3" if x3 else "fp32"),
        sa2="k_sa_rows" if (x3 and sp) else "k_sa_stream<128,128,%s>" % ("x3" if x3 else "fp32"),
        sa3="k_sa3" if (x3 and sp) else "k_sa_stream<256,256,%s>" % ("x3" if x3 else "fp32"),
        ga2="k_ga2<%d>" % ga_group(n_pts) if x3 else "k_ws<DENSE_GROUPMAX, GP=%d>" % ga_group(n_pts),
        heads="k_gemm_x3" if x3 else "k_gemm")


# ---- grouping -------------------------------------------------------------------------------------------------------------------------

def oracle_groups(xyz, radius=RADIUS):
    """fps_idx / nbr / cnt of the three levels from oracle/primitives.c, in the layout of t2p_sample_group (int32; nbr 0 past cnt)."""
    from oracle import lib
    L = lib()
    n_obj, n_pts, _ = xyz.shape
    pos = np.ascontiguousarray(xyz, dtype=F32)
    out = dict(fps_idx=[], nbr=[], cnt=[], pos=[])
    fp = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    nd = n_pts
    for l in range(3):
        nc = (nd + 1) // 2
        idx = np.zeros((n_obj, nc), np.int32)
        L.t2p_oracle_fps(fp(pos, ctypes.c_float), ctypes.c_int64(n_obj), ctypes.c_int32(nd), ctypes.c_int32(nc), fp(idx, ctypes.c_int32))
        nbr = np.zeros((n_obj, nc, 32), np.int32)
        cnt = np.zeros((n_obj, nc), np.int32)
        L.t2p_oracle_ball_query(fp(pos, ctypes.c_float), fp(idx, ctypes.c_int32), ctypes.c_int64(n_obj), ctypes.c_int32(nd),
                                ctypes.c_int32(nc), ctypes.c_float(radius[l]), ctypes.c_int32(32), fp(nbr, ctypes.c_int32),
                                fp(cnt, ctypes.c_int32))
        out["fps_idx"].append(idx)
        out["nbr"].append(np.where(nbr < 0, 0, nbr))
        out["cnt"].append(cnt)
        pos = np.ascontiguousarray(np.take_along_axis(pos, idx[:, :, None].astype(np.int64), axis=1))
        out["pos"].append(pos)
        nd = nc
    return out


def edge_rows(nbr, cnt, cell_ptr, nd, nc, self_loops, wrong=None):
    """(src, dst): global dense rows [n_obj nd) and centroid rows [n_obj nc) of a level's edge rows, sorted by dst (hits in list
    order, then the loop row), from the nbr [n, nc, 32] / cnt [n, nc] tables and the self-loop rule of the module text.
    wrong: self_own (the loop row's source is the object's OWN dense row c) | drop33 (a centroid at the 32-hit cap loses its loop row)."""
    nbr, cnt = np.asarray(nbr).astype(np.int64), np.asarray(cnt).astype(np.int64)
    cell_ptr = np.asarray(cell_ptr).astype(np.int64)
    n = cnt.shape[0]
    first = np.repeat(cell_ptr[:-1], np.diff(cell_ptr))
    rank = np.arange(n) - first
    o, c, s = np.nonzero(np.arange(32)[None, None, :] < cnt[:, :, None])
    pt = nbr[o, c, s]
    if self_loops:
        keep = rank[o] * nd + pt != rank[o] * nc + c
        o, c, pt = o[keep], c[keep], pt[keep]
    src, dst = o * nd + pt, o * nc + c
    if self_loops:
        lo, lc = np.broadcast_to(np.arange(n)[:, None], (n, nc)), np.broadcast_to(np.arange(nc)[None, :], (n, nc))
        lsrc = first[:, None] * nd + rank[:, None] * nc + lc
        if wrong == "self_own":
            lsrc = lo * nd + lc
        on = np.ones((n, nc), bool) if wrong != "drop33" else cnt < 32
        src = np.concatenate([src, lsrc[on]])
        dst = np.concatenate([dst, (lo * nc + lc)[on]])
    order = np.argsort(dst, kind="stable")
    return src[order], dst[order]


# ---- small numeric helpers ----------------------------------------------------------------------------------------------------------

def _r32(x):
    """Round to fp32, keep a float64 container."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(F32).astype(np.float64)


def relu64(x):
    return np.where(x <= 0.0, 0.0, x)


def segmax(vals, dst, n_out, empty=0.0):
    """max of vals [E, N] over the rows of each dst (sorted ascending); segments without a row hold `empty`."""
    out = np.full((n_out, vals.shape[1]), empty, np.float64)
    if len(dst):
        starts = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]])
        out[dst[starts]] = np.maximum.reduceat(vals, starts, axis=0)
    return out


def split_f16(x, trunc=False, lo_scale=1.0):
    """(hi, lo) of the f16x3 split as float64: hi = fp16(x), lo = fp16(lo_scale (x - hi)) / lo_scale; to nearest, or by truncation."""
    def cvt(v):
        with np.errstate(over="ignore", invalid="ignore"):
            h = v.astype(np.float16)
            if trunc:
                big = np.abs(h.astype(np.float64)) > np.abs(v)
                h = np.where(big, np.nextafter(h, np.float16(0)), h)
            return h.astype(np.float64)
    x = np.asarray(x, np.float64)
    hi = cvt(x)
    return hi, cvt((x - hi) * lo_scale) / lo_scale


_FMA = [True]      # the fp32 emulations' default: one fma per k, or (False) a rounded product and an addition


def dot_ordered(a, w, order="tile", start=None, slab=16, fma=None, seed=0):
    """sum_k a[:, k] w[k, :] accumulated in fp32 in the given order, from `start` (a row, or None = 0).  a [M, K], w [K, N] float64
    holding values whose products are exact in float64 (fp16 x fp16, fp32 x fp32).  order: seq | reversed | random (one fma - or,
    fma=False, a rounded product and an addition - per k), tile (per `slab` k one exact block sum, rounded once: an MFMA step),
    pairwise (rounded products, a binary tree)."""
    m, k = a.shape
    n = w.shape[1]
    acc = np.zeros((m, n)) if start is None else np.broadcast_to(_r32(start), (m, n)).copy()
    fma = _FMA[0] if fma is None else fma
    prod = (lambda x, y: x * y) if fma else (lambda x, y: _r32(x * y))
    if order == "tile":
        for k0 in range(0, k, slab):
            acc = _r32(acc + a[:, k0: k0 + slab] @ w[k0: k0 + slab])
        return acc
    if order in ("seq", "reversed", "random"):
        ks = np.arange(k)
        if order == "reversed":
            ks = ks[::-1]
        elif order == "random":
            ks = np.random.default_rng(seed).permutation(k)
        for kk in ks:
            acc = _r32(acc + prod(a[:, kk: kk + 1], w[kk: kk + 1, :]))
        return acc
    if order == "pairwise":
        def tree(lo, hi):
            if hi - lo == 1:
                return _r32(a[:, lo: hi] * w[lo: hi, :])
            mid = (lo + hi) // 2
            return _r32(tree(lo, mid) + tree(mid, hi))
        return _r32(acc + tree(0, k)) if k else acc
    raise ValueError(order)


def _interleave(planes, k, slab):
    """[(a_p, w_p)] of equal K -> (a', w') with K' = len(planes) K: per slab of k, plane after plane - the MFMA issue order."""
    aa, ww = [], []
    for k0 in range(0, k, slab):
        for a, w in planes:
            aa.append(a[:, k0: k0 + slab])
            ww.append(w[k0: k0 + slab])
    return np.concatenate(aa, 1), np.concatenate(ww, 0)


def x3_single(a, w_scaled, order, wrong=None, slab=16, start=None):
    """The scaled single-accumulator f16x3 product: both operands split hi + lo, per slab hi.hi, hi.lo, lo.hi into one fp32 sum."""
    trunc = wrong == "trunc_split"
    ah, al = split_f16(a, trunc)
    wh, wl = split_f16(w_scaled)
    planes = [(ah, wh), (ah, wl), (al, wh)]
    if wrong in ("no_lo_hi", "ga_one_plane"):
        planes = [(ah, wh), (ah, wl)]
    elif wrong == "no_hi_lo":
        planes = [(ah, wh), (al, wh)]
    aa, ww = _interleave(planes, a.shape[1], slab)
    return dot_ordered(aa, ww, order, start=start, slab=slab)


def x3_double(a, w, bias, order, wrong=None, planes_in=None):
    """The two-accumulator form of k_ws / k_ga2 on pack_f16x3 images: acc = bias + sum hi.hi, accx = sum(hi.lo' + lo'.hi) with
    lo' = fp16(2048 (x - hi)); result fma(accx, 2^-11, acc).  planes_in: (hi, lo) of the activations as stored by the layer before."""
    trunc = wrong == "trunc_split"
    ah, al = split_f16(a, trunc, 2048.0) if planes_in is None else planes_in
    wh, wl = split_f16(w, False, 2048.0)
    acc = dot_ordered(ah, wh, order, start=bias)
    cross = [(ah, wl * 2048.0), (al * 2048.0, wh)]
    if wrong in ("no_lo_hi", "ga_one_plane"):
        cross = cross[:1]
    elif wrong == "no_hi_lo":
        cross = cross[1:]
    aa, ww = _interleave(cross, a.shape[1], 16)
    accx = dot_ordered(aa, ww, order)
    return _r32(acc + accx / 2048.0)


def _pad16(x, w):
    """Zero-pad K of (x [M, K], w [K, N]) to a multiple of 16 (the images' K; zero weights there)."""
    k = x.shape[1]
    kp = (k + 15) // 16 * 16
    if kp == k:
        return x, w
    return (np.concatenate([x, np.zeros((x.shape[0], kp - k))], 1), np.concatenate([w, np.zeros((kp - k, w.shape[1]))], 0))


# ---- SA levels ------------------------------------------------------------------------------------------------------------------------

def sa_ref64(feat, pos, cpos, src, dst, w1, b1, w2, b2):
    """One PointConv level in float64: message relu(W2 relu(W1 [x_j | pos_j - pos_i] + b1) + b2), max over the rows of a centroid
    (0 for a centroid without rows).  feat [Nd, Cin], pos [Nd, 3], cpos [Nc, 3] fp32; w1 [Cin + 3, H], w2 [H, C] k-major, folded.
    Returns dict(out [Nc, C], and the per-row intermediates the bound needs)."""
    feat, pos, cpos = (np.asarray(t, np.float64) for t in (feat, pos, cpos))
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (w1, b1, w2, b2))
    dp = pos[src] - cpos[dst]
    x = np.concatenate([feat[src], dp], 1)
    pre1 = x @ w1 + b1
    h = relu64(pre1)
    pre2 = h @ w2 + b2
    act2 = relu64(pre2)
    return dict(out=segmax(act2, dst, cpos.shape[0]), x=x, dp=dp, pre1=pre1, h=h, pre2=pre2, act2=act2)


def _table_terms(feat, pos, cpos, w1, b1, precision, relu=False):
    """err_A [Nd, H], err_B [Nc, H] of the layer-1 tables (module text)."""
    cin = feat.shape[1]
    xa = np.concatenate([np.asarray(feat, np.float64), np.asarray(pos, np.float64)], 1)
    a_star = xa @ w1 + b1
    ref = dict(act=relu64(a_star) if relu else a_star)
    err_a = G.x3_bound(xa, w1, 1.0, b1, ref) if precision == "f16x3" else G.gemm_bound(xa, w1, b1, ref)
    if cpos is None:
        return err_a, None
    wp = np.abs(w1[cin: cin + 3])
    cp = np.asarray(cpos, np.float64)
    err_b = gamma(4) * (np.abs(cp) @ wp) + U * np.abs(cp @ w1[cin: cin + 3])
    return err_a, err_b


def sa_bound(ref, feat, pos, cpos, src, dst, w1, b1, w2, b2, precision, scale, points_kernel):
    """Per-element bound of a level's output [Nc, C] (module text).  points_kernel: layer 1 per edge as k_sa_points does it
    (f16x3, level 1 of 256 points); else the A_j - B_i tables."""
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (w1, b1, w2, b2))
    cin = feat.shape[1]
    if points_kernel:
        assert precision == "f16x3"
        dp32 = _r32(np.asarray(pos, F32)[src] - np.asarray(cpos, F32)[dst])
        e = len(src)
        xaug = np.concatenate([np.asarray(feat, np.float64)[src], dp32, np.ones((e, 1)), np.zeros((e, 1))], 1)
        waug = np.concatenate([w1, b1[None, :], np.zeros((1, w1.shape[1]))], 0)
        e1 = G.x3_bound(xaug, waug, 1.0, None, dict(act=ref["pre1"])) + (U * np.abs(ref["dp"])) @ np.abs(w1[cin: cin + 3])
    else:
        err_a, err_b = _table_terms(feat, pos, cpos, w1, b1, precision)
        e1 = err_a[src] + err_b[dst]
        e1 = e1 + U * (np.abs(ref["pre1"]) + e1)
    hmag = ref["h"] + e1
    row_ref = dict(act=ref["act2"])
    if precision == "f16x3":
        l2 = G.x3_bound(hmag, w2, scale, b2, row_ref)
    else:
        l2 = G.gemm_bound(hmag, w2, b2, row_ref)
    rows = e1 @ np.abs(w2) + l2
    return segmax(rows, dst, ref["out"].shape[0]) + U * np.abs(ref["out"])


def _drain(y, dst, n_cent, b2, scale, wrong, biased):
    """max over a centroid's rows, bias, ReLU, 1 / s.  y [E, C] = the rows' accumulators (scaled by s); biased: they already hold s b2."""
    sb = _r32(np.asarray(b2, np.float64) * (1.0 if wrong == "bias_unscaled" else scale))
    raw = segmax(y, dst, n_cent, empty=-np.inf)
    if wrong == "max_from_zero":
        raw = np.maximum(raw, 0.0)
    r = np.maximum(raw if biased else _r32(raw + sb), 0.0)
    r = np.where(np.isfinite(r), r, 0.0)
    return r if wrong == "no_drain_scale" else _r32(r / scale)


def sa_emul(feat, pos, cpos, src, dst, w1, b1, w2, b2, precision, scale, points_kernel, order="tile", wrong=None):
    """NumPy emulation of a level's documented arithmetic (module text); returns out [Nc, C] (float64 holding fp32 values).
    wrong (f16x3): no_lo_hi | no_hi_lo | trunc_split | no_drain_scale | bias_unscaled | max_from_zero (the row-set variants are
    edge_rows')."""
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (w1, b1, w2, b2))
    feat64, pos32, cpos32 = np.asarray(feat, np.float64), np.asarray(pos, F32), np.asarray(cpos, F32)
    cin, e = feat.shape[1], len(src)
    x3 = precision == "f16x3"
    if points_kernel:
        dp32 = (pos32[src] - cpos32[dst]).astype(np.float64)
        xaug = np.concatenate([feat64[src], dp32, np.ones((e, 1)), np.zeros((e, 1))], 1)
        waug = np.concatenate([w1, b1[None, :], np.zeros((1, w1.shape[1]))], 0)
        pre1 = x3_single(xaug, waug, order, wrong if wrong == "trunc_split" else None, slab=8)
    else:
        xa = np.concatenate([feat64, pos32.astype(np.float64)], 1)
        if x3:
            xp, wp_ = _pad16(xa, w1)
            a_tab = x3_double(xp, wp_, b1, order, wrong if wrong == "trunc_split" else None)
        else:
            a_tab = dot_ordered(xa, w1, order, start=b1)
        c64, wp = cpos32.astype(np.float64), w1[cin: cin + 3]
        b_tab = _r32(_r32(_r32(c64[:, 0:1] * wp[0:1]) + c64[:, 1:2] * wp[1:2]) + c64[:, 2:3] * wp[2:3])
        pre1 = _r32(a_tab[src] - b_tab[dst])
    h = relu64(pre1)
    if x3:
        y = x3_single(h, w2 * scale, order, wrong)
        return _drain(y, dst, cpos.shape[0], b2, scale, wrong, False)
    y = dot_ordered(h, w2, order, start=b2)
    return _drain(y, dst, cpos.shape[0], b2, 1.0, None, True)


# ---- GA ---------------------------------------------------------------------------------------------------------------------------------

def ga_ref64(feat, pos, n_obj, w1, b1, w2, b2):
    """features0 [n_obj, 1024]: relu(W2 relu(W1 [F | xyz] + b1) + b2), max over the object's rows.  feat [n_obj nc, 256], pos [.., 3]."""
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (w1, b1, w2, b2))
    x = np.concatenate([np.asarray(feat, np.float64), np.asarray(pos, np.float64)], 1)
    pre1 = x @ w1 + b1
    h = relu64(pre1)
    act2 = relu64(h @ w2 + b2)
    nc = x.shape[0] // n_obj
    return dict(out=act2.reshape(n_obj, nc, -1).max(1), x=x, pre1=pre1, h=h, act2=act2)


def ga_bound(ref, feat, pos, n_obj, w1, b1, w2, b2, precision):
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (w1, b1, w2, b2))
    e1, _ = _table_terms(feat, pos, None, w1, b1, precision, relu=True)
    hmag = ref["h"] + e1
    row_ref = dict(act=ref["act2"])
    l2 = G.x3_bound(hmag, w2, 1.0, b2, row_ref) if precision == "f16x3" else G.gemm_bound(hmag, w2, b2, row_ref)
    rows = e1 @ np.abs(w2) + l2
    nc = rows.shape[0] // n_obj
    return rows.reshape(n_obj, nc, -1).max(1) + U * np.abs(ref["out"])


def ga_emul(feat, pos, n_obj, w1, b1, w2, b2, precision, order="tile", wrong=None):
    """wrong (f16x3): no_lo_hi | no_hi_lo (layer 2) | trunc_split | ga_one_plane (the hidden row kept as its hi plane only) |
    max_from_zero (the max starts at 0 BEFORE the bias)."""
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (w1, b1, w2, b2))
    x = np.concatenate([np.asarray(feat, np.float64), np.asarray(pos, np.float64)], 1)
    nc = x.shape[0] // n_obj
    if precision == "f16x3":
        xp, wp_ = _pad16(x, w1)
        tr = wrong if wrong == "trunc_split" else None
        h = relu64(x3_double(xp, wp_, b1, order, tr))
        planes = split_f16(h, wrong == "trunc_split", 2048.0)
        if wrong == "max_from_zero":
            y = x3_double(h, w2, None, order, None, planes)
            raw = np.maximum(y.reshape(n_obj, nc, -1).max(1), 0.0)
            return np.maximum(_r32(raw + b2), 0.0)
        y = x3_double(h, w2, b2, order, wrong if wrong != "trunc_split" else None, planes)
    else:
        h = relu64(dot_ordered(x, w1, order, start=b1))
        y = dot_ordered(h, w2, order, start=b2)
    return np.maximum(y.reshape(n_obj, nc, -1).max(1), 0.0)


# ---- lin1 / lin2 / mlp_pointnet / mlp_merge: one dense layer ---------------------------------------------------------------------------

def dense_ref64(a, w, b, relu=True):
    return G.gemm_ref64(np.asarray(a, F32), np.asarray(w, F32), np.asarray(b, F32), relu)["act"]


def dense_bound(ref, a, w, b, precision, scale):
    r = dict(act=ref, out=ref)
    a, w, b = np.asarray(a, F32), np.asarray(w, F32), np.asarray(b, F32)
    return G.x3_bound(a, w, scale, b, r) if precision == "f16x3" else G.gemm_bound(a, w, b, r)


def dense_emul(a, w, b, precision, scale, order="tile", wrong=None, relu=True):
    """k_gemm_x3 (scaled single accumulator, v = fma(acc, 1 / s, b)) / k_gemm (fma chain + b).  wrong: no_lo_hi | no_hi_lo |
    trunc_split | no_drain_scale."""
    a, w, b = np.asarray(a, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    if precision == "f16x3":
        ap, wp_ = _pad16(a, w * scale)
        acc = x3_single(ap, wp_, order, wrong)
        v = _r32(acc * (1.0 if wrong == "no_drain_scale" else 1.0 / scale) + b)
    else:
        v = _r32(dot_ordered(a, w, order) + b)
    return relu64(v) if relu else v


# ---- object head ------------------------------------------------------------------------------------------------------------------------

def normalize64(v):
    n = np.sqrt((v * v).sum(1, keepdims=True))
    return v / np.maximum(n, 1e-12)


def normalize_bound(v, dv):
    """|F.normalize(v + d) computed in fp32 - F.normalize(v)| for |d| <= dv (module text)."""
    d = v.shape[1]
    n = np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1e-12)
    rel = np.sqrt((dv * dv).sum(1, keepdims=True)) / n + gamma(d + 4)
    return (dv + np.abs(v) * rel) / n / (1.0 - np.minimum(rel, 0.5)) + 2 * U * np.abs(v) / n


def mlp3_ref64(x3, w1, b1, w2, b2):
    """Colour / position encoder: relu(W2 relu(W1 x + b1) + b2), then F.normalize.  Returns (pre-normalisation, normalised, hidden)."""
    x3, w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (x3, w1, b1, w2, b2))
    h = relu64(x3 @ w1 + b1)
    v = relu64(h @ w2 + b2)
    return v, normalize64(v), h


def mlp3_bound(x3, w1, b1, w2, b2, v, h):
    x3, w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (x3, w1, b1, w2, b2))
    e1 = gamma(5) * (np.abs(x3) @ np.abs(w1) + np.abs(b1)) + U * h
    e2 = e1 @ np.abs(w2) + gamma(w2.shape[0] + 2) * ((h + e1) @ np.abs(w2) + np.abs(b2)) + U * v
    return normalize_bound(v, e2)


def object_head_ref64(feat, center, mean_rgb, p, use=("class", "color", "position")):
    """obj_emb and its bound-relevant pieces.  feat: the traced features{pointnet_features}; p: the folded fp32 pack (NumPy)."""
    parts, pieces = [], {}
    if "class" in use:
        v = dense_ref64(feat, p["pn_w"], p["pn_b"])
        parts.append(normalize64(v))
        pieces["pn"] = v
    for name, pre, src in (("color", "col", mean_rgb), ("position", "pos", center)):
        if name in use:
            v, nv, h = mlp3_ref64(src, p[pre + "_w1"], p[pre + "_b1"], p[pre + "_w2"], p[pre + "_b2"])
            parts.append(nv)
            pieces[pre] = (v, h)
    cat = np.concatenate(parts, 1)
    pieces["cat"] = cat
    out = cat if len(parts) == 1 else G.gemm_ref64(cat.astype(np.float64), np.asarray(p["merge_w"], np.float64),
                                                   np.asarray(p["merge_b"], np.float64), True)["act"]
    pieces["out"] = out
    return pieces


def object_head_bound(pieces, feat, center, mean_rgb, p, precision, use=("class", "color", "position")):
    errs = []
    if "class" in use:
        e = dense_bound(pieces["pn"], feat, p["pn_w"], p["pn_b"], precision, p.get("pn_scale", 1.0))
        errs.append(normalize_bound(pieces["pn"], e))
    for name, pre, src in (("color", "col", mean_rgb), ("position", "pos", center)):
        if name in use:
            v, h = pieces[pre]
            errs.append(mlp3_bound(src, p[pre + "_w1"], p[pre + "_b1"], p[pre + "_w2"], p[pre + "_b2"], v, h))
    ecat = np.concatenate(errs, 1)
    if len(errs) == 1:
        return ecat
    w, b = np.asarray(p["merge_w"], np.float64), np.asarray(p["merge_b"], np.float64)
    cat = np.abs(pieces["cat"]) + ecat
    r = dict(act=pieces["out"], out=pieces["out"])
    own = G.x3_bound(cat, w, p.get("merge_scale", 1.0), b, r) if precision == "f16x3" else G.gemm_bound(cat, w, b, r)
    return ecat @ np.abs(w) + own


def normalize_emul(v):
    """F.normalize in fp32: rounded squares summed in fp32, sqrt, one division per element."""
    v = _r32(v)
    ss = np.zeros((v.shape[0], 1))
    for k in range(v.shape[1]):
        ss = _r32(ss + _r32(v[:, k: k + 1] * v[:, k: k + 1]))
    n = np.maximum(_r32(np.sqrt(ss)), 1e-12)
    return _r32(v / n)


def object_head_emul(feat, center, mean_rgb, p, precision, order="tile", wrong=None, use=("class", "color", "position")):
    """The object head's documented arithmetic: mlp_pointnet and mlp_merge as dense_emul (k_gemm_x3 / k_gemm), the colour / position
    encoders as fp32 fma chains from the bias, F.normalize in fp32.  wrong: dense_emul's (both GEMMs)."""
    parts = []
    if "class" in use:
        parts.append(normalize_emul(dense_emul(feat, p["pn_w"], p["pn_b"], precision, p.get("pn_scale", 1.0), order, wrong)))
    for name, pre, src in (("color", "col", mean_rgb), ("position", "pos", center)):
        if name in use:
            w1, b1, w2, b2 = (np.asarray(p[pre + k], np.float64) for k in ("_w1", "_b1", "_w2", "_b2"))
            h = relu64(dot_ordered(np.asarray(src, np.float64), w1, "seq", start=b1))
            parts.append(normalize_emul(relu64(dot_ordered(h, w2, order, start=b2))))
    cat = np.concatenate(parts, 1)
    if len(parts) == 1:
        return cat
    return dense_emul(cat, p["merge_w"], p["merge_b"], precision, p.get("merge_scale", 1.0), order, wrong)


# ---- assertions ---------------------------------------------------------------------------------------------------------------------------

def within(got, ref, bound, factor=FACTOR_GPU):
    return G.within(got, ref, bound, factor)


worst_ratio = G.worst_ratio


def max_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) if np.size(ref) else 0.0


def sharp_threshold(emul, ref, precision, stage):
    """R max(max|emul - ref64|, u max|ref64|) of assertion (B)."""
    return R_SHARP[precision][stage] * max(max_err(emul, ref), U * float(np.abs(ref).max()))


def derive_r(maxima):
    """4 x (largest / smallest of the orders' maxima), rounded up to a power of two."""
    ratio = max(maxima) / min(maxima)
    return float(2.0 ** np.ceil(np.log2(4.0 * ratio)))


def digest(*arrays):
    """Key of a reference cache: stage references depend on the stage's inputs alone, and cases that differ only in their
    execution plan (tuning, chunking) hand the same bits to a stage."""
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.shape, a.dtype)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

CELL_SIZES = (1, 2, 5, 9, 23)      # a single-object cell, aliasing across objects, a cell longer than one 8-destination group
ODD_KINDS = {3: "few", 7: "dense", 12: "sparse", 20: "few", 33: "dense"}   # object -> tests/tools/fuzz_cells.odd_object kind


def _case(name, precision="f16x3", self_loops=True, tuning=0, n_pts=256, features=2, chunk=0, seed=11, rescale=None, one_cell=False,
          full_trace=True):
    return dict(name=name, precision=precision, self_loops=self_loops, tuning=tuning, n_pts=n_pts, features=features, chunk=chunk,
                seed=seed, rescale=rescale, one_cell=one_cell, full_trace=full_trace)


# The smallest list that reaches every branch (not a cross product).  full_trace=False leaves nbr / cnt out of the trace: only then
# does the encoder take its default plan (SA1's rows from hit masks, the pruned SA2 / SA3 lists without self loops); the row sets then
# come from oracle/primitives.c, which test_sample_group_bit_exact and the full-trace cases hold the kernel's tables to.
CASES = [
    _case("x3"), _case("fp32", precision="fp32"),
    _case("x3-noloops", self_loops=False), _case("fp32-noloops", precision="fp32", self_loops=False),
    _case("x3-maskplan", full_trace=False), _case("x3-maskplan-noloops", self_loops=False, full_trace=False),
    _case("fp32-maskplan-noloops", precision="fp32", self_loops=False, full_trace=False),
    _case("x3-tuning-d", tuning=0xD), _case("x3-tuning-1", tuning=1), _case("x3-tuning-4", tuning=4, full_trace=False),
    _case("x3-noloops-tuning-4", tuning=4, self_loops=False, full_trace=False), _case("x3-tuning-8", tuning=8, full_trace=False),
    _case("x3-100", n_pts=100), _case("fp32-100", precision="fp32", n_pts=100), _case("x3-64", n_pts=64),
    _case("x3-8", n_pts=8), _case("fp32-8", precision="fp32", n_pts=8), _case("x3-100-noloops", n_pts=100, self_loops=False),
    _case("x3-features0", features=0), _case("x3-features1", features=1), _case("fp32-features0", precision="fp32", features=0),
    _case("x3-chunk8", chunk=8), _case("fp32-chunk8", precision="fp32", chunk=8),
    _case("x3-fill12", seed=12), _case("fp32-fill12", precision="fp32", seed=12),
] + [_case("x3-%s-%s" % (row.replace(" ", "-"), tag), rescale=(row, s))
     for row in ("sa2 hidden", "sa3 output", "ga hidden") for tag, s in (("up", 2.0 ** 4), ("down", 2.0 ** -3))] + [
    _case("x3-onecell", one_cell=True), _case("fp32-onecell", precision="fp32", one_cell=True),
]


def case_objects(n_pts=256, one_cell=False):
    """(xyz, rgb, center, mean_rgb, cell_ptr) of every case: 40 synthetic objects in cells of CELL_SIZES (or one cell), objects
    ODD_KINDS replaced by fuzz_cells' odd ones - "few" (2 - 5 distinct points: tail centroids), "dense" (every ball at the 32-hit cap)
    and "sparse" (balls that hold their centre only); the first n_pts points of each."""
    import importlib.util
    import os
    from text2pos_amd import synthetic as S
    spec = importlib.util.spec_from_file_location("fuzz_cells", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "fuzz_cells.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    n = sum(CELL_SIZES)
    xyz, rgb, center, mean_rgb = (a.copy() for a in S.make_objects(4242, 0, n))
    rng = np.random.default_rng(7)
    for o, kind in sorted(ODD_KINDS.items()):
        xyz[o] = fz.odd_object(rng, kind)
    xyz[20][:] = xyz[20][np.arange(256) % 3]          # exactly the object's first 3 points, whatever n_pts keeps
    xyz, rgb = np.ascontiguousarray(xyz[:, :n_pts]), np.ascontiguousarray(rgb[:, :n_pts])
    ptr = np.array([0, n] if one_cell else np.concatenate([[0], np.cumsum(CELL_SIZES)]), np.int32)
    return xyz, rgb, center, mean_rgb, ptr


# ---- exact inputs: one chain without rounding -------------------------------------------------------------------------------------------
# Points on the 2^-4 grid, colours on the 2^-8 grid; every trunk matrix holds two taps per output column, +-1/2 (+-1/4 too in SA
# level 1), and biases in {-1, -1/2, 0, 1/2, 1}; the BatchNorms are folded already: the designed matrices ARE the folded ones handed
# to the library.  Units (every value a multiple of): colours 2^-8, SA1 hidden 2^-10, SA1 out 2^-12, then one bit per layer - SA2
# 2^-13 / 2^-14, SA3 2^-15 / 2^-16, GA 2^-17 / 2^-18, features1 2^-19, features2 2^-20 - and every activation below 4 (checked on
# the data by exact_headroom(), stage by stage).  So an activation that is read again has at most 21 significant bits and is
# hi + lo exactly (hi's spacing below 4 is at most 2^-9, the residual at most 2^-10 <= 2^9 units: within lo's 11 bits); a product
# of a tap and an activation is a multiple of half the unit, and a partial sum of an output's two products and bias is below
# 2 + 2 + 1 < 8 <= 2^23 such multiples: exact in fp32 in any order, with or without fma; s w is a power of two.  From SA level 2
# on 5 - 10 % of the activations carry a lo plane (12 and more significant bits; in k_sa_points' hidden layer only a few rows do).
# Single-plane weights: hi.hi and lo.hi carry everything, hi.lo is zero.
# The probe channel.  Channel 0 of every layer carries EXACT_PROBE = 1 + 2^-10 - 2^-22 from SA1's hidden layer (no tap, that bias)
# to features2 (one tap of 1 on channel 0 of the layer before, bias 0; no other column reads channel 0).  To nearest it splits
# hi = 1 + 2^-10, lo = -2^-22: exact.  By truncation hi = 1 and the residual 2^-10 - 2^-22 needs 12 bits: a kernel that splits its
# activations by truncation loses 2^-22 at every split site (k_sa_points' hidden rows, the k_ws table inputs, the SA2 / SA3 hidden
# rows, GA's hidden planes, the inputs of lin1 and lin2) and returns other bits in column 0.  With the tap of 1 the largest |w| is
# 1 and the scale of every scaled image 2^14.
#
# Two-plane sets, one per MFMA stage (two_plane = "sa1" | "sa2" | "sa3" | "ga"), for hi.lo: points AND colours on the 2^-4 grid,
# every matrix ONE tap of +-1 per output column and biases in {-1, 0, 1} - so every activation in front of the stage is a multiple
# of 2^-4 below 16 (a layer adds at most 1: 2 + 8; checked on the data): 8 bits, a single fp16 plane.  The stage's second layer
# holds w = r + t 2^-13 on its taps (r, t = +-1).  Scaled image: f16x3_scale gives s = 2^13, s w = +-8192 +- 1, fp16's spacing
# there is 4 or 8, so hi = +-8192 and lo = +-1 exactly; the unscaled pack_f16x3 image of GA: hi = +-1 (spacing 2^-11 or 2^-10),
# lo' = 2048 t 2^-13 = +-1/4.  An output is h (r + t 2^-13) + b2: a multiple of 2^-17 below 17, 22 bits - exact in fp32, and all
# of its t part travels through hi.lo.  The chain is checked up to that stage; behind it the activations have 22 bits.

EXACT_GRID, EXACT_GRID_RGB = 2.0 ** -4, 2.0 ** -8
EXACT_PROBE = 1.0 + 2.0 ** -10 - 2.0 ** -22


TWO_PLANE_STAGES = ("sa1", "sa2", "sa3", "ga")


def exact_objects(two_plane=None):
    """The cases' objects snapped to the 2^-4 grid, their colours to the 2^-8 grid (two-plane sets: 2^-4 as well)."""
    xyz, rgb, center, mean_rgb, ptr = case_objects()
    snap = lambda a, g: (np.round(a / g) * g).astype(F32)
    return snap(xyz, EXACT_GRID), snap(rgb, EXACT_GRID if two_plane else EXACT_GRID_RGB), center, mean_rgb, ptr


def exact_weights(seed=5, two_plane=None):
    """The trunk's folded matrices in the layout of packing._pack_pointnet_fp32 (k-major, K zero-padded), designed as above.
    Every fourth output column of a second layer is negative on every row: negative taps on non-negative inputs, bias -1/2.
    two_plane: the single-tap set whose stage `two_plane` has the two-plane second layer."""
    rng = np.random.default_rng(seed)
    if two_plane is not None:
        assert two_plane in TWO_PLANE_STAGES

        def tap(k_real, k_pad, n, dead_every=0, planes=False):
            w = np.zeros((k_pad, n), F32)
            b = rng.choice([-1.0, 0.0, 1.0], n).astype(F32)
            rows = rng.integers(0, k_real, n)
            r = rng.choice([-1.0, 1.0], n)
            if dead_every:
                dead = np.arange(n) % dead_every == dead_every - 1
                r[dead], b[dead] = -1.0, -1.0
            t = rng.choice([-1.0, 1.0], n) * 2.0 ** -13 if planes else 0.0
            w[rows, np.arange(n)] = (r + t).astype(F32)
            return w, b
        p = dict(sa_w1=[], sa_b1=[], sa_w2=[], sa_b2=[])
        for l, (cin, kpad) in enumerate(((3, 6), (64, 96), (128, 160))):
            w1, b1 = tap(cin + 3, kpad, H[l])
            w2, b2 = tap(H[l], H[l], C[l], 4, two_plane == "sa%d" % (l + 1))
            p["sa_w1"].append(w1), p["sa_b1"].append(b1), p["sa_w2"].append(w2), p["sa_b2"].append(b2)
        p["ga_w1"], p["ga_b1"] = tap(259, 288, 512)
        p["ga_w2"], p["ga_b2"] = tap(512, 512, 1024, 4, two_plane == "ga")
        p["lin1_w"], p["lin1_b"] = tap(1024, 1024, 512)
        p["lin2_w"], p["lin2_b"] = tap(512, 512, 256)
        return p

    def layer(k_real, k_pad, n, vals, dead_every=0, carry=None):
        """carry: what output column 0 does - "make": no tap, bias EXACT_PROBE; "pass": one tap of 1 on input 0, bias 0.  No other
        column taps input 0 of a layer behind SA1's first."""
        w = np.zeros((k_pad, n), F32)
        b = rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], n).astype(F32)
        for col in range(n):
            rows = rng.choice(k_real, 2, replace=False) if carry == "make" else 1 + rng.choice(k_real - 1, 2, replace=False)
            w[rows, col] = rng.choice(vals, 2)
            if dead_every and col % dead_every == dead_every - 1:
                w[rows, col] = -np.abs(w[rows, col])
                b[col] = -0.5
        w[:, 0] = 0.0
        if carry == "make":
            b[0] = EXACT_PROBE
        else:
            w[0, 0], b[0] = 1.0, 0.0
        return w, b
    half, quarter = [-0.5, 0.5], [-0.5, -0.25, 0.25, 0.5]
    p = dict(sa_w1=[], sa_b1=[], sa_w2=[], sa_b2=[])
    for l, (cin, kpad) in enumerate(((3, 6), (64, 96), (128, 160))):
        vals = quarter if l == 0 else half
        w1, b1 = layer(cin + 3, kpad, H[l], vals, 0, "make" if l == 0 else "pass")
        w2, b2 = layer(H[l], H[l], C[l], vals, 4, "pass")
        p["sa_w1"].append(w1), p["sa_b1"].append(b1), p["sa_w2"].append(w2), p["sa_b2"].append(b2)
    p["ga_w1"], p["ga_b1"] = layer(259, 288, 512, half, 0, "pass")
    p["ga_w2"], p["ga_b2"] = layer(512, 512, 1024, half, 4, "pass")
    p["lin1_w"], p["lin1_b"] = layer(1024, 1024, 512, half, 0, "pass")
    p["lin2_w"], p["lin2_b"] = layer(512, 512, 256, half, 0, "pass")
    return p


def exact_headroom(x, unit, top):
    """The premises of exactness on data: every element a multiple of `unit`, every magnitude below `top`."""
    x = np.asarray(x, np.float64)
    return bool(np.all(x / unit == np.round(x / unit)) and np.all(np.abs(x) < top))
