"""Shared by tests/test_gpu_cell_head.py and tests/test_cell_head_ref_host.py: everything behind obj_emb - Chunk::cell_head of
csrc/cell_encoder.hip - ONE STAGE AT A TIME, built on tests/trunk_ref.py and tests/gemm_ref.py (whose dense_*, normalize_*, x3_*,
split_f16, segmax, within, max_err, sharp_threshold, derive_r and FACTOR_GPU are used as they are).  Stages, each stated on the
stage's own input - on the GPU the kernel's traced upstream output (t2p_cell_trace.head_*), so errors do not compound and the one
discrete step, the kNN graph, never stands between a kernel and its reference:

  in    head_in   = F.normalize(obj_emb)                               k_rownorm
  knn   knn_idx   = the kNN of oracle/primitives.c on head_in          k_knn - a pure function of head_in's bits: BIT EQUAL, no
                                                                       near-tie allowance at this level, no cell excused
  edge  head_edge = aggr_j relu(relu(x_i Wp + bp + x_j Wq) W2 + b2)    the two split products P, Q (launch_dense: k_gemm_x3 / k_gemm),
                    over the traced neighbours j of i; aggr = max       then WS_EDGE_KNN of csrc/ws_gemm.hip
                    (variation 0) or mean over the valid count (1)
  pool  head_pool = max / mean over the cell's rows of head_edge       k_segpool
  l1    head_l1   = relu(head_pool W + b); l2 the same on head_l1      launch_gemm (fp32 in BOTH precisions)
  out   out       = F.normalize(head_l2)                               k_rownorm

Per stage (a) `*_ref64`, (b) `*_bound`, (c) `*_emul(order=, wrong=)` as in trunk_ref.  The GPU test asserts (A) |kernel - ref64| <=
2 bound on every element of every stage, (B) max|kernel - ref64| <= R max(max|emul - ref64|, u max|ref64|) for edge, l1 and l2 with
R = R_SHARP below, and (C) bit equality with fp32(ref64) on the exact family at the end of this file.

Documented arithmetic (u = 2^-24; gamma_n, the f16x3 split model and its bounds: gemm_ref).
 * in / out: trunk_ref.normalize_bound with no input error (the stage's input is what the kernel read).
 * P = x Wp + bp, Q = x Wq: gemm_ref's x3_bound (k_gemm_x3: the scaled single accumulator, v = fma(acc, 1 / s, b)) or gemm_bound.
 * edge rows: h = relu(fp32(P_i + Q_j)).  As sa_bound composes the table errors through layer 2:
       e1 = err_P[i] + err_Q[j] + u (|P_i + Q_j| + err_P[i] + err_Q[j])
   f16x3 layer 2 on pack_f16x3 images (hi, lo' = fp16(2048 (x - hi)) of h and of W2), two accumulators acc = b2 + sum hi.hi, accx =
   sum(hi.lo' + lo'.hi), y = fma(accx, 2^-11, acc): x3_bound(|h| + e1, W2, 1, b2) as for GA layer 2; fp32: gemm_bound (fma chains
   of v_mfma_f32_32x32x2_f32).  Lane half h owns k in [h K / 2, (h + 1) K / 2), so MFMA step s holds k = 8 s .. 8 s + 7 of BOTH
   halves (f16x3) or k = s of both (fp32): the emulation's "tile" order walks K in that order (mfma_k_order).
       row[r] = e1[r] |W2| + layer2[r]
   max (signed-int LDS atomicMax against +0 = the ReLU): bound[i] = max over i's rows of row[r] + u |out[i]|;
   mean (8 slots per destination, rows 0-3 summed in order, then rows 4-7, the halves added, one division by the VALID count n_i):
       bound[i] = (sum row[r] + gamma_9 sum(relu(y*[r]) + row[r])) / n_i + u |out[i]|.
 * pool: max is exact (bound 0: bit equality); mean is k_segpool's sequential sum and one division:
       gamma_n sum|x| / n + u |out|.

Wrong emulations (wrong=).  trunk_ref.ARITH_WRONG's names where they apply - at edge: no_lo_hi, no_hi_lo, trunc_split on the three
products, no_drain_scale (accx added without its 2^-11), bias_unscaled (P = (acc + bp) / s); at l1 / l2, which run in fp32 by
design: the layer handed to the f16x3 GEMM with no_lo_hi / no_hi_lo (a wrong dispatch AND a lost plane; a correct f16x3 GEMM or a
truncating split sits inside R of the fp32 chain, see docs/notebook.md).  The head's own: max_from_neg_inf (aggregation without the
implicit ReLU), mean_over_k (divide by knn_k, not by the valid count), neighbour_off_by_one (row j + 1), wq_on_i (Q taken at the
destination), pool_from_zero.  pool_from_zero cannot be told apart on ANY input: head_edge is >= 0 behind its ReLU, so a max that
starts at 0 returns the same bits - it is listed in NOT_SEPARATED and in no stage's list."""
import ctypes

import numpy as np

import gemm_ref as G
import trunk_ref as T

U, F32 = T.U, T.F32
FACTOR_GPU = T.FACTOR_GPU
gamma = T.gamma
KNN_K = 8
KNN_MAX_ROWS, KNN_STAGE = 192, 64          # launch_knn / kKnnStage of csrc/small_kernels.hip
DEFAULT_CHUNK = 65000                      # T2P_DEFAULT_CHUNK_OBJECTS
HEAD_TRACE = ("head_in", "head_edge", "head_pool", "head_l1", "head_l2")
SHARP_STAGES = ("edge", "l1", "l2")
PLANES = ("no_lo_hi", "no_hi_lo", "trunc_split")

# (B): derive_r over the five summation orders of trunk_ref.ORDERS, the largest over the cases the GPU test runs (embedding-path
# tables at D = 256, 128, 64 -> 128 and 300 -> 384, max and mean); re-derived and asserted by tests/test_cell_head_ref_host.py,
# the maxima are recorded in docs/notebook.md ("The cell head held to float64 bounds").
R_SHARP = {"f16x3": dict(edge=32.0, l1=32.0, l2=16.0), "fp32": dict(edge=32.0, l1=32.0, l2=16.0)}
# wrong emulations per stage: every one of them lands above the (B) threshold of its stage in every case (host test)
EDGE_WRONG = {"f16x3": ("no_lo_hi", "no_hi_lo", "no_drain_scale", "bias_unscaled", "max_from_neg_inf", "mean_over_k",
                        "neighbour_off_by_one", "wq_on_i"),
              "fp32": ("max_from_neg_inf", "mean_over_k", "neighbour_off_by_one", "wq_on_i")}
LIN_WRONG = ("no_lo_hi", "no_hi_lo")
# not told apart by (B) at their stage (docs/notebook.md): trunc_split at edge only doubles the split error (the exact family's
# probe channel carries it); pool_from_zero never changes a bit
NOT_SEPARATED = {"edge": ("trunc_split",), "pool": ("pool_from_zero",), "l1": ("trunc_split",), "l2": ("trunc_split",)}


def _register_r():
    """trunk_ref.sharp_threshold looks R up in trunk_ref.R_SHARP: the head's stages go in under `head_<stage>`."""
    for precision, table in R_SHARP.items():
        for stage, r in table.items():
            T.R_SHARP[precision]["head_" + stage] = r


_register_r()


def sharp_threshold(emul, ref, precision, stage):
    return T.sharp_threshold(emul, ref, precision, "head_" + stage)


def x3_scale(w):
    """packing.f16x3_scale in NumPy: the largest power of two s with max|s w| <= 2^14, clipped to [2^-8, 2^15]."""
    m = float(np.abs(w).max())
    return 1.0 if m == 0.0 else float(2.0 ** max(-8, min(15, int(np.floor(np.log2(2.0 ** 14 / m))))))


def head_pack(p):
    """The cell head's part of a folded pack (NumPy), with the scales of the P / Q images."""
    out = {k: np.asarray(p[k], F32) for k in ("g_wp", "g_bp", "g_wq", "g_w2", "g_b2", "lin_w1", "lin_b1", "lin_w2", "lin_b2")}
    for k in ("g_wp", "g_wq"):
        out[k + "_scale"] = float(p[k + "_scale"]) if p.get(k + "_scale") is not None else x3_scale(out[k])
    return out


# ---- the graph --------------------------------------------------------------------------------------------------------------------------

def chunks(cell_ptr, chunk_objects=0):
    """[(c0, c1)] of next_chunk_end (cell_encoder.hip): whole cells, at most chunk_objects objects, a larger cell on its own."""
    cp = np.asarray(cell_ptr).astype(np.int64)
    chunk = chunk_objects if chunk_objects > 0 else DEFAULT_CHUNK
    out, c0, n_cells = [], 0, len(cp) - 1
    while c0 < n_cells:
        c1 = c0 + 1
        while c1 < n_cells and cp[c1 + 1] - cp[c0] <= chunk:
            c1 += 1
        out.append((c0, c1))
        c0 = c1
    return out


def global_rows(knn, cell_ptr, chunk_objects=0):
    """The traced knn_idx (rows local to the call's internal chunk) as global object rows; -1 stays."""
    knn = np.asarray(knn).astype(np.int64)
    cp = np.asarray(cell_ptr).astype(np.int64)
    start = np.zeros(knn.shape[0], np.int64)
    for c0, c1 in chunks(cp, chunk_objects):
        start[cp[c0]: cp[c1]] = cp[c0]
    return np.where(knn >= 0, knn + start[:, None], -1)


def knn_oracle(embn, cell_ptr, k=KNN_K):
    """oracle/primitives.c's kNN (global rows, -1 past the cell's size) on the fp32 rows `embn` AS GIVEN."""
    from oracle import lib
    x = np.ascontiguousarray(embn, F32)
    ptr = np.ascontiguousarray(cell_ptr, np.int32)
    out = np.zeros((x.shape[0], k), np.int32)
    fp = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    lib().t2p_oracle_knn(fp(x, ctypes.c_float), fp(ptr, ctypes.c_int32), ctypes.c_int32(len(ptr) - 1), ctypes.c_int32(x.shape[1]),
                         ctypes.c_int32(k), fp(out, ctypes.c_int32))
    return out.astype(np.int64)


def edge_rows(knn, wrong=None, dsts=None):
    """(src, dst, slot) of the valid entries of knn [n, k] (global rows), sorted by dst then slot.  dsts: these destinations only
    (dst then counts 0 .. len(dsts) - 1).  wrong: neighbour_off_by_one."""
    knn = np.asarray(knn).astype(np.int64)
    n = knn.shape[0]
    sub = knn if dsts is None else knn[np.asarray(dsts)]
    dst, slot = np.nonzero(sub >= 0)
    src = sub[dst, slot]
    if wrong == "neighbour_off_by_one":
        src = np.minimum(src + 1, n - 1)
    return src, dst, slot


def _segsum(vals, dst, n_out):
    out = np.zeros((n_out, vals.shape[1]))
    if len(dst):
        starts = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]])
        out[dst[starts]] = np.add.reduceat(vals, starts, axis=0)
    return out


def mfma_k_order(k, step):
    """The k of MFMA step s: `step` consecutive k of the lower half of K, then the same of the upper half (ws_gemm.hip: lane half
    h owns [h K / 2, (h + 1) K / 2)); step = 8 for v_mfma_f32_32x32x16_f16, 1 for v_mfma_f32_32x32x2_f32."""
    half = k // 2
    lo = np.arange(half).reshape(-1, step)
    return np.concatenate([lo, lo + half], 1).reshape(-1)


# ---- in / out ---------------------------------------------------------------------------------------------------------------------------

def norm_ref64(v):
    return T.normalize64(np.asarray(v, np.float64))


def norm_bound(v):
    v = np.asarray(v, np.float64)
    return T.normalize_bound(v, np.zeros_like(v))


norm_emul = T.normalize_emul


# ---- edge -------------------------------------------------------------------------------------------------------------------------------

def edge_ref64(xn, knn, p, mean, dsts=None):
    """DynamicEdgeConv on the rows xn [n, D] over the table knn [n, k] (global rows, -1 = none), float64.  Returns dict(out [n, D]
    (or [len(dsts), D]), and what the bound needs)."""
    xn = np.asarray(xn, np.float64)
    wp, bp, wq, w2, b2 = (np.asarray(p[k], np.float64) for k in ("g_wp", "g_bp", "g_wq", "g_w2", "g_b2"))
    src, dst, slot = edge_rows(knn, dsts=dsts)
    own = np.arange(xn.shape[0]) if dsts is None else np.asarray(dsts)
    n_out = len(own)
    P, Q = xn @ wp + bp, xn @ wq
    pre1 = P[own[dst]] + Q[src]
    h = T.relu64(pre1)
    act2 = T.relu64(h @ w2 + b2)
    cnt = np.bincount(dst, minlength=n_out).astype(np.float64)[:, None]
    if mean:
        out = _segsum(act2, dst, n_out) / np.maximum(cnt, 1.0)
    else:
        out = T.segmax(act2, dst, n_out)
    return dict(out=out, P=P, Q=Q, pre1=pre1, h=h, act2=act2, src=src, dst=dst, own=own, cnt=cnt)


def edge_bound(ref, xn, p, precision, mean):
    x3 = precision == "f16x3"
    xn = np.asarray(xn, F32)
    w2, b2 = np.asarray(p["g_w2"], np.float64), np.asarray(p["g_b2"], np.float64)
    zero = np.zeros_like(np.asarray(p["g_bp"], F32))
    e_p = T.dense_bound(ref["P"], xn, p["g_wp"], p["g_bp"], precision, p["g_wp_scale"] if x3 else 1.0)
    e_q = T.dense_bound(ref["Q"], xn, p["g_wq"], zero, precision, p["g_wq_scale"] if x3 else 1.0)
    src, dst, own = ref["src"], ref["dst"], ref["own"]
    e1 = e_p[own[dst]] + e_q[src]
    e1 = e1 + U * (np.abs(ref["pre1"]) + e1)
    hmag = ref["h"] + e1
    row_ref = dict(act=ref["act2"])
    l2 = G.x3_bound(hmag, w2, 1.0, b2, row_ref) if x3 else G.gemm_bound(hmag, w2, b2, row_ref)
    rows = e1 @ np.abs(w2) + l2
    n_out = len(own)
    if mean:
        total = _segsum(rows, dst, n_out) + gamma(9) * _segsum(ref["act2"] + rows, dst, n_out)
        return total / np.maximum(ref["cnt"], 1.0) + U * np.abs(ref["out"])
    return T.segmax(rows, dst, n_out) + U * np.abs(ref["out"])


def _pq_emul(x, w, b, precision, scale, order, wrong):
    if precision == "f16x3" and wrong == "bias_unscaled":          # the bias added to the scaled accumulator: (acc + b) / s
        ap, ws = T._pad16(np.asarray(x, np.float64), np.asarray(w, np.float64) * scale)
        return T._r32(T._r32(T.x3_single(ap, ws, order) + np.asarray(b, np.float64)) / scale)
    return T.dense_emul(x, w, b, precision, scale, order, wrong if wrong in PLANES else None, relu=False)


def edge_emul(xn, knn, p, precision, mean, order="tile", wrong=None, dsts=None):
    """The documented arithmetic of the P / Q products and the WS_EDGE_KNN stream (module text); out [n, D] or [len(dsts), D]."""
    x3 = precision == "f16x3"
    xn, knn = np.asarray(xn, np.float64), np.asarray(knn)
    n, d = xn.shape
    w2, b2 = np.asarray(p["g_w2"], np.float64), np.asarray(p["g_b2"], np.float64)
    src, dst, slot = edge_rows(knn, wrong, dsts)
    own = np.arange(n) if dsts is None else np.asarray(dsts)
    n_out = len(own)
    need = np.unique(np.concatenate([own, src]))               # P / Q rows this call reads
    pos = np.full(n, -1, np.int64)
    pos[need] = np.arange(len(need))
    P = _pq_emul(xn[need], p["g_wp"], p["g_bp"], precision, p["g_wp_scale"] if x3 else 1.0, order, wrong)
    Q = _pq_emul(xn[need], p["g_wq"], np.zeros(d), precision, p["g_wq_scale"] if x3 else 1.0, order, wrong)
    q_rows = pos[own[dst]] if wrong == "wq_on_i" else pos[src]
    h = T.relu64(T._r32(P[pos[own[dst]]] + Q[q_rows]))
    if x3:
        ko = mfma_k_order(d, 8) if order == "tile" else np.arange(d)
        hk, wk = h[:, ko], w2[ko]
        if wrong == "no_drain_scale":
            ah, al = T.split_f16(hk, False, 2048.0)
            wh, wl = T.split_f16(wk, False, 2048.0)
            acc = T.dot_ordered(ah, wh, order, start=b2)
            aa, ww = T._interleave([(ah, wl * 2048.0), (al * 2048.0, wh)], d, 16)
            y = T._r32(acc + T.dot_ordered(aa, ww, order))
        else:
            y = T.x3_double(hk, wk, b2, order, wrong if wrong in PLANES else None)
    elif order == "tile":                                      # one fma per k in the MFMA step order
        ko = mfma_k_order(d, 1)
        y = T.dot_ordered(h[:, ko], w2[ko], "seq", start=b2, fma=True)
    else:
        y = T.dot_ordered(h, w2, order, start=b2)
    cnt = np.bincount(dst, minlength=n_out).astype(np.float64)[:, None]
    if not mean:
        raw = T.segmax(y, dst, n_out, empty=-np.inf)
        if wrong == "max_from_neg_inf":
            return np.where(np.isfinite(raw), raw, 0.0)
        return np.maximum(raw, 0.0)
    r = y if wrong == "max_from_neg_inf" else T.relu64(y)
    slots = np.zeros((n_out, 8, y.shape[1]))
    slots[dst, slot] = r
    halves = []
    for s0 in (0, 4):                                          # rows 0-3, then rows 4-7, each from 0 in order
        acc = np.zeros((n_out, y.shape[1]))
        for s in range(s0, s0 + 4):
            acc = T._r32(acc + slots[:, s])
        halves.append(acc)
    total = T._r32(halves[0] + halves[1])
    div = np.full_like(cnt, float(knn.shape[1])) if wrong == "mean_over_k" else np.maximum(cnt, 1.0)
    return np.where(cnt > 0, T._r32(total / div), 0.0)


# ---- pool -------------------------------------------------------------------------------------------------------------------------------

def _cell_of(cell_ptr):
    cp = np.asarray(cell_ptr).astype(np.int64)
    return np.repeat(np.arange(len(cp) - 1), np.diff(cp))


def pool_ref64(x, cell_ptr, mean):
    x = np.asarray(x, np.float64)
    cp = np.asarray(cell_ptr).astype(np.int64)
    if mean:
        return np.add.reduceat(x, cp[:-1], axis=0) / np.diff(cp)[:, None]
    return np.maximum.reduceat(x, cp[:-1], axis=0)


def pool_bound(ref, x, cell_ptr, mean):
    if not mean:
        return np.zeros_like(ref)
    cp = np.asarray(cell_ptr).astype(np.int64)
    n = np.diff(cp)[:, None].astype(np.float64)
    return gamma(n) * np.add.reduceat(np.abs(np.asarray(x, np.float64)), cp[:-1], axis=0) / n + U * np.abs(ref)


def pool_emul(x, cell_ptr, mean, wrong=None):
    """k_segpool: fmaxf from -inf, or the sequential fp32 sum from 0 and one division.  wrong: pool_from_zero."""
    x = np.asarray(x, np.float64)
    cp = np.asarray(cell_ptr).astype(np.int64)
    if not mean:
        out = np.maximum.reduceat(x, cp[:-1], axis=0)
        return np.maximum(out, 0.0) if wrong == "pool_from_zero" else out
    sizes = np.diff(cp)
    acc = np.zeros((len(sizes), x.shape[1]))
    for t in range(int(sizes.max())):
        live = sizes > t
        acc[live] = T._r32(acc[live] + x[cp[:-1][live] + t])
    return T._r32(acc / sizes[:, None])


# ---- l1 / l2 ----------------------------------------------------------------------------------------------------------------------------

def lin_ref64(a, w, b):
    """relu(a w + b) in float64 on the inputs as given (fp32 from a trace, float64 inside head_ref64)."""
    return G.gemm_ref64(np.asarray(a), np.asarray(w), np.asarray(b), True)["act"]


def lin_bound(ref, a, w, b):
    return T.dense_bound(ref, a, w, b, "fp32", 1.0)


def lin_emul(a, w, b, order="tile", wrong=None):
    """launch_gemm: an fp32 fma chain in both precisions.  wrong (no_lo_hi | no_hi_lo | trunc_split): the layer handed to the
    f16x3 GEMM instead, with that fault."""
    if wrong in PLANES:
        return T.dense_emul(a, w, b, "f16x3", x3_scale(np.asarray(w)), order, wrong)
    return T.dense_emul(a, w, b, "fp32", 1.0, order)


# ---- the whole head in float64 ----------------------------------------------------------------------------------------------------------

def head_ref64(obj_emb, cell_ptr, knn, p, mean):
    """The stage references chained on obj_emb in float64 (weights as given: float64 folds in the host test)."""
    xn = norm_ref64(obj_emb)
    edge = edge_ref64(xn, knn, p, mean)["out"]
    pool = pool_ref64(edge, cell_ptr, mean)
    l1 = lin_ref64(pool, p["lin_w1"], p["lin_b1"])
    l2 = lin_ref64(l1, p["lin_w2"], p["lin_b2"])
    return dict(head_in=xn, head_edge=edge, head_pool=pool, head_l1=l1, head_l2=l2, out=norm_ref64(l2))


# ---- which branches a call takes --------------------------------------------------------------------------------------------------------

def kernel_dim(d):
    return (d + 127) // 128 * 128


def knn_stage_rows(max_cell, dim):
    """launch_knn: how many rows of a cell are staged in LDS (0 = the global-load loop for every cell of the launch)."""
    lds = ((max(max_cell, 1) * max_cell + 3) & ~3) * 4
    if dim <= 512 and dim % 4 == 0:
        rows = min(max_cell, KNN_STAGE)
        if lds + rows * (dim + 4) * 4 <= 160 * 1024:
            return rows
    return 0


def branches_reached(case, num_cus=G.NUM_CUS):
    """What a case reaches, per chunk of its call.  A HAND restatement of Chunk::cell_head / next_chunk_end (cell_encoder.hip),
    launch_knn (small_kernels.hip) and launch_ws's WS_EDGE_KNN table (ws_gemm.hip): it changes with those launchers.
    case: dict(sizes, d, precision, variation, chunk)."""
    cp = np.concatenate([[0], np.cumsum(case["sizes"])]).astype(np.int64)
    dk = kernel_dim(case["d"])
    out = dict(group=set(), knn=set(), straddle=False, ragged=False, chunks=0, short_cell=bool(min(case["sizes"]) < KNN_K),
               agg="mean" if case["variation"] == 1 else "max",
               build="ws_edge_knn<%d, %s, %s>" % (dk, {256: "256 columns on 8 waves", 128: "128 columns on 4 waves",
                                                       384: "3 slices of 128 columns on 4 waves"}[dk],
                                                  "x3" if case["precision"] == "f16x3" else "fp32"))
    for c0, c1 in chunks(cp, case.get("chunk", 0)):
        n = int(cp[c1] - cp[c0])
        group = 8 if (n + 31) // 32 < num_cus else 32
        sizes = np.diff(cp[c0: c1 + 1])
        stage = knn_stage_rows(int(sizes.max()), dk)
        local = cp[c0: c1 + 1] - cp[c0]
        out["group"].add(group)
        out["knn"].update("staged" if s <= stage else "unstaged" for s in sizes)
        out["straddle"] |= bool(np.any(local[:-1] // group != (local[1:] - 1) // group))
        out["ragged"] |= n % group != 0
        out["chunks"] += 1
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

EMBED_SIZES = (1, 2, 7, 8, 9, 33, 64, 65, 192)     # 381 objects: cells straddle the 8-destination groups, 381 % 8 != 0
EMBED_DIMS = (256, 128, 64, 300)
FULL_SIZES = T.CELL_SIZES


def _ecase(d, precision, variation, sizes=EMBED_SIZES, chunk=0, tag=""):
    name = "emb-%d-%s-%s%s" % (d, "x3" if precision == "f16x3" else "fp32", "mean" if variation else "max", tag)
    return dict(name=name, d=d, precision=precision, variation=variation, sizes=tuple(sizes), chunk=chunk, seed=11)


EMBED_CASES = [_ecase(d, pr, v) for d in EMBED_DIMS for pr in ("f16x3", "fp32") for v in (0, 1)] + [
    # without the 192-object cell the chunk's cells of up to 64 rows are staged in LDS (with it: none is)
    _ecase(300, pr, v, EMBED_SIZES[:-1], tag="-staged") for pr in ("f16x3", "fp32") for v in (0, 1)] + [
    _ecase(256, "f16x3", 0, chunk=100, tag="-chunk100")]
FULL_CASES = [dict(name="full-%s-%s-fill%d" % ("x3" if pr == "f16x3" else "fp32", "mean" if v else "max", seed), d=256, precision=pr,
                   variation=v, sizes=FULL_SIZES, chunk=8, seed=seed)
              for pr, v, seed in (("f16x3", 0, 11), ("fp32", 0, 11), ("f16x3", 1, 11), ("fp32", 1, 11), ("f16x3", 0, 12), ("fp32", 1, 12))]
GROUP32_CASES = [dict(name="group32-x3-max", d=256, precision="f16x3", variation=0, chunk=0, seed=11),
                 dict(name="group32-fp32-mean", d=256, precision="fp32", variation=1, chunk=0, seed=11)]


def group32_sizes(num_cus):
    """Cells of 1 .. 33 objects, 32 num_cus + 40 objects in all: (n + 31) / 32 >= num_cus, so knn_group is 32."""
    n, sizes, s = 32 * num_cus + 40, [], 0
    while sum(sizes) < n:
        sizes.append(min(s % 33 + 1, n - sum(sizes)))
        s += 1
    return tuple(sizes)


def embed_table(case, sizes=None):
    """(table [n_obj, kernel_dim] fp32, class_idx [n_obj] int32, cell_ptr int32): one random table row per object (pad columns 0),
    and in every cell of 3 objects and more two objects that share a row - distance-0 ties, broken by index."""
    sizes = case["sizes"] if sizes is None else sizes
    cp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n, d, dk = int(cp[-1]), case["d"], kernel_dim(case["d"])
    rng = np.random.default_rng([case["seed"], d, n])
    table = np.zeros((n, dk), F32)
    table[:, :d] = rng.standard_normal((n, d)).astype(F32) * F32(0.5)
    idx = np.arange(n, dtype=np.int32)
    for c, s in enumerate(sizes):
        if s >= 3:
            idx[cp[c] + s // 2] = idx[cp[c]]
    return table, idx, cp


def sample_dsts(cell_ptr, group, seed=0, extra=4):
    """The destinations of the first, the last and `extra` seeded groups of `group` destinations."""
    n = int(cell_ptr[-1])
    n_groups = (n + group - 1) // group
    rng = np.random.default_rng(seed)
    picks = sorted({0, n_groups - 1} | set(rng.choice(n_groups, size=min(extra, n_groups), replace=False).tolist()))
    return np.concatenate([np.arange(g * group, min((g + 1) * group, n)) for g in picks])


# ---- the exact family: head_in to head_l2 without a rounding ------------------------------------------------------------------------------
# Driven through the single-feature embedding path (use_features = ["class"], class_embed): obj_emb is the normalised table row.
# Rows: s in {4, 16, 64, 256} (s <= D) non-zeros of +-1 / sqrt(s) = +-1/2 .. +-1/16 - the fp32 sum of squares is exactly 1 in any
# order, sqrt(1) = 1, x / 1 = x: both normalisations return the row bit for bit; every cell of 3 objects and more repeats a row.
# Weight sets (kind), all biases on the grid below, every fourth column of W2 "dead" (negative taps on h >= 0, negative bias: the
# implicit ReLU of the aggregation shows):
#   single   two taps of +-1/2 or +-1/4 per column in Wp, Wq, W2 (+-1/2 in lin), biases in {-1, -1/2, 0, 1/2, 1}: every activation a
#            single fp16 plane up to h (8 bits); hi.hi carries everything.  On max its channel 0 is trunk_ref's probe: bp[0] =
#            EXACT_PROBE with no tap, W2 and lin pass channel 0 on with one tap of 1 - relu(P_i + Q_j)[0] = 1 + 2^-10 - 2^-22 splits
#            exactly to nearest and loses 2^-22 by truncation.  (Not on mean: n copies of a 23-bit value do not sum exactly.)
#   lowbias  single with bp + t 2^-13: relu(P_i + Q_j) has two planes in front of a single-plane W2 (+-1/2 taps): lo.hi.
#   wpq2     ONE tap of +-1 + t 2^-13 per column of Wp and Wq (s w = +-8192 +- 1: hi = +-8192, lo = +-1), one tap of +-1 elsewhere,
#            biases in {-1, 0, 1}: hi.lo of k_gemm_x3 behind the single-plane rows.
#   w22      one tap of +-1 everywhere, W2 = +-1 + t 2^-13 (pack_f16x3: hi = +-1, lo' = +-1/4) behind h on the 2^-4 grid: hi.lo of
#            the edge stream.
# Units and tops per stage: exact_units() (the probe channel apart: it holds EXACT_PROBE itself from h to head_l2).  Mean divides by min(8, n) and by n: cells of 1 .. 64 objects (powers of two) for
# `single`, of 1, 2 and 4 for the sets with a 2^-13 part (a 64-object mean would need 29 bits there).

EXACT_KINDS = ("single", "lowbias", "wpq2", "w22")
EXACT_MAX_SIZES = (1, 2, 7, 8, 9, 33)        # 60 objects: cells straddle the 8-destination groups, 60 % 8 != 0
EXACT_MEAN_SIZES = {"single": (1, 2, 4, 8, 16, 32, 64), "lowbias": (1, 2, 4, 4, 2, 1), "wpq2": (1, 2, 4, 4, 2, 1), "w22": (1, 2, 4, 4, 2, 1)}
EXACT_CASES = [dict(name="exact-%s-%d-%s" % (kind, d, "mean" if v else "max"), kind=kind, d=d, variation=v,
                    sizes=EXACT_MEAN_SIZES[kind] if v else EXACT_MAX_SIZES, chunk=0)
               for kind in EXACT_KINDS for d in (256, 128) for v in (0, 1)]


def exact_rows(case):
    """(table [R, D] fp32, class_idx [n_obj] int32, cell_ptr int32) of an exact case."""
    sizes, d = case["sizes"], case["d"]
    cp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(cp[-1])
    rng = np.random.default_rng([3, d, n])
    table = np.zeros((n, d), F32)
    for r in range(n):
        s = int(rng.choice([v for v in (4, 16, 64, 256) if v <= d]))
        cols = rng.choice(d, s, replace=False)
        table[r, cols] = (rng.choice([-1.0, 1.0], s) / np.sqrt(s)).astype(F32)
    idx = np.arange(n, dtype=np.int32)
    for c, s in enumerate(sizes):
        if s >= 3:
            idx[cp[c] + s // 2] = idx[cp[c]]
            idx[cp[c + 1] - 1] = idx[cp[c] + 1]
    return table, idx, cp


def exact_weights(case, seed=5):
    """The head's folded matrices of an exact case (module text), k-major fp32."""
    kind, d, mean = case["kind"], case["d"], case["variation"] == 1
    rng = np.random.default_rng([seed, d, EXACT_KINDS.index(kind)])
    one_tap = kind in ("wpq2", "w22")
    grid = [-1.0, 0.0, 1.0] if one_tap else [-1.0, -0.5, 0.0, 0.5, 1.0]

    def layer(vals, planes=False, dead=False, bias=True):
        w = np.zeros((d, d), np.float64)
        b = rng.choice(grid, d) if bias else np.zeros(d)
        for col in range(d):
            if one_tap:
                w[rng.integers(0, d), col] = rng.choice([-1.0, 1.0]) + (rng.choice([-1.0, 1.0]) * 2.0 ** -13 if planes else 0.0)
            else:
                w[rng.choice(d, 2, replace=False), col] = rng.choice(vals, 2)
            if dead and col % 4 == 3:
                w[:, col] = -np.abs(w[:, col])
                b[col] = -1.0 if one_tap else -0.5
        return w, b
    half, quarter = [-0.5, 0.5], [-0.5, -0.25, 0.25, 0.5]
    wp, bp = layer(quarter, planes=kind == "wpq2")
    wq, _ = layer(quarter, planes=kind == "wpq2", bias=False)
    w2, b2 = layer(half if kind == "lowbias" else quarter, planes=kind == "w22", dead=True)
    l1w, l1b = layer(half)
    l2w, l2b = layer(half)
    if kind == "lowbias":
        bp = bp + rng.choice([-1.0, 1.0], d) * 2.0 ** -13
    if kind == "single" and not mean:                   # the probe channel
        wp[:, 0], wq[:, 0], bp[0] = 0.0, 0.0, T.EXACT_PROBE
        for w, b in ((w2, b2), (l1w, l1b), (l2w, l2b)):
            w[0, :], w[:, 0] = 0.0, 0.0
            w[0, 0], b[0] = 1.0, 0.0
    f = lambda a: np.ascontiguousarray(a, F32)
    p = dict(g_wp=f(wp), g_bp=f(bp), g_wq=f(wq), g_w2=f(w2), g_b2=f(b2), lin_w1=f(l1w), lin_b1=f(l1b), lin_w2=f(l2w), lin_b2=f(l2b))
    for k, v in (("g_wp", wp), ("g_bp", bp), ("g_wq", wq), ("g_w2", w2)):
        assert np.array_equal(p[k].astype(np.float64), v), "the designed values are fp32 numbers"
    return head_pack(p)


def exact_units(case):
    """stage -> (unit, top): every value of the stage (and, for a sum, every partial sum - checked on the sum of magnitudes) is a
    multiple of `unit` below `top`, with top / unit <= 2^24: exact in fp32 in any order, with or without fma."""
    kind, mean = case["kind"], case["variation"] == 1
    big = max(case["sizes"])
    u_pq = {"single": 2.0 ** -6, "lowbias": 2.0 ** -13, "wpq2": 2.0 ** -17, "w22": 2.0 ** -4}[kind]   # rows on the 2^-4 grid
    u_rows = u_pq * {"single": 2.0 ** -2, "lowbias": 2.0 ** -1, "wpq2": 1.0, "w22": 2.0 ** -13}[kind]
    u_edge = u_rows / (min(8, big) if mean else 1)
    u_pool = u_edge / (big if mean else 1)
    lt = 1.0 if kind in ("wpq2", "w22") else 0.5
    return dict(pq=(u_pq, 2.0), h=(u_pq, 4.0), rows=(u_rows, 4.0), edge_sum=(u_rows, 32.0), edge=(u_edge, 4.0),
                pool_sum=(u_edge, 4.0 * big), pool=(u_pool, 4.0), l1=(u_pool * lt, 8.0), l2=(u_pool * lt * lt, 8.0))


def exact_headroom(case, table_rows, knn, cell_ptr, p):
    """The premises of exactness on the data: no value and no sum of magnitudes leaves its (unit, top) of exact_units, and every
    top / unit fits fp32's 24 bits.  Returns the float64 stage references (head_ref64) when they hold, else None."""
    units = exact_units(case)
    mean = case["variation"] == 1
    probe = case["kind"] == "single" and not mean           # channel 0 holds EXACT_PROBE at every stage: checked as such
    cut = (lambda v: v[:, 1:]) if probe else (lambda v: v)
    ok = lambda x, key: units[key][1] / units[key][0] <= 2.0 ** 24 and T.exact_headroom(x, *units[key])
    x = np.asarray(table_rows, np.float64)
    if not (np.array_equal((x.astype(F32) ** 2).sum(1, dtype=F32), np.ones(len(x), F32)) and ok(x, "pq")):
        return None
    a = lambda k: np.abs(np.asarray(p[k], np.float64))
    ref = head_ref64(table_rows, cell_ptr, knn, p, mean)
    e = edge_ref64(ref["head_in"], knn, p, mean)
    sums = [(np.abs(x) @ a("g_wp") + a("g_bp"), "pq"), (np.abs(x) @ a("g_wq"), "pq"), (e["pre1"], "h"),
            (e["h"] @ a("g_w2") + a("g_b2"), "rows"), (ref["head_edge"], "edge"),
            (ref["head_pool"], "pool"), (ref["head_pool"] @ a("lin_w1") + a("lin_b1"), "l1"),
            (ref["head_l1"] @ a("lin_w2") + a("lin_b2"), "l2")]
    if mean:                                                   # the sums in front of the two divisions
        sums += [(_segsum(e["act2"], e["dst"], len(x)), "edge_sum"),
                 (np.add.reduceat(ref["head_edge"], np.asarray(cell_ptr[:-1], np.int64), axis=0), "pool_sum")]
    if probe and not all(np.all(ref[k][:, 0] == T.EXACT_PROBE) for k in ("head_edge", "head_pool", "head_l1", "head_l2")):
        return None
    return ref if all(ok(cut(v), key) for v, key in sums) else None
