"""The kNN-graph side of the cell gates (test infrastructure; a plain module, imported by the GPU tests and fuzz_cells.py).

The cell path is continuous up to the object embeddings and then takes one DISCRETE step: DynamicEdgeConv's kNN graph
(models/cell_retrieval.py:46-48).  Two evaluations whose object embeddings differ by 1e-5 can pick another 8th neighbour where
the 8th and 9th distances nearly tie, and the cell's embedding then moves by up to ~5e-2.  Such a cell is not excused here: it
is checked against the float64 oracle's cell head evaluated on the graph the kernel chose (check_cells), and that graph itself
must be a kNN graph of the kernel's own embeddings (knn_violation) whose every difference from the oracle's is a near-tie
(knn_flips).

Neighbour tables are [n_obj, k] global object rows padded with -1 (t2p_cell_trace.knn_idx after global_knn).
"""
import copy
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

TOL = 1e-4                # cell embeddings against the oracle; distance gap of a near-tie (knn_flips)
U = 2.0 ** -24            # fp32 unit roundoff
# Rounding bound of a squared distance as the kernel forms it (k_knn, like the oracle's primitives.c): the sequential fp32 sum
# acc = acc + (a - b)^2 over the 256 coordinates of two fp32-normalised rows.  Per distance d: 255 u d for the sum of 256
# non-negative terms (first order), 3 u d for each term's difference and square, 14 u d for the two rows' fp32 normalisation
# (k_rownorm: a 256-term sum of squares, sqrt, divide - a row scale within 1 +- 7 u each), 16 u d headroom for second-order
# terms: 288 u d in all; plus 8 u absolute per distance for the per-coordinate rounding of the normalised rows
# (2 u sum_t |a_t - b_t| (|a_t| + |b_t|) <= 4 u |a - b| <= 8 u).
KNN_REL = 288 * U         # ~1.7e-5 per unit of squared distance
KNN_ABS = 16 * U          # ~9.5e-7 for a pair of distances


def global_knn(knn, cell_ptr, chunk_objects=0):
    """t2p_cell_trace.knn_idx rows are local to the library's internal chunk (whole cells, at most `chunk_objects` objects -
    the call's; 0 = the library's default; a single larger cell forms its own chunk): add each object's chunk start, keep -1."""
    if chunk_objects <= 0:
        from text2pos_amd.ops import DEFAULT_CHUNK_OBJECTS
        chunk_objects = DEFAULT_CHUNK_OBJECTS
    knn = np.asarray(knn).astype(np.int64)
    chunk0 = np.zeros(knn.shape[0], dtype=np.int64)
    lo = 0
    for c in range(len(cell_ptr) - 1):
        if cell_ptr[c + 1] - lo > chunk_objects:
            lo = cell_ptr[c]
        chunk0[cell_ptr[c]: cell_ptr[c + 1]] = lo
    return np.where(knn >= 0, knn + chunk0[:, None], -1)


def oracle_knn(emb, cell_ptr, k=8):
    """The oracle's own neighbour table (global rows) for fp32 object embeddings `emb` (un-normalised, as traced): primitives.c's
    kNN on F.normalize(emb) in fp32, exactly as DynamicEdgeConv builds it inside OracleCellRetrieval.encode_objects_packed."""
    from oracle import lib
    embn = np.ascontiguousarray(F.normalize(torch.as_tensor(np.asarray(emb)).float(), dim=-1).numpy())
    ptr = np.ascontiguousarray(cell_ptr, dtype=np.int32)
    out = np.zeros((embn.shape[0], k), np.int32)
    fp = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    lib().t2p_oracle_knn(fp(embn, C.c_float), fp(ptr, C.c_int32), C.c_int32(len(ptr) - 1), C.c_int32(embn.shape[1]),
                         C.c_int32(k), fp(out, C.c_int32))
    return out.astype(np.int64)


def normalized64(emb):
    """F.normalize in float64 of [n, D] object embeddings (tensor or array): the coordinates the checks measure distances in."""
    if isinstance(emb, torch.Tensor):
        emb = emb.detach().cpu()
    return F.normalize(torch.as_tensor(np.asarray(emb)).double(), dim=-1).numpy()


def knn_flips(knn_a, knn_b, embn64, cell_ptr):
    """Objects whose DynamicEdgeConv neighbour lists differ between two runs, and the evidence that every such difference
    is a near-tie: the squared distances (float64, from one run's normalised object embeddings) of the neighbours that
    appear in only one of the two lists differ by less than TOL.  Returns (cells containing such an object, worst gap)."""
    knn_a, knn_b = np.asarray(knn_a), np.asarray(knn_b)
    diff = np.flatnonzero((knn_a != knn_b).any(axis=1))
    cell_of = np.repeat(np.arange(len(cell_ptr) - 1), np.diff(cell_ptr))
    worst = 0.0
    for i in diff:
        only = sorted((set(knn_a[i].tolist()) ^ set(knn_b[i].tolist())) - {-1})
        if not only:      # same set, different order: distances tied to the last bit
            continue
        d2 = ((embn64[only] - embn64[i]) ** 2).sum(axis=1)
        worst = max(worst, float(d2.max() - d2.min()))
    return np.unique(cell_of[diff]), worst


def knn_violation(knn, embn64, cell_ptr, k=8):
    """Is `knn` a kNN graph of the normalised object embeddings `embn64` (float64; the KERNEL's own)?  Structure, asserted:
    every object of an n-object cell lists min(k, n) distinct objects of its own cell, then -1 only.  Distances: no chosen
    neighbour c may be farther than an unchosen object u of the cell beyond fp32 rounding (module header),
        d(c) - d(u) <= KNN_REL (d(c) + d(u)) + KNN_ABS          (squared distances; KNN_REL ~ 1.7e-5, KNN_ABS ~ 9.5e-7).
    Returns the worst d(c) - d(u) - KNN_REL (d(c) + d(u)) - KNN_ABS over all objects: <= 0 for a kNN graph (-inf when no cell
    holds more than k objects).  Vectorised per cell size."""
    knn = np.asarray(knn).astype(np.int64)
    embn64 = np.asarray(embn64, dtype=np.float64)
    cell_ptr = np.asarray(cell_ptr).astype(np.int64)
    sizes = np.diff(cell_ptr)
    assert knn.shape == (int(cell_ptr[-1]), k), (knn.shape, int(cell_ptr[-1]), k)
    worst = -np.inf
    for n in np.unique(sizes[sizes > 0]).tolist():
        cells = np.flatnonzero(sizes == n)
        lo = cell_ptr[cells]
        rows = lo[:, None] + np.arange(n)[None, :]                          # [m, n] object rows
        lst = knn[rows]                                                     # [m, n, k]
        kk = min(k, n)
        assert (lst[..., kk:] == -1).all(), f"{n}-object cells: a neighbour list goes on past {kk} entries"
        loc = lst[..., :kk] - lo[:, None, None]
        bad = ~((lst[..., :kk] >= 0) & (loc >= 0) & (loc < n)).all(axis=(1, 2))
        assert not bad.any(), f"cell {int(cells[bad][0])} ({n} objects): a neighbour missing or outside the cell"
        srt = np.sort(loc, axis=-1)
        rep = (srt[..., 1:] == srt[..., :-1]).any(axis=(1, 2))
        assert not rep.any(), f"cell {int(cells[rep][0])} ({n} objects): a neighbour listed twice"
        if kk == n:                                                         # every object of the cell is chosen
            continue
        e = embn64[rows]                                                    # [m, n, D]
        sq = (e * e).sum(-1)
        d2 = np.maximum(sq[:, :, None] + sq[:, None, :] - 2.0 * np.matmul(e, e.transpose(0, 2, 1)), 0.0)
        chosen = np.zeros(d2.shape, dtype=bool)
        np.put_along_axis(chosen, loc, True, axis=-1)
        far = np.where(chosen, d2, -np.inf).max(-1)
        near = np.where(chosen, np.inf, d2).min(-1)
        worst = max(worst, float((far - near - KNN_REL * (far + near) - KNN_ABS).max()))
    return worst


def float64_oracle(om):
    """A float64 copy of an oracle model: its cell_head then runs in float64 throughout."""
    return copy.deepcopy(om).double().eval()


def cell_head64(oracle64, emb, cell_ptr, knn=None):
    """oracle64.cell_head on fp32 object embeddings, as a float64 array (no autograd graph: 12,000 cells would not fit)."""
    if isinstance(emb, torch.Tensor):
        emb = emb.detach().cpu()
    with torch.no_grad():
        return oracle64.cell_head(torch.as_tensor(np.asarray(emb)), cell_ptr, knn=knn).numpy()


def check_cells(got, got_knn, want, want_knn, want_emb, cell_ptr, oracle64, tag):
    """The cell gate.  got / got_knn: a kernel's cell embeddings and neighbour table (global rows); want / want_knn / want_emb:
    the oracle's cell embeddings, neighbour table and (un-normalised) object embeddings; oracle64: float64_oracle(model).
      * cells whose objects' lists all agree with the oracle's as sets: |got - want| < TOL;
      * every list difference a proven near-tie (knn_flips: float64 distance gap < TOL);
      * cells with such a difference: |got - oracle64.cell_head(want_emb, knn=got_knn)| < TOL - the oracle's head, in float64,
        on the graph the kernel chose.
    Returns (flipped cells, worst difference of a flipped cell from that resolved reference, worst near-tie gap)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    got_knn, want_knn = np.asarray(got_knn).astype(np.int64), np.asarray(want_knn).astype(np.int64)
    want_emb = np.asarray(want_emb)
    cell_ptr = np.asarray(cell_ptr).astype(np.int64)
    n_cells = len(cell_ptr) - 1
    assert got.shape == want.shape and got.shape[0] == n_cells, (tag, got.shape, want.shape, n_cells)
    assert got_knn.shape == want_knn.shape and got_knn.shape[0] == int(cell_ptr[-1]), (tag, got_knn.shape, want_knn.shape)
    cell_of = np.repeat(np.arange(n_cells), np.diff(cell_ptr))
    inside = (got_knn < 0) | (cell_of[np.maximum(got_knn, 0)] == cell_of[:, None])
    assert inside.all(), f"{tag}: object {int(np.flatnonzero(~inside.all(1))[0])} has a neighbour outside its cell"
    differ = (np.sort(got_knn, axis=1) != np.sort(want_knn, axis=1)).any(axis=1)
    flipped = np.unique(cell_of[differ])
    _, gap = knn_flips(got_knn, want_knn, normalized64(want_emb), cell_ptr)
    assert gap < TOL, f"{tag}: a neighbour-list difference that is not a near-tie (distance gap {gap:.2e})"
    d = np.abs(got - want).max(axis=1)
    same = np.ones(n_cells, dtype=bool)
    same[flipped] = False
    bad = np.flatnonzero(same & ~(d < TOL))
    assert len(bad) == 0, f"{tag}: cells {bad[:8].tolist()} (on the oracle's kNN graph) differ by {d[bad].max():.2e}"
    resolved = 0.0
    if len(flipped):
        idx = np.concatenate([np.arange(cell_ptr[c], cell_ptr[c + 1]) for c in flipped])
        ptr = np.concatenate([[0], np.cumsum(np.diff(cell_ptr)[flipped])])
        pos = np.full(int(cell_ptr[-1]), -1, dtype=np.int64)
        pos[idx] = np.arange(len(idx))
        sub = np.where(got_knn[idx] >= 0, pos[np.maximum(got_knn[idx], 0)], -1)
        r = np.abs(got[flipped] - cell_head64(oracle64, want_emb[idx], ptr, knn=sub)).max(axis=1)
        assert (r < TOL).all(), (f"{tag}: cells {flipped[~(r < TOL)][:8].tolist()} differ by {r.max():.2e} from the float64 "
                                 f"oracle evaluated on the kNN graph the kernel chose")
        resolved = float(r.max())
    return flipped, resolved, gap
