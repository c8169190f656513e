"""The float64 statement of the distinct-candidates selection (include/t2p_select.h), in NumPy: what every test of
t2p_topk_distinct and of its callers is held to.  Proved on its own in tests/test_distinct_ref_host.py.

Two cells a, b conflict iff fabs(xa - xb) < sep and fabs(ya - yb) < sep (float64 centres, one subtraction each) and, with a group
table, group[a] == group[b].  A query's allowed cells (score above -inf) are walked by (score descending, index ascending); a cell
is accepted iff it conflicts with no cell accepted before it; the walk stops at k accepted."""
import numpy as np


def conflict(cell_xy, cell_group, sep, a, b) -> bool:
    """The conflict relation of rows a, b: comparisons only, so a NaN never conflicts."""
    xy = np.asarray(cell_xy, dtype=np.float64)
    near = bool(np.abs(xy[a, 0] - xy[b, 0]) < sep) and bool(np.abs(xy[a, 1] - xy[b, 1]) < sep)
    return near and (cell_group is None or int(cell_group[a]) == int(cell_group[b]))


def _walk(rows, cell_xy, cell_group, sep, k):
    """Greedy walk over `rows` (already ordered) -> (accepted rows, their positions in `rows`).  A cell is accepted iff no cell
    accepted before it conflicts with it: each accepted cell strikes the cells it conflicts with (the relation is symmetric, and
    striking a cell already passed changes nothing), one vector comparison per accepted cell."""
    rows = np.asarray(rows, dtype=np.int64)
    xy = np.asarray(cell_xy, dtype=np.float64)
    x, y = xy[rows, 0], xy[rows, 1]
    g = np.zeros(len(rows), dtype=np.int64) if cell_group is None else np.asarray(cell_group)[rows].astype(np.int64)
    open_ = np.ones(len(rows), dtype=bool)
    acc, at, pos = [], [], 0
    while len(acc) < k:
        nxt = np.flatnonzero(open_[pos:])
        if not len(nxt):
            break
        p = pos + int(nxt[0])
        acc.append(int(rows[p]))
        at.append(p)
        with np.errstate(invalid="ignore"):                  # (inf - inf: a NaN, which conflicts with nothing)
            hit = (np.abs(x - x[p]) < sep) & (np.abs(y - y[p]) < sep) & (g == g[p])
        open_ &= ~hit
        pos = p + 1
    return acc, at


def select_ref(pool_idx, pool_score, cell_xy, cell_group, sep, k, n_cells, index_offset=0):
    """What t2p_topk_distinct does on a pool: pool_idx int64 / pool_score float64 [nq, pool] in the order of t2p_sim_topk*.
    -> (idx int64 [nq, k], score float64 [nq, k], n_valid int32 [nq], exhausted int32 [nq]).
    The walk ends at the pool's first -inf entry.  Unfilled columns: the first pool entry's index, -inf.  exhausted = 1 iff fewer
    than k were accepted, the pool held no -inf entry and pool < n_cells.  A query with an entry above -inf whose index lies
    outside [index_offset, index_offset + n_cells): n_valid -1, exhausted 0, every column -1 / -inf."""
    pool_idx, pool_score = np.asarray(pool_idx, dtype=np.int64), np.asarray(pool_score, dtype=np.float64)
    nq, pool = pool_idx.shape
    assert 1 <= k <= pool and pool_score.shape == (nq, pool) and sep >= 0
    idx = np.empty((nq, k), dtype=np.int64)
    score = np.full((nq, k), -np.inf, dtype=np.float64)
    n_valid, exhausted = np.zeros(nq, dtype=np.int32), np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        rows = pool_idx[q] - index_offset
        live = ~(pool_score[q] == -np.inf)
        if np.any(live & ((rows < 0) | (rows >= n_cells))):
            idx[q], n_valid[q] = -1, -1
            continue
        stop = int(np.argmin(live)) if not live.all() else pool            # the first -inf entry
        acc, at = _walk(rows[:stop], cell_xy, cell_group, sep, k)
        n = len(acc)
        idx[q, :n], score[q, :n] = pool_idx[q, at], pool_score[q, at]
        idx[q, n:] = pool_idx[q, 0]
        n_valid[q] = n
        exhausted[q] = int(n < k and live.all() and pool < n_cells)
    return idx, score, n_valid, exhausted


def full_ref(scores, cell_xy, cell_group, sep, k):
    """The definition on the full ranking: scores float64 [Nq, Nc] (-inf: the cell is not allowed for the query).
    -> (idx int64 [Nq, k] (-1 behind the accepted cells), n_valid int32 [Nq], depth int64 [Nq]).
    depth: how many ranked cells a pool must hold to give this result - the 1-based rank of the k-th accepted cell, or, when the
    query has fewer than k distinct cells, the number of its allowed cells plus one (the pool must show the list's end)."""
    scores = np.asarray(scores, dtype=np.float64)
    nq, nc = scores.shape
    idx = np.full((nq, k), -1, dtype=np.int64)
    n_valid, depth = np.zeros(nq, dtype=np.int32), np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        order = np.lexsort((np.arange(nc), -scores[q]))                    # score descending, ties (and +-0.0) to the lower index
        order = order[scores[q, order] > -np.inf]
        acc, at = _walk(order, cell_xy, cell_group, sep, k)
        idx[q, :len(acc)] = acc
        n_valid[q] = len(acc)
        depth[q] = at[-1] + 1 if len(acc) == k else len(order) + 1
    return idx, n_valid, depth
