"""The NumPy float64 yardstick of the restricted retrieval tests (t2p_sim_topk_grouped, include/t2p.h; t2p_sim_topk_prior,
include/t2p_serve.h), their shared input generators and the helpers of the GPU cases; no GPU at import, no package.

    geo(q, c) = dx = max(x0[c] - px[q], px[q] - x1[c], 0), dy likewise: dx * dx + dy * dy <= r[q] * r[q]
    grp(q, c) = query_group[q] < 0 or cell_group[c] == query_group[q]          (the prior call: a negative id is "any group")
    same(q, c) = cell_group[c] == query_group[q]                               (the grouped call: strict, whatever the sign)
    s'(q, c)  = allowed ? C64[c] @ q64[q] : -inf,  then a stable descending argsort

np.maximum keeps NaN, and a comparison with NaN is False: a NaN in px, py, r or a box member masks the pair; so does r < 0.
The geometry is integer-valued, so every distance and every r * r is exact and the pairs on the boundary are exact equalities
(tests/test_topk_ref_host.py proves the masks on hand cases and counts them).  The scores are computed per query on one BLAS thread,
once per shape, and left unchanged."""
import functools
from math import isqrt

import numpy as np

LISTS, TILE = {"sim_partial", "topk_merge"}, {"sim_scores", "topk_select"}      # the kernels of the two routes (ops.profile_report)
RADII = (0.0, 5.0, 25.0, 60.0, np.inf)
# (nq, nc, dim, k): the shapes the GPU cases run
SHAPES = [(130, 1000, 256, 100), (260, 1000, 256, 16), (257, 4099, 128, 100), (37, 2500, 384, 16), (17, 12000, 256, 1024),
          (2700, 12000, 128, 17)]


def allowed(xy, radius, box, query_group=None, cell_group=None):
    """bool [nq, nc].  xy [nq, 2], radius [nq], box [nc, 4] = x0 y0 x1 y1 (or all three None: no geometry); groups int [nq] / [nc]
    (or both None)."""
    ok = None
    if box is not None:
        xy, radius, box = (np.asarray(a, dtype=np.float64) for a in (xy, radius, box))
        px, py, r = xy[:, 0, None], xy[:, 1, None], radius[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            dx = np.maximum(np.maximum(box[None, :, 0] - px, px - box[None, :, 2]), 0.0)
            dy = np.maximum(np.maximum(box[None, :, 1] - py, py - box[None, :, 3]), 0.0)
            ok = ((dx * dx + dy * dy) <= r * r) & (r >= 0)
    if cell_group is not None:
        qg, cg = np.asarray(query_group)[:, None], np.asarray(cell_group)[None, :]
        grp = (qg < 0) | (cg == qg)
        ok = grp if ok is None else ok & grp
    assert ok is not None, "neither geometry nor groups"
    return ok


def same_group(query_group, cell_group):
    """bool [nq, nc]: the grouped call's mask - the ids are equal, negative ones included."""
    return np.asarray(query_group)[:, None] == np.asarray(cell_group)[None, :]


@functools.lru_cache(maxsize=None)
def inputs(nq, nc, dim=256):
    """Unit rows in fp32 from default_rng(nq * 31 + nc), rows 7 and 39 copies of row 3 (read-only)."""
    rng = np.random.default_rng(nq * 31 + nc)
    c = rng.standard_normal((nc, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if nc > 40:
        c[7] = c[3]; c[39] = c[3]
    c.setflags(write=False)
    q.setflags(write=False)
    return c, q


@functools.lru_cache(maxsize=None)
def geometry(nq, nc):
    """(xy float64 [nq, 2], radius float64 [nq], box float64 [nc, 4]), all integer-valued (read-only).  30 m cells at stride 10 on a
    W-wide grid; priors uniform over the grid's extent, radii drawn from RADII; queries 0..3 fixed: nothing in reach, r = 0 inside
    nine cells, r = 5 near a corner, r = inf."""
    w = isqrt(nc - 1) + 1
    i = np.arange(nc)
    x0, y0 = 10.0 * (i % w), 10.0 * (i // w)
    box = np.stack([x0, y0, x0 + 30.0, y0 + 30.0], axis=1)
    rng = np.random.default_rng(7000 + nq + nc)
    xy = rng.integers(0, 10 * w + 21, (nq, 2)).astype(np.float64)
    radius = rng.choice(np.array(RADII), nq)
    xy[0], radius[0] = (-1000.0, -1000.0), 60.0
    xy[1], radius[1] = (45.0, 45.0), 0.0
    xy[2], radius[2] = (35.0, 34.0), 5.0
    radius[3] = np.inf
    for a in (xy, radius, box):
        a.setflags(write=False)
    return xy, radius, box


@functools.lru_cache(maxsize=None)
def strict_groups(nq, nc, n_groups):
    """(cell groups, query groups) int32, read-only.  Cell groups uniform over the ids 0 .. G-3, then exactly 5 cells moved to id
    G-2; id G-1 has no cell.  Query 0 is given the empty group, query 1 the 5-cell group, the others are uniform over 0 .. G-3."""
    rng = np.random.default_rng(1000 * n_groups + nq + nc)
    cg = rng.integers(0, n_groups - 2, nc).astype(np.int32)
    cg[rng.choice(nc, 5, replace=False)] = n_groups - 2
    qg = rng.integers(0, n_groups - 2, nq).astype(np.int32)
    qg[0], qg[1] = n_groups - 1, n_groups - 2
    assert (cg == n_groups - 2).sum() == 5 and not (cg == n_groups - 1).any()
    cg.setflags(write=False)
    qg.setflags(write=False)
    return cg, qg


@functools.lru_cache(maxsize=None)
def groups(nq, nc, n_groups):
    """strict_groups, then every fifth query's group set to -1 (any group)."""
    cg, qg = strict_groups(nq, nc, n_groups)
    qg = qg.copy()
    qg[::5] = -1
    qg.setflags(write=False)
    return cg, qg


def scores(c, q):
    """float64 [nq, nc]: per query C64 @ q64 on one BLAS thread."""
    from threadpoolctl import threadpool_limits
    c64, q64 = np.asarray(c, dtype=np.float64), np.asarray(q, dtype=np.float64)
    s = np.empty((q64.shape[0], c64.shape[0]), dtype=np.float64)
    with threadpool_limits(limits=1, user_api="blas"):
        for i in range(q64.shape[0]):
            s[i] = c64 @ q64[i]
    return s


def masked(s, ok):
    out = np.array(s, dtype=np.float64)
    out[~ok] = -np.inf            # a select: whatever the product was, NaN included
    return out


@functools.lru_cache(maxsize=None)
def masked_scores(nq, nc, dim, n_groups=0):
    """The yardstick's masked score rows of inputs / geometry (/ groups when n_groups > 0), once per shape (read-only)."""
    c, q = inputs(nq, nc, dim)
    xy, radius, box = geometry(nq, nc)
    cg, qg = groups(nq, nc, n_groups) if n_groups else (None, None)
    s = masked(scores(c, q), allowed(xy, radius, box, qg, cg))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def grouped_scores(nq, nc, dim, n_groups):
    """The grouped call's yardstick: the score rows of inputs, masked by same_group of strict_groups, once per shape (read-only)."""
    s = masked(scores(*inputs(nq, nc, dim)), same_group(*strict_groups(nq, nc, n_groups)[::-1]))
    s.setflags(write=False)
    return s


def topk(s, k):
    order = np.argsort(-1.0 * s, axis=1, kind="stable")[:, :k]
    return order, np.take_along_axis(s, order, 1)


def min_gap(s, k):
    """Smallest non-zero finite gap inside the yardstick's top k + 1 (nan without one)."""
    _, w = topk(s, min(k + 1, s.shape[1]))
    fin = np.isfinite(w[:, :-1]) & np.isfinite(w[:, 1:])
    with np.errstate(invalid="ignore"):
        gaps = (w[:, :-1] - w[:, 1:])[fin]
    assert (gaps >= 0).all()
    nz = gaps[gaps != 0]
    return float(nz.min()) if nz.size else float("nan")


def check(s, k, idx, score, index_offset=0, rows=None):
    """The yardstick's finite gaps inside the top k + 1 are 0 or above 1e-10; indices equal; finite scores within 1e-12; masked
    entries exactly -inf, in ascending index, behind every finite score; beyond nc cells -1 / -inf.
    rows: compare only these queries (idx / score hold all of them)."""
    if rows is not None:
        s, idx, score = s[rows], idx[rows], score[rows]
    nq, nc = s.shape
    kk = min(k, nc)
    gap = min_gap(s, k)
    assert not gap <= 1e-10, "the generator produced a near-tie inside the top k + 1"
    widx, wscore = topk(s, kk)
    finite = np.isfinite(wscore)
    err = np.abs(score[:, :kk][finite] - wscore[finite]).max() if finite.any() else 0.0
    print(f"nq={nq} nc={nc} k={k}: min non-zero finite gap {gap:.2e}, max|score - yardstick| {err:.2e}, {int((~finite).sum())} masked entries")
    assert idx.shape == (nq, k) and score.shape == (nq, k)
    assert np.array_equal(idx[:, :kk], widx + index_offset)
    assert err < 1e-12
    assert np.array_equal(np.isneginf(score[:, :kk]), ~finite)
    for r in np.flatnonzero((~finite).any(axis=1)):
        m = idx[r, :kk][~finite[r]]
        assert (np.diff(m) > 0).all()
        assert finite[r, : kk - len(m)].all()
    if nc < k:
        assert (idx[:, nc:] == -1).all() and np.isneginf(score[:, nc:]).all()


# ---- helpers of the GPU cases (torch and the package are imported where they are used) ----------------------------------
def dev():
    import torch
    return torch.device("cuda:0")


def profiled(fn):
    """(fn(), the kernels it launched: name -> (launches, ms))"""
    import torch
    from text2pos_amd import ops
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        out = fn()
    finally:
        ops.profile_enable(False)
    return out, ops.profile_report()
