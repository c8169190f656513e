"""t2p_sim_topk_prior (csrc/sim_topk.hip, MASK_PRIOR instantiations; include/t2p_serve.h) against the NumPy float64 yardstick
tests/topk_ref.py (proved on hand cases by tests/test_topk_ref_host.py): indices equal, finite scores within 1e-12 (the project's
bar for float64 scores), masked entries exactly -inf in ascending index behind every finite score.  Every case first asserts that
the yardstick's finite gaps inside the top k + 1 are 0 or above 1e-10, so a last-bit difference between the kernel's fma chain and
BLAS can reorder only exact duplicates.  Then: bit identity with the unrestricted and the grouped call where the prior allows
everything, the route, NaN on both routes, reads past the end, embed_dim 300 and the wrappers' refusals."""
import numpy as np
import pytest
import torch

import topk_ref as P
from topk_ref import LISTS, TILE, dev as _dev, profiled as _profiled

pytestmark = pytest.mark.gpu


def _up(a):
    return torch.tensor(np.asarray(a), device=_dev())           # (the cached inputs are read-only: torch.tensor copies)


def _topk(c, q, k, xy, radius, box, cg=None, qg=None, **kw):
    import text2pos_amd as t2p
    c, q = (_up(a) if isinstance(a, np.ndarray) else a for a in (c, q))
    groups = {} if cg is None else dict(cell_groups=np.array(cg), query_groups=np.array(qg))
    idx, score = t2p.retrieve_topk(c, q, k, cell_boxes=np.array(box), query_xy=np.array(xy), query_radius=np.array(radius), **groups, **kw)
    return idx.cpu().numpy(), score.cpu().numpy()


# ---- 1. against the yardstick -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nc,dim,k", [(130, 1000, 256, 1), (130, 1000, 256, 10), (130, 1000, 256, 16),       # the register lists
                                         (130, 1000, 256, 17), (130, 1000, 256, 100),                              # the score tile
                                         (260, 1000, 256, 16),                                                     # the score tile at k <= 16
                                         (257, 4099, 128, 100), (37, 2500, 384, 16), (17, 12000, 256, 1024)])
def test_prior_vs_yardstick(nq, nc, dim, k):
    c, q = P.inputs(nq, nc, dim)
    xy, radius, box = P.geometry(nq, nc)
    idx, score = _topk(c, q, k, xy, radius, box)
    s = P.masked_scores(nq, nc, dim)
    P.check(s, k, idx, score)
    n = np.isfinite(s).sum(axis=1)
    assert n[:4].tolist() == [0, 9, 18, nc]
    # query 0: nothing in reach - masked cells only, 0 .. k-1; query 1: its nine cells first, then masked cells in index order
    assert idx[0].tolist() == list(range(k)) and np.isneginf(score[0]).all()
    nine = np.flatnonzero(np.isfinite(s[1])).tolist()
    assert sorted(idx[1, :min(k, 9)].tolist()) == nine[:9] if k >= 9 else set(idx[1].tolist()) <= set(nine)
    if k > 9:
        assert idx[1, 9:].tolist() == [i for i in range(nc) if i not in set(nine)][: k - 9] and np.isneginf(score[1, 9:]).all()
    assert np.isfinite(score[3, :min(k, nc)]).all()


def test_groups_combined_with_geometry():
    nq, nc, dim, n_groups = 130, 1000, 256, 7
    c, q = P.inputs(nq, nc, dim)
    xy, radius, box = P.geometry(nq, nc)
    cg, qg = P.groups(nq, nc, n_groups)
    s = P.masked_scores(nq, nc, dim, n_groups)
    geo_only = P.masked_scores(nq, nc, dim)
    assert (np.isfinite(s).sum() < np.isfinite(geo_only).sum()) and np.array_equal(s[5], geo_only[5]) and qg[5] == -1   # -1: any group
    for k in (10, 100):
        idx, score = _topk(c, q, k, xy, radius, box, cg, qg)
        P.check(s, k, idx, score)


def test_two_chunks_of_the_score_tile():
    """2700 x 12000 at k = 17: one score row is 96,000 B, a chunk holds 2,688 queries, queries 2,688 .. 2,699 run in the second
    chunk with the per-query arrays offset.  All of the second chunk and every 64th query of the first are compared."""
    from text2pos_amd import _lib as L
    nq, nc, dim, k = 2700, 12000, 128, 17
    assert (L.DEFINES["T2P_SIM_TOPK_MAX_K"], 12000 * 8) == (1024, 96000) and ((256 << 20) - 256) // 96000 // 128 * 128 == 2688
    c, q = P.inputs(nq, nc, dim)
    xy, radius, box = P.geometry(nq, nc)
    rows = np.r_[np.arange(0, 2688, 64), np.arange(2688, nq)]
    s = P.masked(P.scores(c, q[rows]), P.allowed(xy[rows], radius[rows], box))
    assert len({tuple(xy[r]) + (radius[r],) for r in rows[-12:]}) > 6                 # the second chunk's priors differ from one another
    (idx, score), rep = _profiled(lambda: _topk(c, q, k, xy, radius, box))
    assert set(rep) == TILE and all(n == 2 for n, _ in rep.values())
    P.check(s, k, idx[rows], score[rows])


# ---- 2. bit identity where the prior allows everything ------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
def test_an_all_allowing_prior_is_the_other_calls_bit_for_bit(k):
    import text2pos_amd as t2p
    nq, nc = 130, 1000
    c, q = (_up(a) for a in P.inputs(nq, nc))
    xy, _, box = P.geometry(nq, nc)
    inf = np.full(nq, np.inf)
    cg, qg = P.groups(nq, nc, 7)
    qg = np.where(qg < 0, 3, qg).astype(np.int32)                 # (the grouped call has no "any group")
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    geo = dict(cell_boxes=box, query_xy=xy, query_radius=inf)
    for off in (0, 1000):
        plain = t2p.retrieve_topk(c, q, k, index_offset=off)
        grouped = t2p.retrieve_topk(c, q, k, index_offset=off, cell_groups=cg, query_groups=qg)
        assert same(t2p.retrieve_topk(c, q, k, index_offset=off, **geo), plain)                                   # every radius inf
        assert same(t2p.retrieve_topk(c, q, k, index_offset=off, cell_groups=cg, query_groups=qg, **geo), grouped)  # ... plus groups
        assert same(t2p.retrieve_topk(c, q, k, index_offset=off, cell_groups=cg, query_groups=np.full(nq, -1, np.int32), **geo), plain)
        assert int(plain[0].min()) >= off and not same(plain, grouped)


# ---- 3. the route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nc,k,want", [(130, 1000, 10, LISTS), (130, 1000, 17, TILE), (260, 1000, 16, TILE)])
def test_the_prior_call_takes_the_same_two_routes(nq, nc, k, want):
    from text2pos_amd import ops
    c, q = (_up(a) for a in P.inputs(nq, nc))
    xy, radius, box = (_up(a) for a in P.geometry(nq, nc))
    for groups in ({}, dict(zip(("cell_group", "query_group"), (_up(a) for a in P.groups(nq, nc, 7))))):
        _, rep = _profiled(lambda: ops.sim_topk_prior(q, c, k, query_xy=xy, query_radius=radius, cell_box=box, **groups))
        assert set(rep) == want and all(n == 1 for n, _ in rep.values()), rep
    cg, qg = (_up(a) for a in P.groups(nq, nc, 7))
    (idx, score), rep = _profiled(lambda: ops.sim_topk_prior(q, c, k, query_group=qg, cell_group=cg))             # groups alone
    assert set(rep) == want and all(n == 1 for n, _ in rep.values()), rep
    s = P.masked(P.scores(*P.inputs(nq, nc)), P.allowed(None, None, None, qg.cpu().numpy(), cg.cpu().numpy()))
    P.check(s, k, idx.cpu().numpy(), score.cpu().numpy())


# ---- 4. NaN -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 32])
def test_nan_rows_and_nan_boxes(k):
    """60 cells in a row of disjoint 10 m squares, every query at (50, 5) with r = 45: cells 0..9 are in reach, cells 10..59 are not.
    Cell 4 (allowed) and cell 12 (masked) have a NaN row: the nine finite allowed cells come first, cell 4 never, then the masked cells
    10, 11, 12, ... at -inf.  A NaN in any member of cell 7's box masks cell 7: it is retrieved at -inf, first of the masked cells."""
    c, q = (a.copy() for a in P.inputs(4, 60))
    c[4, 5] = np.nan
    c[12, 200] = np.nan
    i = np.arange(60.0)
    box = np.stack([10.0 * i, 0.0 * i, 10.0 * i + 10.0, 0.0 * i + 10.0], axis=1)
    xy, radius = np.tile([50.0, 5.0], (4, 1)), np.full(4, 45.0)
    ok = P.allowed(xy, radius, box)
    assert ok[0].tolist() == [True] * 10 + [False] * 50                            # cell 9 starts at x = 90: dx = 40 <= 45; cell 10: 50
    idx, score = _topk(c, q, k, xy, radius, box)
    allowed = [j for j in range(10) if j != 4]
    for r in range(4):
        assert sorted(idx[r, :9].tolist()) == allowed and np.isfinite(score[r, :9]).all()
        assert idx[r, 9:].tolist() == list(range(10, 10 + k - 9)) and np.isneginf(score[r, 9:]).all()
    assert 12 in idx[0].tolist() and not (idx == 4).any()
    widx, wscore = P.topk(P.masked(P.scores(c, q), ok), k)
    assert np.array_equal(idx, widx) and np.abs(score[:, :9] - wscore[:, :9]).max() < 1e-12
    for member in range(4):
        nb = box.copy()
        nb[7, member] = np.nan
        with pytest.raises(ValueError, match=r"cell_boxes\[7\].*NaN"):
            _topk(c, q, k, xy, radius, nb)
        idx, score = _topk(c, q, k, xy, radius, nb, validate=False)
        still = [j for j in allowed if j != 7]
        for r in range(4):
            assert sorted(idx[r, :8].tolist()) == still and np.isfinite(score[r, :8]).all(), member
            assert idx[r, 8:].tolist() == [7] + list(range(10, 10 + k - 9)) and np.isneginf(score[r, 8:]).all(), member
    # a NaN prior or radius masks every pair of its query (the wrapper refuses them; the kernel's own answer is all -inf)
    for what in ("x", "y", "r", "negative r"):
        bxy, brad = xy.copy(), radius.copy()
        if what in ("x", "y"):
            bxy[2, "xy".index(what)] = np.nan
        else:
            brad[2] = np.nan if what == "r" else -1.0
        with pytest.raises(ValueError, match=r"\[2\]"):
            _topk(c, q, k, bxy, brad, box)
        idx, score = _topk(c, q, k, bxy, brad, box, validate=False)
        assert idx[2].tolist() == list(range(k)) and np.isneginf(score[2]).all(), what
        assert sorted(idx[1, :9].tolist()) == allowed and np.isfinite(score[1, :9]).all(), what


# ---- 5. nothing is read past cell_box[nc - 1] or cell_group[nc - 1] -----------------------------------------------------
@pytest.mark.parametrize("k", [16, 100])
def test_boxes_and_groups_are_not_read_past_the_end(k):
    """nc = 1001 (a ragged last 32-cell block); cell_box and cell_group are the first 1001 entries of longer tensors whose following
    entries would pass (a box around every prior, the queries' group), while the last 40 real cells are masked: no index >= nc
    appears and the result is that of exactly sized copies."""
    from text2pos_amd import ops
    nq, nc = 33, 1001
    c, q = (_up(a) for a in P.inputs(nq, nc))
    xy, radius, box = P.geometry(nq, nc)
    radius = np.where(np.isinf(radius), 60.0, radius)
    longer_box = np.tile([-1e6, -1e6, 1e6, 1e6], (2048, 1))
    longer_box[:nc] = box
    longer_box[nc - 40:nc] = [5e6, 5e6, 5e6 + 30, 5e6 + 30]                         # out of every prior's reach
    longer_grp = np.ones(2048, np.int32)
    longer_grp[:nc] = np.random.default_rng(3).integers(0, 2, nc)
    longer_box, longer_grp = _up(longer_box), _up(longer_grp)
    vb, vg = longer_box[:nc], longer_grp[:nc]
    assert vb.data_ptr() == longer_box.data_ptr() and vb.is_contiguous() and vg.data_ptr() == longer_grp.data_ptr()
    dxy, drad, qg = _up(xy), _up(radius), torch.ones(nq, dtype=torch.int32, device=_dev())
    for groups_v, groups_e in (({}, {}), (dict(query_group=qg, cell_group=vg), dict(query_group=qg, cell_group=vg.clone()))):
        vi, vs = ops.sim_topk_prior(q, c, k, query_xy=dxy, query_radius=drad, cell_box=vb, **groups_v)
        ei, es = ops.sim_topk_prior(q, c, k, query_xy=dxy, query_radius=drad, cell_box=vb.clone(), **groups_e)
        assert int(vi.max()) < nc and int(vi.min()) >= 0
        assert torch.equal(vi, ei) and torch.equal(vs.view(torch.int64), es.view(torch.int64))
        ok = P.allowed(xy, radius, vb.cpu().numpy(), *((qg.cpu().numpy(), vg.cpu().numpy()) if groups_v else (None, None)))
        assert not ok[:, nc - 40:].any()
        P.check(P.masked(P.scores(*P.inputs(nq, nc)), ok), k, vi.cpu().numpy(), vs.cpu().numpy())


# ---- 6. other widths, refusals ------------------------------------------------------------------------------------------
def test_embed_dim_300_is_padded():
    """embed_dim 300 -> the 384 kernels with zero columns, restricted as unrestricted."""
    rng = np.random.default_rng(300)
    c = rng.standard_normal((500, 300)).astype(np.float32)
    q = rng.standard_normal((9, 300)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    xy, radius, box = P.geometry(9, 500)
    cg, qg = rng.integers(0, 3, 500).astype(np.int64), rng.integers(-1, 3, 9).astype(np.int64)     # int64 input is converted
    for k in (10, 20):
        idx, score = _topk(c, q, k, xy, radius, box, cg, qg)
        P.check(P.masked(P.scores(c, q), P.allowed(xy, radius, box, qg, cg)), k, idx, score)


def test_wrapper_refusals():
    import text2pos_amd as t2p
    from text2pos_amd import _lib as L, ops
    nq, nc = 130, 1000
    c, q = (_up(a) for a in P.inputs(nq, nc))
    xy, radius, box = (_up(a) for a in P.geometry(nq, nc))
    cg, qg = (_up(a) for a in P.groups(nq, nc, 7))
    geo = dict(query_xy=xy, query_radius=radius, cell_box=box)
    ops.profile_enable(True)
    try:
        for k in (0, 1025):
            with pytest.raises(L.T2PError, match=r"\[1,1024\]"):
                ops.sim_topk_prior(q, c, k, **geo)
        for bad, text in ((dict(query_xy=xy[:-1].contiguous()), "expected"), (dict(query_radius=radius[:-1].contiguous()), "expected"),
                          (dict(cell_box=box[:, :2].contiguous()), "expected"), (dict(query_xy=xy.float()), "float64"),
                          (dict(query_radius=radius.float()), "float64"), (dict(cell_box=box.float()), "float64"),
                          (dict(cell_box=box.cpu()), "no CPU path"), (dict(query_xy=xy.t().contiguous().t()), "contiguous"),
                          (dict(query_group=qg.long(), cell_group=cg), "int32"), (dict(query_group=qg[:-1].contiguous(), cell_group=cg), "query groups"),
                          (dict(query_group=qg), "go together"), (dict(cell_box=None), "go together")):
            with pytest.raises(RuntimeError, match=text):
                ops.sim_topk_prior(q, c, 10, **{**geo, **bad})
        with pytest.raises(RuntimeError, match="call sim_topk"):
            ops.sim_topk_prior(q, c, 10)
        with pytest.raises(RuntimeError, match="dim"):
            ops.sim_topk_prior(q, c[:, :128].contiguous(), 10, **geo)
    finally:
        ops.profile_enable(False)
    assert ops.profile_report() == {}                                                # nothing was launched
    with pytest.raises(ValueError, match="go together"):
        t2p.retrieve_topk(c, q, 10, cell_boxes=box, query_xy=xy)
    with pytest.raises(ValueError, match=r"query_radius has shape \(129,\)"):
        t2p.retrieve_topk(c, q, 10, cell_boxes=box, query_xy=xy, query_radius=radius[:-1])
    idx, score = ops.sim_topk_prior(q[:0], c, 10, **dict(geo, query_xy=xy[:0], query_radius=radius[:0]))
    assert tuple(idx.shape) == (0, 10) and tuple(score.shape) == (0, 10)
