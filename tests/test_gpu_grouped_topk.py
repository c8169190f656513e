"""t2p_sim_topk_grouped (csrc/sim_topk.hip, MASK_GROUP instantiations) against tests/topk_ref.py's NumPy restatement of the
reference's street oracle (evaluation/pipeline.py:93-108): per query float64 `C @ q` on one BLAS thread, every cell of another group set to -inf, stable
descending argsort.  Indices must match exactly, finite scores within 1e-12 (the project's bar for float64 scores), masked entries
are exactly -inf in ascending index.  Every case first asserts that the yardstick's finite gaps inside the top k + 1 are 0 or above
1e-10, so a last-bit difference between the kernel's fma chain and BLAS cannot reorder anything but exact duplicates."""
import numpy as np
import pytest
import torch

import topk_ref as R
from topk_ref import dev as _dev, inputs as _inputs, strict_groups as _groups

pytestmark = pytest.mark.gpu


def _restate_scores(c, q, cg, qg):
    return R.masked(R.scores(c, q), R.same_group(qg, cg))


def _topk(c, q, k, cg, qg, **kw):
    import text2pos_amd as t2p
    c, q = (torch.tensor(a, device=_dev()) if isinstance(a, np.ndarray) else a for a in (c, q))   # (the cached inputs are read-only)
    idx, score = t2p.retrieve_topk(c, q, k, cell_groups=np.array(cg), query_groups=np.array(qg), **kw)
    return idx.cpu().numpy(), score.cpu().numpy()


# ---- 1. against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nc,dim,n_groups,k", [(130, 1000, 256, 7, 1), (130, 1000, 256, 7, 10), (130, 1000, 256, 7, 16),
                                                  (130, 1000, 256, 7, 17), (130, 1000, 256, 7, 100),
                                                  (257, 4099, 128, 13, 100),
                                                  (37, 2500, 384, 5, 16),
                                                  (17, 12000, 256, 3, 1024)])
def test_grouped_vs_restatement(nq, nc, dim, n_groups, k):
    c, q = _inputs(nq, nc, dim)
    cg, qg = _groups(nq, nc, n_groups)
    idx, score = _topk(c, q, k, cg, qg)
    R.check(R.grouped_scores(nq, nc, dim, n_groups), k, idx, score)
    # query 0's group is empty: masked cells only, 0 .. k-1; query 1's group has 5 cells: they come first
    assert idx[0].tolist() == list(range(k)) and np.isneginf(score[0]).all()
    five = set(np.flatnonzero(cg == n_groups - 2).tolist())
    assert set(idx[1, :min(k, 5)].tolist()) <= five and np.isfinite(score[1, :min(k, 5)]).all()
    if k > 5:
        rest = [i for i in range(nc) if i not in five][: k - 5]
        assert idx[1, 5:].tolist() == rest and np.isneginf(score[1, 5:]).all()


# ---- 2. one group: the ungrouped call, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
def test_all_one_group_is_the_ungrouped_call(k):
    import text2pos_amd as t2p
    nq, nc = 130, 1000
    c, q = (torch.tensor(a, device=_dev()) for a in _inputs(nq, nc))
    cg, qg = np.full(nc, -7, np.int32), np.full(nq, -7, np.int32)
    for off in (0, 1000):
        wi, ws = t2p.retrieve_topk(c, q, k, index_offset=off)
        gi, gs = t2p.retrieve_topk(c, q, k, index_offset=off, cell_groups=cg, query_groups=qg)
        assert torch.equal(wi, gi) and torch.equal(ws.view(torch.int64), gs.view(torch.int64))
        assert int(wi.min()) >= off


# ---- 3. ties across the mask --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [17, 40, 16])
def test_ties_across_the_mask(k):
    """Rows 100..159 copy row 3 and query 0 IS row 3; rows 100..129 are in the query's group, rows 3 and 130..159 are not.  k = 17:
    rows 100..116.  k = 40: rows 100..129, then the ten best distinct allowed cells.  Masked copies never appear while allowed
    cells remain."""
    c, q = (a.copy() for a in _inputs(33, 1000))
    fresh = np.random.default_rng(5).standard_normal((2, 256)).astype(np.float32)
    c[[7, 39]] = fresh / np.linalg.norm(fresh, axis=1, keepdims=True)     # (the generator's own two copies of row 3 go)
    c[100:160] = c[3]
    q[0] = c[3]
    cg = np.random.default_rng(9).integers(0, 2, 1000).astype(np.int32)   # groups 0 / 1 elsewhere
    cg[100:130] = 1
    cg[3] = 0
    cg[130:160] = 0
    qg = np.ones(33, np.int32)
    idx, score = _topk(c, q, k, cg, qg)
    s = _restate_scores(c, q, cg, qg)
    R.check(s, k, idx, score)
    assert idx[0, :min(k, 30)].tolist() == list(range(100, 100 + min(k, 30)))
    assert (score[0, :min(k, 30)] == score[0, 0]).all()
    masked_copies = {3} | set(range(130, 160))
    assert not (set(idx[0].tolist()) & masked_copies) and np.isfinite(score).all()
    assert (cg[idx] == 1).all()
    if k > 30:
        assert (score[0, 30:] < score[0, 0]).all() and len(set(idx[0, 30:].tolist())) == k - 30


# ---- 4. NaN -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 32])
def test_nan_allowed_never_masked_as_minus_inf(k):
    """Cells 0..9 are the queries' group, cells 10..59 are not; cell 4 (allowed) and cell 12 (masked) have a NaN row.  The nine
    finite allowed cells come first, cell 4 never, then the masked cells 10, 11, 12, ... at -inf: the mask is a select."""
    c, q = (a.copy() for a in _inputs(4, 60))
    c[4, 5] = np.nan
    c[12, 200] = np.nan
    cg = np.r_[np.zeros(10, np.int32), np.ones(50, np.int32)]
    qg = np.zeros(4, np.int32)
    idx, score = _topk(c, q, k, cg, qg)
    allowed = [i for i in range(10) if i != 4]
    for r in range(4):
        assert sorted(idx[r, :9].tolist()) == allowed and np.isfinite(score[r, :9]).all()
        assert idx[r, 9:].tolist() == list(range(10, 10 + k - 9)) and np.isneginf(score[r, 9:]).all()
    assert 12 in idx[0].tolist() and not (idx == 4).any()
    s = _restate_scores(c, q, cg, qg)
    widx, wscore = R.topk(s, k)                                   # (NumPy sorts the allowed NaN last: beyond k)
    assert np.array_equal(idx, widx) and np.abs(score[:, :9] - wscore[:, :9]).max() < 1e-12


# ---- 5. nothing is read past cell_group[nc - 1] -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 100])
def test_cell_groups_are_not_read_past_the_end(k):
    """nc = 1001 (a ragged last 32-cell block); cell_group is the first 1001 entries of a longer tensor whose following entries
    equal the queries' group: no index >= nc appears and the result is that of an exactly sized copy."""
    nq, nc = 33, 1001
    c, q = (torch.tensor(a, device=_dev()) for a in _inputs(nq, nc))
    longer = np.ones(2048, np.int32)
    longer[:nc] = np.random.default_rng(3).integers(0, 2, nc)
    longer[nc - 40:nc] = 0                                               # the last cells are masked; what follows them is not
    longer = torch.tensor(longer, device=_dev())
    qg = torch.ones(nq, dtype=torch.int32, device=_dev())
    view = longer[:nc]
    assert view.data_ptr() == longer.data_ptr() and view.is_contiguous()
    import text2pos_amd as t2p
    vi, vs = t2p.retrieve_topk(c, q, k, cell_groups=view, query_groups=qg)
    ei, es = t2p.retrieve_topk(c, q, k, cell_groups=view.clone(), query_groups=qg)
    assert int(vi.max()) < nc and int(vi.min()) >= 0
    assert torch.equal(vi, ei) and torch.equal(vs.view(torch.int64), es.view(torch.int64))
    R.check(_restate_scores(c.cpu().numpy(), q.cpu().numpy(), view.cpu().numpy(), qg.cpu().numpy()), k, vi.cpu().numpy(), vs.cpu().numpy())


# ---- 6. which kernels run, what is refused ------------------------------------------------------------------------------
def test_grouped_call_runs_the_same_two_paths_and_refuses_bad_arguments():
    import text2pos_amd as t2p
    from text2pos_amd import _lib as L, ops
    c, q = (torch.tensor(a, device=_dev()) for a in _inputs(130, 1000))
    cg, qg = (torch.tensor(a, device=_dev()) for a in _groups(130, 1000, 7))
    for k, want in ((10, {"sim_partial", "topk_merge"}), (17, {"sim_scores", "topk_select"})):
        torch.cuda.synchronize()
        ops.profile_report()
        ops.profile_enable(True)
        try:
            ops.sim_topk_grouped(q, c, qg, cg, k)
        finally:
            ops.profile_enable(False)
        rep = ops.profile_report()
        assert set(rep) == want and all(n == 1 for n, _ in rep.values())
    ops.profile_enable(True)
    try:
        for k in (0, 1025):
            with pytest.raises(L.T2PError, match=r"\[1,1024\]"):
                ops.sim_topk_grouped(q, c, qg, cg, k)
        with pytest.raises(RuntimeError, match="query groups"):
            ops.sim_topk_grouped(q, c, qg[:-1], cg, 10)
        with pytest.raises(RuntimeError, match="int32"):
            ops.sim_topk_grouped(q, c, qg.long(), cg, 10)
    finally:
        ops.profile_enable(False)
    assert ops.profile_report() == {}
    with pytest.raises(ValueError, match="outside int32"):
        t2p.retrieve_topk(c, q, 10, cell_groups=np.full(1000, 2 ** 31, np.int64), query_groups=np.zeros(130, np.int64))
    with pytest.raises(ValueError, match="go together"):
        t2p.retrieve_topk(c, q, 10, cell_groups=cg)


def test_embed_dim_300_is_padded():
    """embed_dim 300 -> the 384 kernel with zero columns, grouped as ungrouped."""
    rng = np.random.default_rng(300)
    c = rng.standard_normal((500, 300)).astype(np.float32)
    q = rng.standard_normal((9, 300)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    cg, qg = rng.integers(0, 3, 500).astype(np.int64), rng.integers(0, 3, 9).astype(np.int64)   # int64 input is converted
    idx, score = _topk(c, q, 20, cg, qg)
    R.check(_restate_scores(c, q, cg, qg), 20, idx, score)
