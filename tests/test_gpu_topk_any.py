"""t2p_sim_topk for 17 <= k <= 1024 (csrc/sim_topk.hip: score tile + radix selection + LDS sort) against the float64 oracle,
and the k <= 16 register-list path left exactly as it was.  Scores must agree with the oracle to 1e-12 (the project's bar
for float64 scores) and indices exactly; every shape's oracle scores are checked for near-ties first, so a last-bit
difference between the kernel's fma chain and BLAS cannot reorder anything but exact duplicates."""
import functools

import numpy as np
import pytest
import torch

from topk_ref import dev as _dev, inputs as _inputs, profiled as _profiled

pytestmark = pytest.mark.gpu

KMAX = 1024


@functools.lru_cache(maxsize=None)
def _device_inputs(nq, nc, dim=256):
    c, q = _inputs(nq, nc, dim)
    return torch.tensor(c, device=_dev()), torch.tensor(q, device=_dev())


def _oracle(c, q, k):
    """oracle.model.retrieve_topk_f64 on ONE BLAS thread (a pool computes the last rows of each thread's block through another
    kernel, so two copies of a row can differ in the last bit and lose their tie: test_retrieval_config3_one_ranks_share)."""
    from oracle.model import retrieve_topk_f64
    from threadpoolctl import threadpool_limits
    with threadpool_limits(limits=1, user_api="blas"):
        return retrieve_topk_f64(np.asarray(c), np.asarray(q), k)


def _topk(c, q, k, **kw):
    import text2pos_amd as t2p
    idx, score = t2p.retrieve_topk(c, q, k, **kw)
    return idx.cpu().numpy(), score.cpu().numpy()


def _check_vs_oracle(c, q, k, idx, score):
    nc = c.shape[0]
    kk = min(k, nc)
    widx, wscore = _oracle(c, q, min(k + 1, nc))
    gaps = wscore[:, :-1] - wscore[:, 1:]
    assert (gaps >= 0).all()
    assert gaps[gaps != 0].size == 0 or gaps[gaps != 0].min() > 1e-10, "the generator produced a near-tie inside the top k + 1"
    print(f"nq={q.shape[0]} nc={nc} k={k}: min non-zero oracle gap {gaps[gaps != 0].min() if (gaps != 0).any() else float('nan'):.2e}, "
          f"max|score - oracle| {np.abs(score[:, :kk] - wscore[:, :kk]).max():.2e}")
    assert idx.shape == (q.shape[0], k) and score.shape == (q.shape[0], k)
    assert np.array_equal(idx[:, :kk], widx[:, :kk])
    assert np.abs(score[:, :kk] - wscore[:, :kk]).max() < 1e-12
    if nc < k:
        assert (idx[:, nc:] == -1).all() and np.isneginf(score[:, nc:]).all()


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nc,k,dim", [(3, 40, 64, 256),           # k > nc: the tail is -1 / -inf
                                         (130, 1000, 17, 256),       # the first k of the select path; a partial query block
                                         (257, 4099, 100, 128),      # odd sizes, dim 128
                                         (17, 12000, 1024, 256),     # KMAX
                                         (5, 1024, 1024, 384),       # the full ranking, k == nc, dim 384
                                         (64, 100001, 256, 256)])    # BASELINE configs[2]'s uneven database
def test_any_k_vs_oracle(nq, nc, k, dim):
    c, q = _inputs(nq, nc, dim)
    dc, dq = _device_inputs(nq, nc, dim)
    idx, score = _topk(dc, dq, k)
    _check_vs_oracle(c, q, k, idx, score)


# ---- 2. ties at the k-th place ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [17, 20, 61, 62])
def test_ties_at_kth_place_keep_lowest_indices(k):
    """Rows 100..159 copy row 3 and query 0 IS row 3: 61 cells tie for rank 1 of query 0.  The k kept are row 3 and the copies of
    lowest index, ascending (k = 62: all 61, then the runner-up)."""
    c, q = (a.copy() for a in _inputs(33, 1000))
    fresh = np.random.default_rng(5).standard_normal((2, 256)).astype(np.float32)
    c[[7, 39]] = fresh / np.linalg.norm(fresh, axis=1, keepdims=True)     # (the generator's own two copies of row 3 go)
    c[100:160] = c[3]
    q[0] = c[3]
    idx, score = _topk(c, q, k)
    tied = [3] + list(range(100, 160))
    assert idx[0, :min(k, 61)].tolist() == tied[:min(k, 61)]
    assert (score[0, :min(k, 61)] == score[0, 0]).all()
    if k > 61:
        assert idx[0, 61] not in tied and score[0, 61] < score[0, 0]
    widx, wscore = _oracle(c, q, k)
    assert np.array_equal(idx, widx)
    assert np.abs(score - wscore).max() < 1e-12


def test_all_rows_identical():
    """5,000 copies of one row: every cell ties at every place; the 300 kept are cells 0..299 in order."""
    c0, q = _inputs(9, 50)
    c = np.ascontiguousarray(np.tile(c0[:1], (5000, 1)))
    idx, score = _topk(c, q, 300)
    assert np.array_equal(idx, np.tile(np.arange(300), (9, 1)))
    assert (score == score[:, :1]).all()
    assert np.abs(score[:, 0] - c[0].astype(np.float64) @ q.astype(np.float64).T).max() < 1e-12


def test_signed_zero_scores_tie():
    """Queries live in dims 0..127; rows 0..149 of the database are zero there (their scores are exact zeros, sums of +0.0 and
    -0.0 products: row 5 carries -0.0 where row 4 carries +0.0, row 6 is row 4 negated), rows 150..199 are not.  Zero scores tie
    whatever their sign and come out by ascending index, between the positive and the negative scores."""
    rng = np.random.default_rng(77)
    c = rng.standard_normal((200, 256)).astype(np.float32)
    c[:150, :128] = 0.0
    c[5, :128] = -0.0
    c[6] = -c[4]
    assert np.signbit(c[6, :128]).all() and np.signbit(c[5, :128]).all() and not np.signbit(c[4, :128]).any()
    q = rng.standard_normal((6, 256)).astype(np.float32)
    q[:, 128:] = 0.0
    q[3] = -np.abs(q[3])          # every product of a query with a zero row has the sign of the zero, or its opposite
    q[4, :128] = np.abs(q[4, :128])
    k = 190
    idx, score = _topk(c, q, k)
    widx, wscore = _oracle(c, q, k)
    assert np.array_equal(idx, widx)
    assert np.abs(score - wscore).max() < 1e-12
    for r in range(6):
        zero = np.flatnonzero(score[r] == 0.0)
        assert len(zero) == 150 and idx[r, zero].tolist() == list(range(150))        # one block, by index
        assert (score[r, :zero[0]] > 0).all() and (score[r, zero[-1] + 1:] < 0).all()


# ---- 3. same bits across k ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nc", [(257, 4099), (1250, 12000)])
def test_same_bits_across_k(nq, nc):
    """A pair's score does not depend on k and neither does the order: the k = 16 result (register lists) is the prefix of the
    k = 17 and k = 1024 results (score tile + selection), indices and score bits."""
    dc, dq = _device_inputs(nq, nc)
    i16, s16 = _topk(dc, dq, 16)
    i17, s17 = _topk(dc, dq, 17)
    i100, s100 = _topk(dc, dq, 100)
    imax, smax = _topk(dc, dq, KMAX)
    for i, s in ((i17, s17), (imax, smax)):
        assert np.array_equal(i[:, :16], i16)
        assert np.array_equal(s[:, :16].view(np.int64), s16.view(np.int64))
    assert np.array_equal(imax[:, :100], i100) and np.array_equal(smax[:, :100].view(np.int64), s100.view(np.int64))
    assert (imax >= 0).all() and all(len(set(r.tolist())) == KMAX for r in imax[:8])
    ioff, soff = _topk(dc, dq, 100, index_offset=5000)
    assert np.array_equal(ioff, i100 + 5000) and np.array_equal(soff.view(np.int64), s100.view(np.int64))


# ---- 4. NaN and short lists ---------------------------------------------------------------------------------------------
def test_nan_row_is_never_retrieved():
    c, q = (a.copy() for a in _inputs(4, 20))
    c[11, 5] = np.nan
    idx, score = _topk(c, q, 32)
    assert (idx[:, 19:] == -1).all() and np.isneginf(score[:, 19:]).all()
    assert (idx[:, :19] >= 0).all() and not (idx == 11).any() and np.isfinite(score[:, :19]).all()
    assert all(sorted(r.tolist()) == [i for i in range(20) if i != 11] for r in idx[:, :19])
    keep = np.array([i for i in range(20) if i != 11])
    widx, wscore = _oracle(c[keep], q, 19)
    assert np.array_equal(idx[:, :19], keep[widx]) and np.abs(score[:, :19] - wscore).max() < 1e-12
    i16, s16 = _topk(c, q, 16)
    assert np.array_equal(idx[:, :16], i16) and np.array_equal(score[:, :16].view(np.int64), s16.view(np.int64))


# ---- 5. determinism -----------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    import text2pos_amd as t2p
    dc, dq = _device_inputs(1000, 12000)
    a_i, a_s = t2p.retrieve_topk(dc, dq, 100)
    a_i, a_s = a_i.clone(), a_s.clone()
    b_i, b_s = t2p.retrieve_topk(dc, dq, 100)
    assert torch.equal(a_i, b_i) and torch.equal(a_s.view(torch.int64), b_s.view(torch.int64))


# ---- 6. k <= 16 untouched -----------------------------------------------------------------------------------------------
def _kernel_names(dc, dq, k):
    import text2pos_amd as t2p
    return _profiled(lambda: t2p.retrieve_topk(dc, dq, k))[1]


def test_small_k_runs_the_register_list_kernels():
    from text2pos_amd import _lib as L
    dc, dq = _device_inputs(130, 1000)
    rep = _kernel_names(dc, dq, 10)
    assert set(rep) == {"sim_partial", "topk_merge"} and all(n == 1 for n, _ in rep.values())
    rep = _kernel_names(dc, dq, 17)          # the select path does not reuse topk_merge
    assert set(rep) == {"sim_scores", "topk_select"} and all(n == 1 for n, _ in rep.values())
    for nq, nc in ((130, 1000), (1000, 12000), (1250, 100000)):
        sizes = {L.lib().t2p_sim_topk_workspace_bytes(nq, nc, k) for k in (1, 10, 16)}
        assert len(sizes) == 1


# ---- 7. refusals launch nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, KMAX + 1])
def test_refused_k(k):
    import text2pos_amd as t2p
    from text2pos_amd import _lib as L, ops
    dc, dq = _device_inputs(130, 1000)
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        with pytest.raises(L.T2PError, match=r"\[1,1024\]"):
            t2p.retrieve_topk(dc, dq, k)
    finally:
        ops.profile_enable(False)
    assert ops.profile_report() == {}


def test_no_queries_launch_nothing():
    import text2pos_amd as t2p
    from text2pos_amd import ops
    dc, _ = _device_inputs(130, 1000)
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        idx, score = t2p.retrieve_topk(dc, torch.zeros((0, 256), device=_dev()), 100)
    finally:
        ops.profile_enable(False)
    assert ops.profile_report() == {} and idx.shape == (0, 100) and score.shape == (0, 100)


# ---- 8. shard merge at k = 100 ------------------------------------------------------------------------------------------
def test_shard_merge_at_k_100():
    """The (64, 100001) database ranked shard by shard (8 shards of distributed.shard_range, their index offsets) and merged on the
    host by (score descending, index ascending) equals the unsharded ranking."""
    from text2pos_amd import distributed as TD
    nc, k = 100001, 100
    dc, dq = _device_inputs(64, nc)
    idx, score = _topk(dc, dq, k)
    cand_i, cand_s = [], []
    for r in range(8):
        lo, hi = TD.shard_range(nc, r, 8)
        i_r, s_r = _topk(dc[lo:hi], dq, k, index_offset=lo)
        cand_i.append(i_r)
        cand_s.append(s_r)
    cand_i, cand_s = np.concatenate(cand_i, 1), np.concatenate(cand_s, 1)
    order = np.lexsort((cand_i, -cand_s), axis=1)[:, :k]
    assert np.array_equal(np.take_along_axis(cand_i, order, 1), idx)
    assert np.array_equal(np.take_along_axis(cand_s, order, 1), score)


# ---- 9. pipeline --------------------------------------------------------------------------------------------------------
def test_pipeline_top_k_20(hip_model, fine_pair_gpu):
    """run_coarse / evaluate with top_k = (1, 5, 20) on the synthetic scene of tests/test_gpu_headline.py (36 cells, 16 poses): 20
    distinct cells per query whose first 5 are the (1, 5) run's list, equal k = 1 / k = 5 tables, and all three stages' tables
    keyed 1 / 5 / 20; a top_k beyond the kernel's limit is refused before the model is asked for anything."""
    from test_gpu_headline import _toy_scene
    from text2pos_amd import io as IO, pipeline as PL
    np.random.seed(7)      # Object3d.create_padding draws from np.random
    cells, poses = _toy_scene(n_cells=36, n_poses=16, seed=13)
    sc = IO.Scenes(cells, poses)
    threshs = (5, 10, 15)
    tf = PL.PerCellTransform(256, 5)
    retr20, acc20 = PL.run_coarse(hip_model, sc, tf, (1, 5, 20), threshs)
    retr5, acc5 = PL.run_coarse(hip_model, sc, tf, (1, 5), threshs)
    assert len(retr20) == 16 and all(len(r) == 20 and len(set(r)) == 20 for r in retr20)
    assert [r[:5] for r in retr20] == retr5
    for name in ("hit", "close", "localisation"):
        assert set(acc20[name]) == {1, 5, 20}
        assert acc20[name][1] == acc5[name][1] and acc20[name][5] == acc5[name][5]
    assert acc20["hit"][20] >= acc20["hit"][5] >= acc20["hit"][1]
    prod_fine, _ = fine_pair_gpu
    out = PL.evaluate(hip_model, prod_fine, sc, tf, top_k=(1, 5, 20), threshs=threshs, pad_size=16)
    assert out["retrievals"] == retr20
    for name in ("hit", "close", "localisation", "fine_mean", "fine_offset"):
        assert set(out[name]) == {1, 5, 20}, name
    assert set(out["fine_mean_conf"]) == {1}

    class Spy:
        device, embed_dim = _dev(), 256

        def _fail(self, *a, **kw):
            raise AssertionError("the model was called before top_k was checked")
        encode_objects = encode_text = encode_scene_cells = encode_objects_packed = __call__ = _fail

    for fn in (lambda: PL.run_coarse(Spy(), sc, tf, (1, 2000), threshs),
               lambda: PL.evaluate(Spy(), Spy(), sc, tf, top_k=(1, 2000), threshs=threshs)):
        with pytest.raises(ValueError, match="1024"):
            fn()
