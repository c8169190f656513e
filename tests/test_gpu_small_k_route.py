"""t2p_sim_topk / t2p_sim_topk_grouped at k <= 16 take their path by problem size (csrc/sim_topk.hip: nq * nc >=
T2P_SIM_TOPK_TILE_MIN_PAIRS runs k_sim_scores + k_topk_select with the caller's k, below it the register lists run), never by k.
At the smallest routed shape the result is held to the float64 oracle (indices exact, scores to 1e-12) and, bit for bit, to the
register-list path on the same pairs: the same call on query blocks of 8, which stay below the threshold."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_topk_any as TA
from topk_ref import LISTS, TILE, dev as _dev, profiled as _profiled

pytestmark = pytest.mark.gpu

NQ, QBLOCK = 97, 8
KS = (1, 10, 16)


def _ws(nq, nc, k):
    from text2pos_amd import _lib as L
    return int(L.lib().t2p_sim_topk_workspace_bytes(nq, nc, k))


@functools.lru_cache(maxsize=None)
def _threshold():
    """T of the rule nq * nc >= T: the header's constant, confirmed on the library's own size query (one query: below T the
    lists' workspace, from T on one row of the score tile)."""
    from text2pos_amd import _lib as L
    t = L.DEFINES["T2P_SIM_TOPK_TILE_MIN_PAIRS"]
    tile_row = lambda nc: 8 * ((nc + 15) // 16 * 16) + 256
    assert _ws(1, t, 10) == tile_row(t) and _ws(1, t - 1, 10) != tile_row(t - 1)
    assert t > 130 * 1000
    return t


def _routed_nc():
    nc = -(-_threshold() // NQ)
    while nc % 16 == 0:
        nc += 1
    return nc


@functools.lru_cache(maxsize=None)
def _inputs(nq, nc, dim):
    """Finite unit rows; twelve cell rows are exact copies of earlier rows (ties -> ascending index)."""
    rng = np.random.default_rng(97 * nc + dim)
    c = rng.standard_normal((nc, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    dst = rng.choice(np.arange(nc // 2, nc), 12, replace=False)
    src = rng.choice(np.arange(0, nc // 2), 12, replace=False)
    c[dst] = c[src]
    q[0] = c[src[0]]           # query 0's best cell has a copy: a tie at the first place
    assert np.isfinite(c).all() and np.isfinite(q).all()
    c.setflags(write=False)
    q.setflags(write=False)
    return c, q, torch.tensor(c, device=_dev()), torch.tensor(q, device=_dev())


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _by_blocks(fn, nq):
    """fn(q_lo, q_hi) on query blocks of QBLOCK, concatenated; every block call must have run the register-list kernels."""
    idx, score = [], []
    for lo in range(0, nq, QBLOCK):
        hi = min(lo + QBLOCK, nq)
        out, rep = _profiled(lambda: fn(lo, hi))
        assert set(rep) == LISTS and all(n == 1 for n, _ in rep.values()), rep
        i, s = _np(out)
        idx.append(i)
        score.append(s)
    return np.concatenate(idx), np.concatenate(score)


@pytest.mark.parametrize("dim", [256, 128])
def test_routed_call_equals_oracle_and_register_lists(dim):
    import text2pos_amd as t2p
    nc = _routed_nc()
    assert NQ * nc >= _threshold() > QBLOCK * nc and nc % 16 != 0
    c, q, dc, dq = _inputs(NQ, nc, dim)
    for k in KS if dim == 256 else (10,):
        out, rep = _profiled(lambda: t2p.retrieve_topk(dc, dq, k))
        assert set(rep) == TILE and all(n == 1 for n, _ in rep.values()), rep
        idx, score = _np(out)
        TA._check_vs_oracle(c, q, k, idx, score)
        bidx, bscore = _by_blocks(lambda lo, hi: t2p.retrieve_topk(dc, dq[lo:hi], k), NQ)
        assert np.array_equal(idx, bidx)
        assert np.array_equal(score.view(np.int64), bscore.view(np.int64))
    assert (idx[0, :2] >= 0).all() and score[0, 0] == score[0, 1] and idx[0, 0] < idx[0, 1]      # the planted tie


def test_index_offset_on_the_routed_path():
    import text2pos_amd as t2p
    nc = _routed_nc()
    _, _, dc, dq = _inputs(NQ, nc, 256)
    i0, s0 = _np(t2p.retrieve_topk(dc, dq, 10))
    out, rep = _profiled(lambda: t2p.retrieve_topk(dc, dq, 10, index_offset=123456789012))
    assert set(rep) == TILE
    i1, s1 = _np(out)
    assert np.array_equal(i1, i0 + 123456789012) and np.array_equal(s1.view(np.int64), s0.view(np.int64))


def test_grouped_call_takes_the_same_route():
    """Group 5 holds 7 cells (< k = 10): its queries get those 7 by score, then masked cells at -inf in ascending index."""
    from text2pos_amd import ops
    nc, k = _routed_nc(), 10
    c, q, dc, dq = _inputs(NQ, nc, 256)
    rng = np.random.default_rng(3)
    cg = rng.integers(0, 3, nc).astype(np.int32)
    small = np.sort(rng.choice(nc, 7, replace=False))
    cg[small] = 5
    qg = rng.integers(0, 3, NQ).astype(np.int32)
    qg[[2, 50, 96]] = 5
    dcg, dqg = torch.tensor(cg, device=_dev()), torch.tensor(qg, device=_dev())
    out, rep = _profiled(lambda: ops.sim_topk_grouped(dq, dc, dqg, dcg, k))
    assert set(rep) == TILE and all(n == 1 for n, _ in rep.values()), rep
    idx, score = _np(out)
    bidx, bscore = _by_blocks(lambda lo, hi: ops.sim_topk_grouped(dq[lo:hi], dc, dqg[lo:hi], dcg, k), NQ)
    assert np.array_equal(idx, bidx) and np.array_equal(score.view(np.int64), bscore.view(np.int64))
    others = np.flatnonzero(cg != 5)[:k - 7]
    for r in (2, 50, 96):
        want = c[small].astype(np.float64) @ q[r].astype(np.float64)
        order = np.argsort(-want, kind="stable")
        assert np.array_equal(idx[r, :7], small[order]) and np.abs(score[r, :7] - want[order]).max() < 1e-12
        assert np.isneginf(score[r, 7:]).all() and np.array_equal(idx[r, 7:], others)
    for r in (0, 1, 95):                                   # an ordinary group: the unrestricted ranking of its own cells
        keep = np.flatnonzero(cg == qg[r])
        widx, wscore = TA._oracle(c[keep], q[r:r + 1], k)
        assert np.array_equal(idx[r], keep[widx[0]]) and np.abs(score[r] - wscore[0]).max() < 1e-12


def test_small_calls_stay_on_the_lists_and_the_workspace_ignores_k():
    import text2pos_amd as t2p
    _, _, dc, dq = _inputs(130, 1000, 256)
    _, rep = _profiled(lambda: t2p.retrieve_topk(dc, dq, 10))
    assert set(rep) == LISTS and all(n == 1 for n, _ in rep.values())
    t, nc = _threshold(), _routed_nc()
    for nq, n in ((130, 1000), (QBLOCK, nc), (NQ, nc - 16), (NQ, nc), (1000, 12000), (1250, 100000)):
        assert len({_ws(nq, n, k) for k in KS}) == 1, (nq, n)
    assert NQ * (nc - 16) < t and _ws(NQ, nc, 10) == _ws(NQ, nc, 17) and _ws(NQ, nc - 16, 10) != _ws(NQ, nc - 16, 17)
