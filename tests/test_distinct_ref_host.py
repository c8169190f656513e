"""tests/distinct_ref.py, the float64 statement of the distinct-candidates selection, proved on its own: random 10 m grids with
duplicate centres, score ties and groups.  Nothing here touches the library; the GPU tests hold t2p_topk_distinct to this file."""
import numpy as np
import pytest

import distinct_ref as R


def grid_case(seed, nq, nc, n_groups=0, tie_every=3):
    """Cells on a square 10 m grid, every fifth one on its predecessor's centre; scores from a small set of values
    (many ties), every tie_every-th cell sharing its predecessor's score in every query; groups (or None)."""
    rng = np.random.default_rng(seed)
    side = max(2, int(np.ceil(np.sqrt(nc))))
    at = rng.permutation(side * side)[:nc]
    xy = np.stack([(at % side) * 10.0, (at // side) * 10.0], axis=1).astype(np.float64)
    xy[4::5] = xy[3::5][: len(xy[4::5])]
    scores = rng.integers(0, max(4, nc // 2), size=(nq, nc)).astype(np.float64) / 64.0
    scores[:, tie_every::tie_every] = scores[:, tie_every - 1:-1:tie_every][:, : scores[:, tie_every::tie_every].shape[1]]
    group = rng.integers(0, n_groups, size=nc).astype(np.int32) if n_groups else None
    return xy, scores, group


def ranking(scores):
    nq, nc = scores.shape
    order = np.stack([np.lexsort((np.arange(nc), -scores[q])) for q in range(nq)])
    return order.astype(np.int64), np.take_along_axis(scores, order, axis=1)


CASES = [(0, 5, 40, 0), (1, 4, 97, 3), (2, 6, 150, 0), (3, 3, 64, 2)]


@pytest.mark.parametrize("seed,nq,nc,n_groups", CASES)
@pytest.mark.parametrize("sep,k", [(10.0, 3), (30.0, 5), (30.0, 12), (1e-9, 4)])
def test_accepted_cells_are_the_greedy_choice(seed, nq, nc, n_groups, sep, k):
    xy, scores, group = grid_case(seed, nq, nc, n_groups)
    idx, n_valid, depth = R.full_ref(scores, xy, group, sep, k)
    order, _ = ranking(scores)
    for q in range(nq):
        acc = idx[q, : n_valid[q]].tolist()
        assert (idx[q, n_valid[q]:] == -1).all() and len(set(acc)) == len(acc)
        for i, a in enumerate(acc):                          # pairwise non-conflicting
            assert not any(R.conflict(xy, group, sep, a, b) for b in acc[:i])
        rank = {int(c): r for r, c in enumerate(order[q])}
        assert [rank[a] for a in acc] == sorted(rank[a] for a in acc)          # in ranking order
        last = rank[acc[-1]]
        for c in order[q, :last].tolist():                   # every skipped cell above the last accepted one lost to an EARLIER accepted cell
            if c not in acc:
                assert any(R.conflict(xy, group, sep, c, a) for a in acc if rank[a] < rank[c]), (q, c)
        if n_valid[q] == k:
            assert depth[q] == last + 1
        else:                                                # fewer than k: every cell of the list conflicts with an accepted one (or is one)
            assert depth[q] == nc + 1
            assert all(c in acc or any(R.conflict(xy, group, sep, c, a) for a in acc) for c in order[q].tolist())


@pytest.mark.parametrize("seed,nq,nc,n_groups", CASES)
def test_sep_zero_is_the_plain_prefix_and_sep_inf_one_cell_per_group(seed, nq, nc, n_groups):
    xy, scores, group = grid_case(seed, nq, nc, n_groups)
    order, ranked = ranking(scores)
    for k in (1, 7, nc):
        idx, n_valid, depth = R.full_ref(scores, xy, group, 0.0, k)
        assert np.array_equal(idx, order[:, :k]) and (n_valid == k).all() and (depth == k).all()
        sidx, sscore, sn, sx = R.select_ref(order[:, :k], ranked[:, :k], xy, group, 0.0, k, nc)      # the smallest pool there is
        assert np.array_equal(sidx, order[:, :k]) and np.array_equal(sscore.view(np.int64), ranked[:, :k].view(np.int64))
        assert (sn == k).all() and (sx == 0).all()
    n_places = max(1, n_groups)
    idx, n_valid, _ = R.full_ref(scores, xy, group, np.inf, n_places + 1)
    for q in range(nq):
        got = idx[q, : n_valid[q]].tolist()
        g = [0] * len(got) if group is None else group[got].tolist()
        assert len(set(g)) == len(g) and n_valid[q] == (1 if group is None else len(set(group.tolist())))
        for c, gc in zip(got, g):                            # each the best cell of its group
            members = np.arange(nc) if group is None else np.flatnonzero(group == gc)
            assert c == members[np.lexsort((members, -scores[q, members]))[0]]


def test_ties_go_to_the_lower_index():
    xy = np.array([[0.0, 0.0], [100.0, 0.0], [100.0, 5.0], [0.0, 5.0], [200.0, 0.0]])
    scores = np.array([[1.0, 1.0, 1.0, 1.0, 1.0], [0.0, -0.0, 2.0, 2.0, -np.inf]])
    idx, n_valid, depth = R.full_ref(scores, xy, None, 10.0, 3)
    assert idx.tolist() == [[0, 1, 4], [2, 3, -1]] and n_valid.tolist() == [3, 2] and depth.tolist() == [5, 5]
    # a masked cell is not a candidate, however it is placed; +-0.0 tie to the lower index
    idx, n_valid, _ = R.full_ref(scores[1:], xy, None, 0.0, 4)
    assert idx.tolist() == [[2, 3, 0, 1]] and n_valid.tolist() == [4]
    # exactly sep apart does not conflict (strict comparison); a NaN centre conflicts with nothing
    xy2 = np.array([[0.0, 0.0], [10.0, 0.0], [np.nan, 0.0], [9.999, 9.999]])
    idx, n_valid, _ = R.full_ref(np.array([[4.0, 3.0, 2.0, 1.0]]), xy2, None, 10.0, 4)
    assert idx.tolist() == [[0, 1, 2, -1]] and n_valid.tolist() == [3]
    # conflicts need both axes within sep, and the same group
    xy3 = np.array([[0.0, 0.0], [5.0, 50.0], [5.0, 5.0], [5.0, 5.0]])
    idx, _, _ = R.full_ref(np.array([[4.0, 3.0, 2.0, 1.0]]), xy3, np.array([0, 0, 0, 1], dtype=np.int32), 10.0, 4)
    assert idx.tolist() == [[0, 1, 3, -1]]


@pytest.mark.parametrize("seed,nq,nc,n_groups", CASES)
@pytest.mark.parametrize("sep,k", [(30.0, 4), (20.0, 9)])
def test_a_pool_of_at_least_the_depth_gives_the_definition(seed, nq, nc, n_groups, sep, k):
    xy, scores, group = grid_case(seed, nq, nc, n_groups)
    scores = scores.copy()
    scores[1, nc // 3:] = -np.inf                            # a query with a restricted list, as the prior path returns it
    order, ranked = ranking(scores)
    want, want_n, depth = R.full_ref(scores, xy, group, sep, k)
    assert (depth <= nc).any()
    seen = set()
    assert depth.max() > k                                   # so the pool one short of it cuts a query short
    for pool in sorted({k, k + 1, int(depth.min()), min(nc, int(depth.max()) - 1), min(nc, int(depth.max())), nc // 2, nc}):
        idx, score, n_valid, exhausted = R.select_ref(order[:, :pool], ranked[:, :pool], xy, group, sep, k, nc)
        for q in range(nq):
            n = n_valid[q]
            assert (idx[q, n:] == order[q, 0]).all() and np.isneginf(score[q, n:]).all()               # the fill rule
            assert np.array_equal(score[q, :n], scores[q, idx[q, :n]])
            if pool >= depth[q] or pool == nc:
                assert exhausted[q] == 0 and n == want_n[q] and np.array_equal(idx[q, :n], want[q, :n])
                seen.add("deep enough")
            else:                                            # too short a pool: a prefix of the definition, and flagged unless it saw the list's end
                assert n < k and np.array_equal(idx[q, :n], want[q, :n])
                assert exhausted[q] == int(np.isfinite(ranked[q, :pool]).all())
                seen.add("cut short")
            if exhausted[q] == 0:
                assert np.array_equal(idx[q, :n], want[q, :n]) and n == want_n[q]
    assert seen == {"deep enough", "cut short"}


def test_select_ref_marks_a_pool_index_outside_the_table():
    xy = np.zeros((5, 2))
    pool_idx = np.array([[0, 1, 2], [0, 4, 2], [3, -1, -1], [7, 9, 8]], dtype=np.int64)
    pool_score = np.array([[3.0, 2.0, 1.0], [3.0, 2.0, 1.0], [1.0, -np.inf, -np.inf], [3.0, 2.0, 1.0]])
    idx, score, n_valid, exhausted = R.select_ref(pool_idx, pool_score, xy, None, 0.0, 2, 4)
    assert n_valid.tolist() == [2, -1, 1, -1] and exhausted.tolist() == [0, 0, 0, 0]
    assert idx.tolist() == [[0, 1], [-1, -1], [3, 3], [-1, -1]] and np.isneginf(score[1]).all() and np.isneginf(score[2, 1])
    idx, _, n_valid, _ = R.select_ref(pool_idx + 5, pool_score, xy, None, 0.0, 2, 5, index_offset=5)   # the offset moves the window
    assert n_valid.tolist() == [2, 2, 1, -1] and idx[1].tolist() == [5, 9]
