"""The yardstick of the restricted retrieval (tests/topk_ref.py) on hand cases: no GPU, no package.  The GPU cases of
tests/test_gpu_prior_topk.py and tests/test_gpu_grouped_topk.py compare the kernels with it, so its masks are proved here on pairs
whose answer is known by hand."""
import numpy as np
import pytest

import topk_ref as P

BOX = np.array([[10.0, 20.0, 40.0, 50.0]])          # one cell: [10, 40] x [20, 50]


def _one(x, y, r, box=BOX):
    return bool(P.allowed(np.array([[x, y]], dtype=np.float64), np.array([r], dtype=np.float64), box)[0, 0])


def test_the_345_corner_is_in_and_the_next_radius_below_is_out():
    # 3 left of and 4 below the corner (10, 20): distance exactly 5
    assert _one(7.0, 16.0, 5.0) and not _one(7.0, 16.0, np.nextafter(5.0, 0.0))
    assert _one(43.0, 54.0, 5.0) and not _one(43.0, 54.0, np.nextafter(5.0, 0.0))          # the opposite corner (40, 50)
    assert _one(7.0, 30.0, 3.0) and not _one(7.0, 30.0, np.nextafter(3.0, 0.0))            # an edge: dy = 0
    # the distance is to the square, not to its centre (25, 35): a point 1 m outside a corner is 22 m from the centre
    assert _one(41.0, 50.0, 1.0)


def test_radius_zero_keeps_the_closed_square():
    assert _one(25.0, 35.0, 0.0)                      # inside
    assert _one(10.0, 35.0, 0.0) and _one(25.0, 50.0, 0.0)   # on an edge
    assert _one(10.0, 20.0, 0.0) and _one(40.0, 50.0, 0.0)   # on a corner
    assert not _one(np.nextafter(10.0, 0.0), 35.0, 0.0) and not _one(25.0, np.nextafter(50.0, 60.0), 0.0)   # outside
    assert _one(25.0, 35.0, -0.0)                     # -0.0 >= 0


def test_radius_inf_keeps_every_cell_and_a_negative_radius_none():
    far = np.array([[1e300, -1e300, 1e300, -1e300]])
    assert _one(0.0, 0.0, np.inf, far) and _one(-1e308, 1e308, np.inf)
    assert not _one(25.0, 35.0, -1.0) and not _one(25.0, 35.0, -np.inf) and not _one(25.0, 35.0, -1e-300)


@pytest.mark.parametrize("place", ["px", "py", "r", "x0", "y0", "x1", "y1"])
@pytest.mark.parametrize("radius", [0.0, 60.0, np.inf])
def test_a_nan_in_any_of_the_seven_places_masks_the_pair(place, radius):
    v = dict(px=25.0, py=35.0, r=radius, x0=10.0, y0=20.0, x1=40.0, y1=50.0)
    assert _one(v["px"], v["py"], v["r"], np.array([[v["x0"], v["y0"], v["x1"], v["y1"]]]))          # the point is inside
    v[place] = np.nan
    assert not _one(v["px"], v["py"], v["r"], np.array([[v["x0"], v["y0"], v["x1"], v["y1"]]]))


def test_groups_and_their_combination_with_the_geometry():
    xy, r = np.array([[25.0, 35.0], [25.0, 35.0], [0.0, 0.0]]), np.array([0.0, 0.0, 1.0])
    box = np.array([[10.0, 20.0, 40.0, 50.0], [10.0, 20.0, 40.0, 50.0], [100.0, 100.0, 130.0, 130.0]])
    qg, cg = np.array([-1, 4, -1], np.int32), np.array([4, 5, 4], np.int32)
    assert P.allowed(None, None, None, qg, cg).tolist() == [[True, True, True], [True, False, True], [True, True, True]]
    assert P.allowed(xy, r, box, qg, cg).tolist() == [[True, True, False], [True, False, False], [False, False, False]]
    assert P.allowed(xy, r, box).tolist() == [[True, True, False], [True, True, False], [False, False, False]]


def test_the_grouped_mask_is_strict_where_the_prior_reads_a_negative_id_as_any_group():
    qg, cg = np.array([-1, 4, -7], np.int32), np.array([4, -1, -7, 5], np.int32)
    assert P.same_group(qg, cg).tolist() == [[False, True, False, False], [True, False, False, False], [False, False, True, False]]
    assert P.allowed(None, None, None, qg, cg).tolist() == [[True] * 4, [True, False, False, False], [True] * 4]
    cg7, qg7 = P.strict_groups(130, 1000, 7)
    assert (qg7 >= 0).all() and np.array_equal(P.groups(130, 1000, 7)[0], cg7) and (P.groups(130, 1000, 7)[1][1::5] == qg7[1::5]).all()


def test_masked_pairs_are_minus_inf_whatever_the_product_and_sort_last_in_index_order():
    s = np.array([[0.5, np.nan, 0.9, 0.5, np.nan, 0.1]])
    ok = np.array([[True, False, True, True, True, False]])
    m = P.masked(s, ok)
    assert np.isneginf(m[0, [1, 5]]).all() and np.isnan(m[0, 4])
    idx, sc = P.topk(m, 5)
    assert idx.tolist() == [[2, 0, 3, 1, 5]] and np.isneginf(sc[0, 3:]).all()          # the allowed NaN (cell 4) is beyond them


def test_the_generator_is_what_the_gpu_cases_were_sized_for():
    """Queries 0..3 of every shape allow 0, 9, 18 and all cells; the boundary holds exact equalities; 130 x 1000 has queries with no
    cell and queries with every cell."""
    for nq, nc, _, _ in P.SHAPES[:5]:
        xy, r, box = P.geometry(nq, nc)
        assert all(float(v).is_integer() for v in xy.ravel()) and all(float(v).is_integer() for v in box.ravel())
        ok = P.allowed(xy, r, box)
        assert ok.sum(axis=1)[:4].tolist() == [0, 9, 18, nc], (nq, nc)
        px, py = xy[:, 0, None], xy[:, 1, None]
        dx = np.maximum(np.maximum(box[None, :, 0] - px, px - box[None, :, 2]), 0.0)
        dy = np.maximum(np.maximum(box[None, :, 1] - py, py - box[None, :, 3]), 0.0)
        on = ((dx * dx + dy * dy) == (r * r)[:, None]) & np.isfinite(r)[:, None]
        assert 45 <= int(on.sum()) <= 650 and ok[on].all(), (nq, nc, int(on.sum()))
    n = P.allowed(*P.geometry(130, 1000)).sum(axis=1)
    assert int((n == 0).sum()) == 3 and int((n == 1000).sum()) == 27
    cg, qg = P.groups(130, 1000, 7)
    assert (qg[::5] == -1).all() and (qg[1::5] >= 0).all() and (cg == 5).sum() == 5
