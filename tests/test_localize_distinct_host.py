"""The host side of distinct candidates (no GPU): the arguments of Localizer.localize and of the command, and unpack_result on
hand-made rows of a call with distinct_radius - two more columns, the selection's n_valid and its exhausted flag."""
import json

import numpy as np
import pytest

from text2pos_amd import localize as LZ, retrieval as RT


def test_arguments_are_checked_on_the_host():
    assert LZ.check_distinct_args(None, None, 10, 2048) is None
    assert LZ.check_distinct_args(30, None, 10, 2048) == (30.0, 320)                # 32 k
    assert LZ.check_distinct_args(0, None, 1, 2048) == (0.0, 64)                    # at least one chunk of the kernel
    assert LZ.check_distinct_args(np.inf, None, 100, 2048) == (np.inf, 1024)        # the ranking's limit
    assert LZ.check_distinct_args(np.float32(5), 7, 4, 9) == (5.0, 7) and LZ.check_distinct_args(5.0, None, 4, 9) == (5.0, 9)
    assert RT.default_distinct_pool(2048, 10) == 320 and RT.default_distinct_pool(50, 10) == 50
    for radius, pool in ((-1e-9, None), (float("nan"), None), ("30 m", None), ([1.0], None), (True, None), (-np.inf, None),
                         (1.0, 3), (1.0, 10), (1.0, 4.5), (1.0, True), (None, 9)):
        with pytest.raises(ValueError, match="distinct_radius|distinct_pool"):
            LZ.check_distinct_args(radius, pool, 4, 9)
    with pytest.raises(ValueError, match=r"distinct_pool=2000 outside \[top_k, min\(len\(db\), 1024\)\] = \[10, 1024\]"):
        LZ.check_distinct_args(1.0, 2000, 10, 5000)


def test_command_line_flags():
    base = ["query", "--db", "db.pt", "--path_coarse", "c", "--path_fine", "f", "--hints", "x"]
    a = LZ.parse_args(base)
    assert a.distinct is None and a.distinct_pool is None
    a = LZ.parse_args(base + ["--distinct", "30", "--distinct_pool", "256"])
    assert a.distinct == 30.0 and a.distinct_pool == 256
    assert LZ.parse_args(base + ["--distinct", "inf"]).distinct == np.inf
    with pytest.raises(SystemExit):
        LZ.parse_args(base + ["--distinct_pool", "256"])


def _rows(k, cells, scores, matched, n_valid=None, exhausted=None):
    """Packed rows as Localizer._run_chunk writes them: positions derived from the cell row so that a mix-up shows."""
    cells, scores, matched = (np.asarray(a, dtype=np.float64) for a in (cells, scores, matched))
    nq = len(cells)
    pos = [np.stack([cells + 0.25 * i, cells + 0.5 * i], axis=2).reshape(nq, 2 * k) for i in range(1, 5)]
    cols = [cells, scores] + pos + [matched, np.zeros((nq, 1))]
    if n_valid is not None:
        cols += [np.asarray(n_valid, dtype=np.float64)[:, None], np.asarray(exhausted, dtype=np.float64)[:, None]]
    return np.concatenate(cols, axis=1)


def test_unpack_result_of_a_distinct_call():
    k, ids = 3, [f"c{i}" for i in range(6)]
    inf = -np.inf
    #       three places | two, the pool ran out | one, the list ended | none allowed
    cells = [[4, 0, 2], [5, 1, 5], [3, 3, 3], [0, 0, 0]]
    scores = [[0.9, 0.8, 0.1], [0.7, 0.6, inf], [0.5, inf, inf], [inf, inf, inf]]
    matched = [[1, 3, 3], [0, 2, 5], [2, 4, 4], [1, 1, 1]]
    res = LZ.unpack_result(_rows(k, cells, scores, matched, [3, 2, 1, 0], [0, 1, 0, 0]), k, ids, False, distinct=True)
    assert res.distinct and res.restricted and res.exhausted.dtype == bool and res.exhausted.tolist() == [False, True, False, False]
    assert res.n_valid.tolist() == [3, 2, 1, 0] and res.n_valid.dtype == np.int32
    assert res.cell_rows.tolist() == [[4, 0, 2], [5, 1, -1], [3, -1, -1], [-1, -1, -1]]
    assert res.cell_ids == [["c4", "c0", "c2"], ["c5", "c1", None], ["c3", None, None], [None, None, None]]
    assert res.matched.tolist() == [[1, 3, 3], [0, 2, 0], [2, 0, 0], [0, 0, 0]]
    assert res.best.tolist() == [1, 1, 0, -1]                # most matched among the valid columns, the first on ties
    assert np.array_equal(res.best_world_xy[:3], res.world_xy[[0, 1, 2], [1, 1, 0]]) and np.isnan(res.best_world_xy[3]).all()
    assert np.isnan(res.world_xy[1, 2]).all() and np.isfinite(res.world_xy[1, :2]).all()
    lines = [res.to_json(q) for q in range(4)]
    assert all(json.dumps(line, allow_nan=False) for line in lines)
    assert [line["exhausted"] for line in lines] == [False, True, False, False] and [line["n_valid"] for line in lines] == [3, 2, 1, 0]
    assert lines[1]["cell_ids"] == ["c5", "c1"] and lines[3]["best"] is None and set(lines[0]) == set(LZ._RESULT_FIELDS) | {"n_valid", "exhausted"}
    # a pool index outside the database: the kernel marks the query, the call names it
    with pytest.raises(IndexError, match=r"Localizer.localize: query 2\b.*pool index"):
        LZ.unpack_result(_rows(k, cells, scores, matched, [3, 2, -1, 0], [0, 1, 0, 0]), k, ids, False, distinct=True)


def test_existing_callers_of_unpack_result_are_unaffected():
    k, ids = 2, ["a", "b", "c"]
    rows = _rows(k, [[2, 0], [1, 2]], [[0.5, 0.25], [0.75, -np.inf]], [[1, 2], [3, 4]])
    plain = LZ.unpack_result(rows, k, ids, False)
    assert not plain.distinct and not plain.restricted and plain.exhausted.tolist() == [False, False] and plain.n_valid.tolist() == [2, 2]
    assert set(plain.to_json(0)) == set(LZ._RESULT_FIELDS)
    restricted = LZ.unpack_result(rows, k, ids, True, "somewhere")
    assert restricted.restricted and not restricted.distinct and restricted.n_valid.tolist() == [2, 1]
    assert set(restricted.to_json(1)) == set(LZ._RESULT_FIELDS) | {"n_valid"}
