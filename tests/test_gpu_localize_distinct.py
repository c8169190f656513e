"""Localizer.localize with distinct_radius (-m gpu): the top_k candidates are top_k different places (t2p_topk_distinct over the
ranked pool, include/t2p_select.h).  On the 9-cell toy world of tests/test_gpu_localize_prior.py - disjoint 30 m squares at
(30 (i % 4), 30 (i // 4)), centres 15 m inside - with k = 4.  At a radius of 31 m a cell conflicts with its up to eight neighbours
(the centres are 30 m apart), at 30 m with none (the comparison is strict).  Held to tests/distinct_ref.py and to the composition
retrieve_topk_distinct on the same encodings; the host side (arguments, unpacking) is tests/test_localize_distinct_host.py."""
import json

import numpy as np
import pytest
import torch

import distinct_ref as R
from test_gpu_localize_prior import _calibrate, _dev, _fresh_models, N_PTS, PAD, SEED, HINTS, K
from fine_scene import make_fine_scene

pytestmark = pytest.mark.gpu
RADIUS = 31.0
FIELDS = ("pos_in_cell_mean", "pos_in_cell", "world_xy_mean", "world_xy")


@pytest.fixture(scope="module")
def world(vocab):
    from text2pos_amd import evaluation as E, localize as LZ, pipeline as PL
    from text2pos_amd.scene import DeviceScene
    cells, poses = make_fine_scene(9, 7, 41, PAD, HINTS)
    tf = PL.PerCellTransform(N_PTS, SEED)
    scene = DeviceScene(cells, _dev(), n_pad=PAD, pad_seed=SEED)
    hints = [E.create_hint_description(p) for p in poses]
    coarse, fine = _fresh_models(vocab)
    _calibrate(coarse, fine, scene, tf, hints)
    db = LZ.CellDatabase.build(coarse, fine, cells, tf, PAD)
    centers = np.array([[30.0 * (i % 4) + 15.0, 30.0 * (i // 4) + 15.0] for i in range(9)])
    assert np.array_equal(db.cell_centers().cpu().numpy(), centers)
    names = ["a"] * 4 + ["b"] * 5
    two = LZ.CellDatabase(db.coarse, db.fine, db.center_xy, db.bbox_xy, db.cell_size, db.cell_ids, names, db.meta)
    with torch.no_grad():
        text = coarse.encode_text([" ".join(h) for h in hints])
    return dict(cells=cells, poses=poses, hints=hints, coarse=coarse, fine=fine, db=db, loc=LZ.Localizer(coarse, fine, db), two=two,
                loc_two=LZ.Localizer(coarse, fine, two), centers=centers, text=text,
                one_group=np.zeros(9, dtype=np.int32), two_groups=np.array([0] * 4 + [1] * 5, dtype=np.int32))


def _same(a, b, fields=None):
    for f in fields or list(vars(a)):
        x, y = getattr(a, f), getattr(b, f)
        assert (np.array_equal(x, y, equal_nan=True) if isinstance(x, np.ndarray) else x == y), f


def _profiled(fn):
    from text2pos_amd import ops
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        out = fn()
    finally:
        ops.profile_enable(False)
    return out, ops.profile_report()


def _check_states(res, k, ids):
    """The states of a Localization with fewer than k valid candidates (the restricted handling)."""
    valid = np.arange(k)[None, :] < res.n_valid[:, None]
    assert res.restricted and res.distinct and res.exhausted.dtype == bool and res.n_valid.dtype == np.int32
    assert (res.cell_rows[valid] >= 0).all() and (res.cell_rows[~valid] == -1).all()
    assert np.isfinite(res.scores[valid]).all() and np.isneginf(res.scores[~valid]).all() and (res.matched[~valid] == 0).all()
    assert res.cell_ids == [[ids[j] if ok else None for j, ok in zip(r, v)] for r, v in zip(res.cell_rows, valid)]
    for f in FIELDS:
        assert np.isnan(getattr(res, f)[~valid]).all() and np.isfinite(getattr(res, f)[valid]).all(), f
    best = np.where(res.n_valid > 0, np.argmax(np.where(valid, res.matched, -1), axis=1), -1)      # most matched objects, first on ties
    assert np.array_equal(res.best, best)
    has = res.n_valid > 0
    assert np.array_equal(res.best_world_xy[has], res.world_xy[has, res.best[has]]) and np.isnan(res.best_world_xy[~has]).all()
    return valid


def test_without_a_radius_the_call_is_todays(world):
    from text2pos_amd import localize as LZ
    w, loc = world, world["loc"]
    plain, rep = _profiled(lambda: loc.localize(w["hints"], top_k=K))
    assert "topk_distinct" not in rep and {"sim_partial", "topk_merge"} <= set(rep)
    _same(loc.localize(w["hints"], top_k=K, distinct_radius=None, distinct_pool=None), plain)
    _same(loc.localize_poses(w["poses"], top_k=K, distinct_radius=None), plain)
    assert not plain.restricted and not plain.distinct and plain.exhausted.tolist() == [False] * 7 and plain.exhausted.dtype == bool
    assert set(plain.to_json(0)) == set(LZ._RESULT_FIELDS)
    # radius 0 conflicts with nothing, and 30 m (the centres' distance, compared strictly) neither: the same candidates, bit for bit
    for radius in (0.0, 30.0):
        zero, rep = _profiled(lambda: loc.localize(w["hints"], top_k=K, distinct_radius=radius))
        assert rep["topk_distinct"][0] == 1 and zero.distinct and zero.restricted
        _same(zero, plain, LZ._RESULT_FIELDS + ("n_valid", "exhausted"))


def test_candidates_are_distinct_places(world):
    import text2pos_amd as t2p
    w, loc, db = world, world["loc"], world["db"]
    res = loc.localize(w["hints"], top_k=K, distinct_radius=RADIUS)
    valid = _check_states(res, K, db.cell_ids)
    print("rows:\n", res.cell_rows, "\nn_valid:", res.n_valid.tolist(), "exhausted:", res.exhausted.tolist(), "\nmatched:\n", res.matched)
    for q in range(7):                                       # pairwise non-conflicting
        rows = res.cell_rows[q, : res.n_valid[q]].tolist()
        assert len(rows) >= 1 and not any(R.conflict(w["centers"], None, RADIUS, a, b) for i, a in enumerate(rows) for b in rows[:i])
    assert not res.exhausted.any()                           # the default pool is the whole database
    # rows, n_valid, exhausted: the composition on the same encodings, and the definition on the full ranking
    idx, scores, n_valid, exhausted = (t.cpu().numpy() for t in t2p.retrieve_topk_distinct(
        db.coarse, w["text"], K, db.cell_centers(), RADIUS, cell_groups=None))
    assert np.array_equal(res.n_valid, n_valid) and np.array_equal(res.exhausted, exhausted != 0)
    assert np.array_equal(res.cell_rows[valid], idx[valid]) and np.array_equal(res.scores[valid].view(np.int64), scores[valid].view(np.int64))
    full_i, full_s = (t.cpu().numpy() for t in t2p.retrieve_topk(db.coarse, w["text"], 9))
    s = np.empty((7, 9))
    np.put_along_axis(s, full_i, full_s, axis=1)
    want, want_n, _ = R.full_ref(s, w["centers"], None, RADIUS, K)
    assert np.array_equal(res.n_valid, want_n) and np.array_equal(res.cell_rows, want)
    plain = loc.localize(w["hints"], top_k=K)
    assert (res.cell_rows != plain.cell_rows).any(), "the plain top-4 should hold neighbouring cells somewhere"
    assert (res.n_valid < K).any() and (res.n_valid > 1).all()
    # every selected cell: the positions and matches an unrestricted call reports for that cell
    every = loc.localize(w["hints"], top_k=9)
    for q in range(7):
        for j in range(res.n_valid[q]):
            at = int(np.flatnonzero(every.cell_rows[q] == res.cell_rows[q, j])[0])
            assert res.matched[q, j] == every.matched[q, at] and res.scores[q, j] == every.scores[q, at]
            for f in FIELDS:
                assert np.array_equal(getattr(res, f)[q, j], getattr(every, f)[q, at]), (f, q, j)
    assert (res.matched > 0).any(), "the comparison needs matched objects"
    # the memory knob, mixed hint counts and localize_poses change nothing
    _same(loc.localize(w["hints"], top_k=K, queries_per_call=3, distinct_radius=RADIUS), res)
    _same(loc.localize_poses(w["poses"], top_k=K, distinct_radius=RADIUS, distinct_pool=9), res)
    mixed = [w["hints"][0][:3], w["hints"][1], w["hints"][2][:2], w["hints"][3]]
    both = loc.localize(mixed, top_k=K, distinct_radius=RADIUS)
    parts = [loc.localize([m], top_k=K, distinct_radius=RADIUS) for m in mixed]
    for f in ("cell_rows", "scores", "matched", "n_valid", "exhausted", "best", "world_xy"):
        assert np.array_equal(getattr(both, f), np.concatenate([getattr(p, f) for p in parts]), equal_nan=True), f
    line = res.to_json(int(np.argmin(res.n_valid)))
    assert json.dumps(line, allow_nan=False) and line["exhausted"] is False and line["n_valid"] == len(line["cell_ids"]) == res.n_valid.min()


def test_scenes_and_priors_with_distinct_candidates(world):
    import text2pos_amd as t2p
    w, loc, two = world, world["loc_two"], world["two"]
    hints = w["hints"][:6]
    names = two.scene_names
    # cells of different scenes never suppress each other: at radius inf one cell per scene, the best of each
    res = loc.localize(hints, top_k=K, distinct_radius=np.inf)
    _check_states(res, K, two.cell_ids)
    full_i = t2p.retrieve_topk(two.coarse, w["text"][:6], 9)[0].cpu().numpy()
    assert res.n_valid.tolist() == [2] * 6 and not res.exhausted.any()
    for q in range(6):
        best_of = [next(int(c) for c in full_i[q] if names[c] == s) for s in ("a", "b")]
        assert sorted(res.cell_rows[q, :2].tolist()) == sorted(best_of) and res.cell_rows[q, 0] == full_i[q, 0]
    one = world["loc"].localize(hints, top_k=K, distinct_radius=np.inf)              # one scene: the best cell alone
    assert one.n_valid.tolist() == [1] * 6 and np.array_equal(one.cell_rows[:, 0], full_i[:, 0])
    # with a scene: masked cells are never selected, and the selection is the composition's
    scenes = ["a", "b", None, "a", None, "b"]
    res = loc.localize(hints, top_k=K, scenes=scenes, distinct_radius=RADIUS)
    valid = _check_states(res, K, two.cell_ids)
    for q, s in enumerate(scenes):
        assert s is None or all(names[j] == s for j in res.cell_rows[q, : res.n_valid[q]]), (q, s)
    qg = np.array([-1 if s is None else "ab".index(s) for s in scenes], np.int32)
    idx, scores, n_valid, exhausted = (t.cpu().numpy() for t in t2p.retrieve_topk_distinct(
        two.coarse, w["text"][:6], K, two.cell_centers(), RADIUS, cell_groups=w["two_groups"], query_groups=qg,
        cell_boxes=two.cell_boxes(), query_xy=np.zeros((6, 2)), query_radius=np.full(6, np.inf)))
    assert np.array_equal(res.n_valid, n_valid) and np.array_equal(res.exhausted, exhausted != 0) and not exhausted.any()
    assert np.array_equal(res.cell_rows[valid], idx[valid]) and np.array_equal(res.scores[valid].view(np.int64), scores[valid].view(np.int64))
    # with a prior: (15, 15) r = 15 reaches cells 0, 1, 4, all neighbours of each other -> in one scene the best of the three alone,
    # with cell 4 in another scene it and the better of cells 0, 1
    near = world["loc"].localize(hints, top_k=K, prior_xy=(15, 15), prior_radius=15)
    res = world["loc"].localize(hints, top_k=K, prior_xy=(15, 15), prior_radius=15, distinct_radius=RADIUS)
    _check_states(res, K, two.cell_ids)
    assert near.n_valid.tolist() == [3] * 6 and res.n_valid.tolist() == [1] * 6 and not res.exhausted.any()
    assert np.array_equal(res.cell_rows[:, 0], near.cell_rows[:, 0]) and set(res.cell_rows[:, 0].tolist()) <= {0, 1, 4}
    for f in FIELDS + ("matched", "scores"):
        assert np.array_equal(getattr(res, f)[:, 0], getattr(near, f)[:, 0]), f
    res = loc.localize(hints, top_k=K, prior_xy=(15, 15), prior_radius=15, distinct_radius=RADIUS)
    _check_states(res, K, two.cell_ids)
    assert res.n_valid.tolist() == [2] * 6 and all(4 in r[:2] and (0 in r[:2]) != (1 in r[:2]) for r in res.cell_rows.tolist())
    # scenes "a" = cells 0..3 in a row: at 31 m cells 0 and 2, or 0 and 3, or 1 and 3 - two candidates, never a masked one
    res = loc.localize(hints, top_k=K, prior_xy=(15, 15), prior_radius=np.inf, scenes="a", distinct_radius=RADIUS)
    assert res.n_valid.tolist() == [2] * 6 and (res.cell_rows[:, :2] < 4).all() and (np.abs(np.diff(res.cell_rows[:, :2], axis=1)) >= 2).all()


def test_a_pool_too_small_is_reported(world):
    import text2pos_amd as t2p
    w, loc, db = world, world["loc"], world["db"]
    res = loc.localize(w["hints"], top_k=K, distinct_radius=np.inf, distinct_pool=K)       # 4 of 9 cells ranked, one place among them
    valid = _check_states(res, K, db.cell_ids)
    assert res.n_valid.tolist() == [1] * 7 and res.exhausted.tolist() == [True] * 7 and valid.sum() == 7
    line = res.to_json(2)
    assert json.dumps(line, allow_nan=False) and line["exhausted"] is True and line["n_valid"] == 1 and len(line["world_xy"]) == 1
    for pool in (K, 5, 9):
        res = loc.localize(w["hints"], top_k=K, distinct_radius=RADIUS, distinct_pool=pool)
        valid = _check_states(res, K, db.cell_ids)
        idx, scores, n_valid, exhausted = (t.cpu().numpy() for t in t2p.retrieve_topk_distinct(db.coarse, w["text"], K, db.cell_centers(),
                                                                                            RADIUS, pool=pool))
        assert np.array_equal(res.n_valid, n_valid) and np.array_equal(res.exhausted, exhausted != 0)
        assert np.array_equal(res.cell_rows[valid], idx[valid])
        assert np.array_equal(res.exhausted, res.n_valid < K) if pool < 9 else not res.exhausted.any()
    for kw, word in ((dict(distinct_radius=-1.0), "distinct_radius"), (dict(distinct_radius=float("nan")), "distinct_radius"),
                     (dict(distinct_radius="far"), "distinct_radius"), (dict(distinct_radius=[30.0, 30.0]), "distinct_radius"),
                     (dict(distinct_radius=30.0, distinct_pool=K - 1), r"distinct_pool=3 outside \[top_k, min\(len\(db\), 1024\)\] = \[4, 9\]"),
                     (dict(distinct_radius=30.0, distinct_pool=10), "distinct_pool=10 outside"),
                     (dict(distinct_pool=9), "distinct_pool needs distinct_radius")):
        with pytest.raises(ValueError, match=word):
            loc.localize(w["hints"], top_k=K, **kw)


def test_query_command_with_distinct(world, tmp_path, capsys):
    """`localize query --distinct 31 [--distinct_pool N]` prints Localizer.localize's lines with n_valid and exhausted."""
    import weights as W
    import text2pos_amd as t2p
    from text2pos_amd import data as D, io as IO, localize as LZ, pipeline as PL
    from text2pos_amd.scene import DeviceScene
    w = world
    base = str(tmp_path / "k360")
    IO.save_scene(base, "toy1", w["cells"], w["poses"])
    scenes = IO.load_scenes(base, ["toy1"])
    words, classes = scenes.get_known_words(), scenes.get_known_classes()
    coarse = t2p.CellRetrievalNetwork(classes, D.COLOR_NAMES, words, PL._model_args(256))
    fine = t2p.SuperGlueMatch(classes, D.COLOR_NAMES, words, PL._model_args(128, num_layers=2))
    W.fill_state_dict(coarse, 11)
    W.fill_state_dict(fine, 14)
    coarse, fine = coarse.to(_dev()), fine.to(_dev())
    tf = PL.PerCellTransform(256, SEED)
    _calibrate(coarse, fine, DeviceScene(scenes.all_cells, _dev(), n_pad=PAD, pad_seed=SEED), tf, w["hints"], n_pts=256)
    pc, pf, out = str(tmp_path / "coarse.pth"), str(tmp_path / "fine.pth"), str(tmp_path / "db.pt")
    torch.save(coarse.state_dict(), pc)
    torch.save(fine.state_dict(), pf)
    common = ["--path_coarse", pc, "--path_fine", pf, "--fine_num_layers", "2"]
    LZ.main(["build", "--base_path", base, "--scenes", "toy1", "--out", out, "--pad_size", str(PAD), "--seed", str(SEED)] + common)
    capsys.readouterr()
    loc = LZ.Localizer(coarse, fine, LZ.CellDatabase.load(out, _dev()))
    queries = [w["hints"][0], w["hints"][1]]
    for flags, kw in ((["--distinct", "31"], dict(distinct_radius=31.0)),
                      (["--distinct", "inf", "--distinct_pool", str(K)], dict(distinct_radius=np.inf, distinct_pool=K))):
        LZ.main(["query", "--db", out, "--hints", *queries[0], "--top_k", str(K)] + flags + common)
        text = capsys.readouterr().out
        assert "NaN" not in text and "Infinity" not in text
        lines = [json.loads(s) for s in text.strip().splitlines() if s.startswith("{")]
        want = loc.localize(queries[:1], top_k=K, **kw)
        assert len(lines) == 1 and lines[0] == json.loads(json.dumps(want.to_json(0), allow_nan=False))
        assert lines[0]["n_valid"] == int(want.n_valid[0]) == len(lines[0]["cell_ids"]) and lines[0]["exhausted"] is bool(want.exhausted[0])
    assert lines[0]["n_valid"] == 1 and lines[0]["exhausted"] is True               # one place among the four ranked cells
    with pytest.raises(SystemExit):
        LZ.main(["query", "--db", out, "--hints", *queries[0], "--distinct_pool", "9"] + common)
    with pytest.raises(ValueError, match="distinct_pool=99 outside"):
        LZ.main(["query", "--db", out, "--hints", *queries[0], "--top_k", str(K), "--distinct", "31", "--distinct_pool", "99"] + common)
