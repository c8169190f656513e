"""Localizer.localize with a prior (-m gpu): a position and a radius, a scene, or both restrict the ranking itself
(t2p_sim_topk_prior).  On the 9-cell toy world of tests/test_gpu_localize.py - disjoint 30 m squares at (30 (i % 4), 30 (i // 4)) - with
k = 4: the number of valid candidates per prior, the result against the composition of encode_text, retrieve_topk with the prior,
match_indexed and localize_poses, the invalid columns, the recomputed best, scenes, the memory knob, the unrestricted call and the
command.  The host side (argument checks, post-processing on hand-made arrays) is tests/test_prior_topk_host.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localize_ref as LR  # noqa: E402
from fine_scene import make_fine_scene  # noqa: E402

pytestmark = pytest.mark.gpu
PAD, N_PTS, SEED, HINTS, K = 6, 64, 5, 6, 4
#          prior          radius  n_valid
PRIORS = [((15.0, 15.0), 0.0, 1),                      # inside cell 0 alone
          ((15.0, 15.0), 15.0, 3),                     # cells 0, 1, 4: the edge distance is exactly 15; the diagonal cell 5 at 450 > 225 is out
          ((-100.0, -100.0), 10.0, 0),
          ((500.0, -3.0), np.inf, 4)]


def _dev():
    return torch.device("cuda:0")


def _fresh_models(vocab, n_pts=N_PTS, coarse_args=None):
    """The two models of tests/test_gpu_localize.py: deterministic weights, a match head that peaks."""
    import weights as W
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    from text2pos_amd.pipeline import _model_args
    coarse = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], coarse_args or S.default_args(pointnet_numpoints=n_pts))
    W.fill_state_dict(coarse, 11)
    fa = _model_args(128, num_layers=2)
    fa.pointnet_numpoints = n_pts
    fine = t2p.SuperGlueMatch(vocab["classes"], vocab["colors"], vocab["words"], fa)
    W.fill_state_dict(fine, 14)
    with torch.no_grad():
        fine.superglue.final_proj.weight.mul_(4.0)
        fine.superglue.final_proj.bias.mul_(4.0)
    return coarse.to(_dev()), fine.to(_dev())


def _calibrate(coarse, fine, scene, tf, hints, n_pts=N_PTS):
    """BatchNorm statistics that match the data (one train-mode pass, cumulative averaging): distinct embeddings."""
    for model in (coarse, fine):
        bns = [m for m in (model if model is coarse else model.object_encoder).modules() if isinstance(m, torch.nn.BatchNorm1d)]
        for m in bns:
            m.reset_running_stats()
            m.momentum = None
        model.train()
        with torch.no_grad():
            if model is coarse:
                packed, cp, _ = scene.pack_cells(tf, 0, scene.n_cells)
                model.encode_objects_packed(*packed, cp)
            else:
                ids = scene.padded_object_ids(PAD)
                keys = tf.keys(np.arange(scene.n_cells)[:, None], np.arange(PAD)[None, :])
                packed = scene.pack(ids.reshape(-1), keys.reshape(-1), n_pts)
                model.forward_packed(*packed, np.arange(scene.n_cells + 1, dtype=np.int32) * PAD,
                                     [hints[i % len(hints)] for i in range(scene.n_cells)])
        model.eval()
        for m in bns:
            m.momentum = 0.1


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
    assert np.array_equal(db.cell_boxes().cpu().numpy(), np.array([[30.0 * (i % 4), 30.0 * (i // 4), 30.0 * (i % 4) + 30, 30.0 * (i // 4) + 30]
                                                                   for i in range(9)]))
    return dict(cells=cells, poses=poses, hints=hints, coarse=coarse, fine=fine, db=db, loc=LZ.Localizer(coarse, fine, db))


def _composed(w, hints, k, xy, radius, cell_groups=None, query_groups=None):
    """encode_text + retrieve_topk with the prior + match_indexed + localize_poses, read back entry by entry."""
    import text2pos_amd as t2p
    from text2pos_amd import ops
    from text2pos_amd.superglue_matcher import MATCH_THRESHOLD
    db, mc, mf = w["db"], w["coarse"], w["fine"]
    nq = len(hints)
    groups = {} if cell_groups is None else dict(cell_groups=cell_groups, query_groups=query_groups)
    with torch.no_grad():
        rows, scores = t2p.retrieve_topk(db.coarse, mc.encode_text([" ".join(h) for h in hints]), k, cell_boxes=db.cell_boxes(),
                                         query_xy=np.asarray(xy, dtype=np.float64), query_radius=np.asarray(radius, dtype=np.float64), **groups)
        obj_row = rows.reshape(-1).to(torch.int32)
        hint_row = torch.arange(nq, dtype=torch.int32, device=rows.device).repeat_interleave(k)
        out = ops.match_indexed(db.fine, mf.encode_hints(hints).contiguous(), obj_row, hint_row, mf._match_pack(), mf.sinkhorn_iters, MATCH_THRESHOLD)
    rows_h = rows.cpu().numpy()
    m0, off = out["matches0"].cpu().numpy(), out["offsets"].cpu().numpy()
    want = LR.poses(m0, off, rows_h.reshape(-1).astype(np.int32), nq, k, db.center_xy.cpu().numpy(), db.bbox_xy.cpu().numpy(),
                    db.cell_size.cpu().numpy())
    cxy = db.center_xy.cpu().numpy()[rows_h.reshape(-1)]
    a = LR.magnitude(cxy, off)
    return dict(rows=rows_h, scores=scores.cpu().numpy(), want=want, pos_bound=LR.pos_bound(PAD, a),
                world_bound=LR.world_bound(PAD, a, float(db.bbox_xy.abs().max()), 30.0))


def _check_restricted(res, comp, k, ids):
    """res (a restricted Localization) against the composition on the valid columns, and the stated values on the others."""
    valid = comp["scores"] > -np.inf
    n_valid = valid.sum(axis=1)
    nq = len(n_valid)
    assert res.restricted and res.n_valid.dtype == np.int32 and np.array_equal(res.n_valid, n_valid)
    assert np.array_equal(valid, np.arange(k)[None, :] < n_valid[:, None])                         # the valid columns come first
    assert np.array_equal(res.cell_rows[valid], comp["rows"][valid]) and (res.cell_rows[~valid] == -1).all()
    assert np.array_equal(res.scores[valid].view(np.int64), comp["scores"][valid].view(np.int64)) and np.isneginf(res.scores[~valid]).all()
    assert res.cell_ids == [[ids[j] if ok else None for j, ok in zip(r, v)] for r, v in zip(comp["rows"], valid)]
    want = comp["want"]
    assert np.array_equal(res.matched[valid], want["matched"][valid]) and (res.matched[~valid] == 0).all()
    for name, ref, bound in (("pos_in_cell_mean", "pos_mean", comp["pos_bound"]), ("pos_in_cell", "pos_offset", comp["pos_bound"]),
                             ("world_xy_mean", "world_mean", comp["world_bound"]), ("world_xy", "world_offset", comp["world_bound"])):
        got = getattr(res, name)
        assert got.shape == (nq, k, 2) and np.isnan(got[~valid]).all() and np.isfinite(got[valid]).all(), name
        if valid.any():
            assert np.abs(got[valid] - want[ref][valid]).max() <= bound, name
    best = np.where(n_valid > 0, np.argmax(np.where(valid, want["matched"], -1), axis=1), -1)
    assert res.best.dtype == np.int32 and np.array_equal(res.best, best)
    full = n_valid == k
    assert np.array_equal(res.best[full], want["best"][full])                                    # all columns valid: the device's value
    has = n_valid > 0
    assert np.array_equal(res.best_world_xy[has], res.world_xy[has, res.best[has]]) and np.isnan(res.best_world_xy[~has]).all()


def test_priors_against_the_composition(world):
    w, loc = world, world["loc"]
    # every prior with every pose's hints: 7 x 4 queries, the priors cycling fastest
    hints = [h for h in w["hints"] for _ in PRIORS]
    xy = np.array([p[0] for _ in w["hints"] for p in PRIORS])
    radius = np.array([p[1] for _ in w["hints"] for p in PRIORS])
    res = loc.localize(hints, top_k=K, prior_xy=xy, prior_radius=radius)
    assert res.n_valid.reshape(len(w["hints"]), len(PRIORS)).tolist() == [[p[2] for p in PRIORS]] * len(w["hints"])    # 1, 3, 0, 4 occur
    comp = _composed(w, hints, K, xy, radius)
    _check_restricted(res, comp, K, w["db"].cell_ids)
    print("n_valid:", res.n_valid.tolist(), "\nmatched:\n", res.matched, "\nbest:", res.best.tolist())
    assert (res.matched > 0).any(), "the comparison needs matched objects"
    assert set(res.cell_rows[1::4][:, :3].reshape(-1).tolist()) == {0, 1, 4} and (res.cell_rows[0::4, 0] == 0).all()
    # the device's best sits on a masked column somewhere: the host recomputation is what the result holds
    dev_best = comp["want"]["best"]
    print("device best:", dev_best.tolist())
    # one prior for all, scalars; localize_poses passes them through; the memory knob and mixed hint counts change nothing
    one = loc.localize(w["hints"], top_k=K, prior_xy=(15, 15), prior_radius=15)
    assert one.n_valid.tolist() == [3] * 7
    for f in ("cell_rows", "scores", "matched", "best", "world_xy", "n_valid"):
        assert np.array_equal(getattr(one, f), getattr(res, f)[1::4], equal_nan=True), f
    same = lambda a, b: all((np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) if isinstance(getattr(a, f), np.ndarray)
                             else getattr(a, f) == getattr(b, f)) for f in list(vars(a)))
    assert same(loc.localize_poses(w["poses"], top_k=K, prior_xy=(15, 15), prior_radius=15), one)
    assert same(loc.localize(hints, top_k=K, queries_per_call=3, prior_xy=xy, prior_radius=radius), res)
    mixed = [hints[0][:3], hints[1], hints[2][:2], hints[3], hints[5]]
    sel = [0, 1, 2, 3, 5]
    both = loc.localize(mixed, top_k=K, prior_xy=xy[sel], prior_radius=radius[sel])
    parts = [loc.localize([mixed[i]], top_k=K, prior_xy=xy[sel[i]], prior_radius=radius[sel[i]]) for i in range(5)]
    for f in vars(both):
        x = getattr(both, f)
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, np.concatenate([getattr(p, f) for p in parts]), equal_nan=True), f
    assert both.n_valid.tolist() == [1, 3, 0, 4, 3] and both.cell_ids == [p.cell_ids[0] for p in parts]


def test_scenes(world):
    from text2pos_amd import localize as LZ
    w, db = world, world["db"]
    names = ["a"] * 4 + ["b"] * 5
    two = LZ.CellDatabase(db.coarse, db.fine, db.center_xy, db.bbox_xy, db.cell_size, db.cell_ids, names, db.meta)   # the plain constructor
    assert two.scene_index()[0] == ["a", "b"] and two.scene_index()[1].tolist() == [0] * 4 + [1] * 5
    loc = LZ.Localizer(w["coarse"], w["fine"], two)
    hints = w["hints"][:6]
    scenes = ["a", "b", None, "a", None, "b"]
    res = loc.localize(hints, top_k=K, scenes=scenes)
    assert res.restricted and res.n_valid.tolist() == [4] * 6
    for q, s in enumerate(scenes):
        assert s is None or all(names[j] == s for j in res.cell_rows[q]), (q, s)
    plain = loc.localize(hints, top_k=K)
    assert np.array_equal(res.cell_rows[[2, 4]], plain.cell_rows[[2, 4]]) and np.array_equal(res.scores[[2, 4]], plain.scores[[2, 4]])
    assert {names[j] for j in plain.cell_rows.reshape(-1)} == {"a", "b"}, "the unrestricted ranking should mix the scenes"
    two_w = dict(w, db=two)
    qg = np.array([-1 if s is None else "ab".index(s) for s in scenes], np.int32)
    cg = two.scene_index()[1]
    comp = _composed(two_w, hints, K, np.zeros((6, 2)), np.full(6, np.inf), cg, qg)
    _check_restricted(res, comp, K, two.cell_ids)
    # a scene and a prior together: scene "a" is cells 0..3 (the first row), the prior reaches cells 0, 1, 4 -> cells 0 and 1
    res = loc.localize(hints, top_k=K, prior_xy=(15, 15), prior_radius=15, scenes="a")
    assert res.n_valid.tolist() == [2] * 6 and all(sorted(r[:2].tolist()) == [0, 1] for r in res.cell_rows)
    _check_restricted(res, _composed(two_w, hints, K, np.tile([15.0, 15.0], (6, 1)), np.full(6, 15.0), cg, np.zeros(6, np.int32)), K, two.cell_ids)
    assert loc.localize(hints, top_k=K, scenes="a").n_valid.tolist() == [4] * 6                  # scene "a" has exactly four cells
    with pytest.raises(ValueError, match=r"unknown scene 'toy1'.*\['a', 'b'\]"):
        loc.localize(hints, top_k=K, scenes="toy1")
    # the tables follow the database when it grows
    from text2pos_amd.pipeline import PerCellTransform
    small = LZ.CellDatabase.build(w["coarse"], w["fine"], w["cells"][:5], PerCellTransform(N_PTS, SEED), PAD)
    grow = LZ.Localizer(w["coarse"], w["fine"], small)
    assert grow.localize(hints[:2], top_k=K, prior_xy=(45, 15), prior_radius=0).n_valid.tolist() == [1, 1]          # cell 1 alone
    assert tuple(grow.prior_tables()[0].shape) == (5, 4)
    small.extend(w["coarse"], w["fine"], w["cells"][5:])
    again = grow.localize(hints[:2], top_k=K, prior_xy=(75, 45), prior_radius=0)
    assert tuple(grow.prior_tables()[0].shape) == (9, 4) and again.n_valid.tolist() == [1, 1] and (again.cell_rows[:, 0] == 6).all()


def test_an_unrestricted_call_is_todays(world):
    """Without any of the three arguments: the unrestricted kernels, today's fields, n_valid = K.  With an all-allowing prior: the
    same rows, score bits and positions through the restricted path."""
    from text2pos_amd import localize as LZ, ops
    w, loc = world, world["loc"]
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        res = loc.localize(w["hints"], top_k=K)
    finally:
        ops.profile_enable(False)
    assert {"sim_partial", "topk_merge"} <= set(ops.profile_report())
    assert not res.restricted and res.n_valid.tolist() == [K] * 7 and res.n_valid.dtype == np.int32
    assert set(res.to_json(0)) == set(LZ._RESULT_FIELDS)
    # field by field against the chain the call has always been (tests/test_gpu_localize.py holds it to the models' forward)
    import text2pos_amd as t2p
    from text2pos_amd.superglue_matcher import MATCH_THRESHOLD
    db, mc, mf = w["db"], w["coarse"], w["fine"]
    with torch.no_grad():
        rows, scores = t2p.retrieve_topk(db.coarse, mc.encode_text([" ".join(h) for h in w["hints"]]), K)
        obj_row = rows.reshape(-1).to(torch.int32)
        hint_row = torch.arange(7, dtype=torch.int32, device=rows.device).repeat_interleave(K)
        out = ops.match_indexed(db.fine, mf.encode_hints(w["hints"]).contiguous(), obj_row, hint_row, mf._match_pack(), mf.sinkhorn_iters, MATCH_THRESHOLD)
        pose = ops.localize_poses(out["matches0"], out["offsets"], obj_row, 7, K, db.center_xy, db.bbox_xy, db.cell_size)
    host = lambda t: t.cpu().numpy()
    assert np.array_equal(res.cell_rows, host(rows)) and np.array_equal(res.scores.view(np.int64), host(scores).view(np.int64))
    for f, name in (("pos_in_cell_mean", "pos_mean"), ("pos_in_cell", "pos_offset"), ("world_xy_mean", "world_mean"), ("world_xy", "world_offset"),
                    ("matched", "matched"), ("best", "best")):
        assert np.array_equal(getattr(res, f), host(pose[name])), f
    assert res.cell_ids == [[db.cell_ids[j] for j in r] for r in host(rows)]
    assert np.array_equal(res.best_world_xy, res.world_xy[np.arange(7), res.best])
    wide = loc.localize(w["hints"], top_k=K, prior_xy=(0, 0), prior_radius=np.inf)
    assert wide.restricted and wide.n_valid.tolist() == [K] * 7
    for f in LZ._RESULT_FIELDS:
        x, y = getattr(wide, f), getattr(res, f)
        assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), f
    assert json.dumps(wide.to_json(3), allow_nan=False) and set(wide.to_json(3)) == set(LZ._RESULT_FIELDS) | {"n_valid"}


def test_query_command_with_a_prior(world, tmp_path, capsys):
    """`localize query --prior 15 15 --radius 15 --scene toy1` prints Localizer.localize's restricted lines."""
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
    qfile = tmp_path / "queries.txt"
    qfile.write_text(" | ".join(w["hints"][1]) + "\n")
    LZ.main(["query", "--db", out, "--hints", *w["hints"][0], "--queries_file", str(qfile), "--top_k", str(K), "--prior", "15", "15",
             "--radius", "15", "--scene", "toy1"] + common)
    text = capsys.readouterr().out
    assert "NaN" not in text and "Infinity" not in text
    lines = [json.loads(s) for s in text.strip().splitlines() if s.startswith("{")]
    want = LZ.Localizer(coarse, fine, LZ.CellDatabase.load(out, _dev())).localize([w["hints"][0], w["hints"][1]], top_k=K, prior_xy=(15, 15),
                                                                                  prior_radius=15, scenes="toy1")
    assert len(lines) == 2 and want.n_valid.tolist() == [3, 3]
    for q, line in enumerate(lines):
        assert line == json.loads(json.dumps(want.to_json(q), allow_nan=False))
        assert line["n_valid"] == 3 and len(line["cell_ids"]) == 3 and len(line["world_xy"]) == 3 and len(line["best_world_xy"]) == 2
    LZ.main(["query", "--db", out, "--hints", *w["hints"][0], "--top_k", str(K), "--prior", "-100", "-100", "--radius", "10"] + common)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["n_valid"] == 0 and line["best"] is None and line["best_world_xy"] is None and line["cell_ids"] == []
    with pytest.raises(ValueError, match="unknown scene 'elsewhere'"):
        LZ.main(["query", "--db", out, "--hints", *w["hints"][0], "--top_k", str(K), "--scene", "elsewhere"] + common)
