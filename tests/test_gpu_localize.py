"""GPU side of the serving path (-m gpu): t2p_match_indexed against t2p_match on index_select'ed inputs (bit for bit),
t2p_localize_poses against tests/localize_ref.py within the bound derived there, localize.CellDatabase.build / extend against the
entry points they chain, and Localizer.localize against the straightforward composition of encode_text, retrieve_topk, forward_packed
and evaluation.positions_in_cell.  Small shapes throughout; the host side is tests/test_localize_host.py."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_rescale as GR  # noqa: E402
import localize_ref as LR  # noqa: E402
from fine_scene import make_fine_scene  # noqa: E402

pytestmark = pytest.mark.gpu
PAD, N_PTS, SEED, HINTS = 6, 64, 5, 6


def _dev():
    return torch.device("cuda:0")


# ---- t2p_match_indexed --------------------------------------------------------------------------------------------------------------
_MATCHERS = {}


def _matcher(vocab, d, precision):
    """A SuperGlueMatch of two layer pairs at embed_dim d with deterministic weights (only its matcher half is used here)."""
    import weights as W
    import text2pos_amd as t2p
    from text2pos_amd.pipeline import _model_args
    if (d, precision) not in _MATCHERS:
        m = t2p.SuperGlueMatch(vocab["classes"], vocab["colors"], vocab["words"], _model_args(d, num_layers=2), precision=precision)
        W.fill_state_dict(m, 14)
        with torch.no_grad():
            m.superglue.final_proj.weight.mul_(4.0)          # scores that peak: some objects match, some do not
            m.superglue.final_proj.bias.mul_(4.0)
        _MATCHERS[(d, precision)] = m.to(_dev()).eval()
    return _MATCHERS[(d, precision)]


def _tables(seed, n_cells, m, n_queries, n, d):
    g = torch.Generator().manual_seed(seed)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, generator=g), dim=-1).to(_dev()).contiguous()
    return unit(n_cells, m, d), unit(n_queries, n, d)


KEYS = ("P", "matches0", "matches1", "matching_scores0", "matching_scores1", "offsets")
# (n_cells, M, n_queries, N, D, obj_row, hint_row)
INDEXED = {
    "repeated, out of order": (5, 16, 3, 6, 128, [4, 0, 0, 3, 1, 4, 2, 2, 0, 4, 1, 3], [2, 2, 0, 1, 0, 1, 2, 0, 0, 1, 1, 2]),
    "one token each": (2, 1, 2, 1, 64, [1, 0, 1], [0, 0, 1]),
    "63 x 63": (2, 63, 2, 63, 64, [1, 0], [0, 1]),
    "63 x 1": (2, 63, 2, 1, 64, [1, 0], [0, 1]),
    "1 x 63": (2, 1, 2, 63, 64, [1, 1], [1, 0]),
    "51 x 51": (2, 51, 2, 51, 64, [0, 1], [1, 1]),
    "D = 256": (4, 16, 2, 6, 256, [3, 0, 2], [1, 0, 1]),
}


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("case", list(INDEXED))
def test_match_indexed_is_match_on_gathered_inputs(vocab, case, precision):
    """Whatever t2p_match gives on the index_select'ed tables - its outputs, or its refusal where a sample's attention rows pass the
    LDS it may use (63 + 63 tokens need 220 KiB at any D) - t2p_match_indexed gives, bit for bit."""
    from text2pos_amd import _lib, ops
    n_cells, m, n_queries, n, d, obj_row, hint_row = INDEXED[case]
    model = _matcher(vocab, d, precision)
    obj, hint = _tables(len(case), n_cells, m, n_queries, n, d)
    ro, rh = (torch.tensor(r, dtype=torch.int32, device=_dev()) for r in (obj_row, hint_row))
    w = model._match_pack()
    try:
        want = ops.match(obj.index_select(0, ro.long()).contiguous(), hint.index_select(0, rh.long()).contiguous(), w, 50, 0.2)
    except _lib.T2PError as e:
        assert case == "63 x 63" and "rc=-3" in str(e) and "LDS" in str(e)
        with pytest.raises(_lib.T2PError, match=r"rc=-3.*LDS"):
            ops.match_indexed(obj, hint, ro, rh, w, 50, 0.2)
        return
    got = ops.match_indexed(obj, hint, ro, rh, w, 50, 0.2)
    torch.cuda.synchronize()
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert torch.isfinite(got["P"]).all()
    if case == "repeated, out of order":
        assert bool((got["matches0"] >= 0).any()) and bool((got["matches0"] < 0).any())
        assert torch.equal(got["P"][2], got["P"][8]) and torch.equal(got["P"][5], got["P"][9])         # (0, 0) and (4, 1) come twice
        assert not torch.equal(got["P"][1], got["P"][2])                                               # (0, 2) is another sample


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_match_indexed_empty_batch_and_bad_rows(vocab, precision):
    from text2pos_amd import ops
    n_cells, m, n_queries, n, d, obj_row, hint_row = INDEXED["repeated, out of order"]
    model = _matcher(vocab, d, precision)
    obj, hint = _tables(3, n_cells, m, n_queries, n, d)
    w = model._match_pack()
    none = torch.zeros(0, dtype=torch.int32, device=_dev())
    out = ops.match_indexed(obj, hint, none, none, w, 50, 0.2)
    assert tuple(out["P"].shape) == (0, m + 1, n + 1) and tuple(out["matches0"].shape) == (0, m) and tuple(out["offsets"].shape) == (0, n, 2)
    ro, rh = (torch.tensor(r, dtype=torch.int32, device=_dev()) for r in (obj_row, hint_row))
    clean = ops.match_indexed(obj, hint, ro, rh, w, 50, 0.2)
    for victim, (table, value) in {3: ("obj", n_cells), 7: ("obj", -1), 5: ("hint", n_queries), 0: ("hint", -2 ** 31)}.items():
        a, b = ro.clone(), rh.clone()
        (a if table == "obj" else b)[victim] = value
        got = ops.match_indexed(obj, hint, a, b, w, 50, 0.2)
        torch.cuda.synchronize()
        assert torch.isnan(got["P"][victim]).all() and bool((got["matches0"][victim] == -1).all()) and bool((got["matches1"][victim] == -1).all())
        keep = [s for s in range(len(obj_row)) if s != victim]
        for k in KEYS:
            assert torch.equal(got[k][keep], clean[k][keep]), (victim, k)
    with pytest.raises(RuntimeError, match="disagree"):
        ops.match_indexed(obj, hint, ro, rh[:5].contiguous(), w, 50, 0.2)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.match_indexed(obj, hint, ro.long(), rh, w, 50, 0.2)


# ---- t2p_localize_poses -------------------------------------------------------------------------------------------------------------
def _pose_case(seed, q, k, m, n, n_cells=7):
    rng = np.random.default_rng(seed)
    b = q * k
    m0 = rng.integers(-1, n, size=(b, m)).astype(np.int64)
    m0[0] = -1                                                                   # nothing matched
    if b > 1:
        m0[1] = rng.integers(0, n, size=m)                                       # every slot matched
    if k >= 4 and q > 1:                                                         # a tie for the most matched objects: the first wins
        last = (q - 1) * k
        m0[last: last + k] = -1
        m0[last + 1, : min(2, m)] = 0
        m0[last + 3, : min(2, m)] = n - 1
    off = rng.uniform(-0.5, 0.5, size=(b, n, 2)).astype(np.float32)
    row = rng.integers(0, n_cells, size=b).astype(np.int32)
    center = rng.uniform(-0.3, 1.4, size=(n_cells, m, 2))
    bbox = rng.uniform(0, 3000.0, size=(n_cells, 2))
    size = np.full(n_cells, 30.0) + rng.integers(0, 3, size=n_cells)
    return dict(q=q, k=k, m=m, n=n, m0=m0, off=off, row=row, center=center, bbox=bbox, size=size)


def _up(c):
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return {k: to(c[k]) for k in ("m0", "off", "row", "center", "bbox", "size")}


def _poses(c, t=None, check=True):
    from text2pos_amd import ops
    t = t or _up(c)
    out = ops.localize_poses(t["m0"], t["off"], t["row"], c["q"], c["k"], t["center"], t["bbox"], t["size"], check=check)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bounds(c):
    a = LR.magnitude(c["center"], c["off"])
    return LR.pos_bound(c["m"], a), LR.world_bound(c["m"], a, float(np.abs(c["bbox"]).max()), float(np.abs(c["size"]).max()))


POSE_SHAPES = [(3, 4, 16, 6), (2, 1, 5, 4), (2, 1024, 2, 3), (1, 5, 63, 63), (5, 10, 16, 6), (1, 1, 1, 1), (3, 70, 6, 6)]


@pytest.mark.parametrize("shape", POSE_SHAPES)
def test_localize_poses_against_the_reference(shape):
    c = _pose_case(11 + shape[1], *shape)
    want = LR.poses(c["m0"], c["off"], c["row"], c["q"], c["k"], c["center"], c["bbox"], c["size"])
    got = _poses(c)
    pb, wb = _bounds(c)
    for name, bound in (("pos_mean", pb), ("pos_offset", pb), ("world_mean", wb), ("world_offset", wb)):
        assert got[name].shape == (c["q"], c["k"], 2) and got[name].dtype == np.float64
        err = np.abs(got[name] - want[name]).max()
        print(f"{shape} {name}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, name
    assert got["matched"].dtype == np.int32 and np.array_equal(got["matched"], want["matched"])
    assert got["best"].dtype == np.int32 and np.array_equal(got["best"], want["best"])
    assert np.array_equal(got["best"], np.argmax((c["m0"] >= 0).sum(axis=1).reshape(c["q"], c["k"]), axis=1))     # run_fine's statement
    assert (got["pos_mean"][0, 0] == 0.5).all() and (got["pos_offset"][0, 0] == 0.5).all() and got["matched"][0, 0] == 0
    if c["q"] * c["k"] > 1:
        assert got["matched"].reshape(-1)[1] == c["m"]
    if c["k"] >= 4 and c["q"] > 1:
        assert got["best"][-1] == 1 and got["matched"][-1, 1] == got["matched"][-1, 3] == min(2, c["m"])
    again = _poses(c)
    assert all(np.array_equal(again[k], got[k]) for k in got)                                     # call to call: the same bits


def test_outputs_are_overwritten_and_nothing_behind_them():
    from text2pos_amd import _lib
    c = _pose_case(4, 3, 5, 7, 4)
    t = _up(c)
    b, q = c["q"] * c["k"], c["q"]
    f64 = [torch.full((2 * b + 16,), float("nan"), dtype=torch.float64, device=_dev()) for _ in range(4)]
    matched = torch.full((b + 16,), -9, dtype=torch.int32, device=_dev())
    best = torch.full((q + 16,), -9, dtype=torch.int32, device=_dev())
    for x in f64:
        x[2 * b:] = -7.0
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = _lib.lib().t2p_localize_poses(p(t["m0"]), p(t["off"]), p(t["row"]), q, c["k"], c["m"], c["n"], p(t["center"]), p(t["bbox"]),
                                       p(t["size"]), c["center"].shape[0], p(f64[0]), p(f64[1]), p(f64[2]), p(f64[3]), p(matched), p(best),
                                       C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream))
    _lib.check(rc, "t2p_localize_poses")
    torch.cuda.synchronize()
    want = _poses(c)
    for x, name in zip(f64, ("pos_mean", "pos_offset", "world_mean", "world_offset")):
        assert np.array_equal(x[: 2 * b].cpu().numpy().reshape(q, c["k"], 2), want[name]) and bool((x[2 * b:] == -7.0).all()), name
    assert np.array_equal(matched[:b].cpu().numpy().reshape(q, c["k"]), want["matched"]) and bool((matched[b:] == -9).all())
    assert np.array_equal(best[:q].cpu().numpy(), want["best"]) and bool((best[q:] == -9).all())


@pytest.mark.parametrize("what", ["cell_row_high", "cell_row_negative", "matches0_high", "matches0_low", "nan_offset", "nan_offset_unused"])
def test_a_bad_input_marks_the_sample_and_raises(what):
    c = _pose_case(9, 3, 4, 16, 6)
    good = _poses(c)
    victim = (1, 2)
    s = victim[0] * c["k"] + victim[1]
    c["m0"][s, 4] = 2                                                                      # (hint 2 is in use, hint 5 is not)
    c["m0"][s][c["m0"][s] == 5] = -1
    good = _poses(c)
    if what == "cell_row_high":
        c["row"][s] = c["center"].shape[0]
    elif what == "cell_row_negative":
        c["row"][s] = -1
    elif what == "matches0_high":
        c["m0"][s, 3] = c["n"]
    elif what == "matches0_low":
        c["m0"][s, 3] = -2
    elif what == "nan_offset":
        c["off"][s, 2, 1] = np.nan
    else:
        c["off"][s, 5, 0] = np.nan
    got = _poses(c, check=False)
    want = LR.poses(c["m0"], c["off"], c["row"], c["q"], c["k"], c["center"], c["bbox"], c["size"])
    keep = np.ones((c["q"], c["k"]), bool)
    keep[victim] = False
    for name in ("pos_mean", "pos_offset", "world_mean", "world_offset"):
        assert np.isnan(got[name][victim]).all(), name
        assert np.array_equal(got[name][keep], good[name][keep]), name                         # the other samples are untouched
    assert got["matched"][victim] == -1 and np.array_equal(got["matched"][keep], good["matched"][keep])
    assert np.array_equal(got["best"], want["best"]) and got["best"][victim[0]] != victim[1]
    with pytest.raises(IndexError, match="query 1, candidate 2"):
        _poses(c)


def test_a_query_without_a_good_sample_has_no_best():
    c = _pose_case(2, 2, 3, 5, 4)
    c["row"][3:] = 99
    got = _poses(c, check=False)
    assert got["best"][1] == -1 and (got["matched"][1] == -1).all() and got["best"][0] >= 0 and (got["matched"][0] >= 0).all()


def test_localize_poses_wrapper_refusals():
    from text2pos_amd import ops
    c = _pose_case(1, 2, 3, 5, 4)
    t = _up(c)
    with pytest.raises(RuntimeError, match="do not describe"):
        ops.localize_poses(t["m0"], t["off"], t["row"], 3, 3, t["center"], t["bbox"], t["size"])
    with pytest.raises(RuntimeError, match="tables"):
        ops.localize_poses(t["m0"], t["off"], t["row"], 2, 3, t["center"][:, :4].contiguous(), t["bbox"], t["size"])
    with pytest.raises(RuntimeError, match="dtype"):
        ops.localize_poses(t["m0"], t["off"], t["row"], 2, 3, t["center"].float(), t["bbox"], t["size"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.localize_poses(t["m0"].cpu(), t["off"], t["row"], 2, 3, t["center"], t["bbox"], t["size"])


# ---- the database and the localizer -------------------------------------------------------------------------------------------------
def _fresh_models(vocab, fine_seed=14):
    import weights as W
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    from text2pos_amd.pipeline import _model_args
    coarse = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(pointnet_numpoints=N_PTS))
    W.fill_state_dict(coarse, 11)
    fa = _model_args(128, num_layers=2)
    fa.pointnet_numpoints = N_PTS
    fine = t2p.SuperGlueMatch(vocab["classes"], vocab["colors"], vocab["words"], fa)
    W.fill_state_dict(fine, fine_seed)
    with torch.no_grad():
        fine.superglue.final_proj.weight.mul_(4.0)
        fine.superglue.final_proj.bias.mul_(4.0)
    return coarse.to(_dev()), fine.to(_dev())


def _calibrate(coarse, fine, scene, tf, hints, n_pts=N_PTS):
    """Random-init weights with BatchNorm statistics that match the data (one train-mode pass over the scene's cells, cumulative
    averaging in the object encoders): distinct embeddings, as a trained checkpoint has."""
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
    from text2pos_amd import evaluation as E, io as IO, pipeline as PL
    from text2pos_amd.scene import DeviceScene
    cells, poses = make_fine_scene(9, 7, 41, PAD, HINTS)
    tf = PL.PerCellTransform(N_PTS, SEED)
    scene = DeviceScene(cells, _dev(), n_pad=PAD, pad_seed=SEED)
    hints = [E.create_hint_description(p) for p in poses]
    coarse, fine = _fresh_models(vocab)
    _calibrate(coarse, fine, scene, tf, hints)
    return dict(cells=cells, poses=poses, tf=tf, scene=scene, hints=hints, coarse=coarse, fine=fine, scenes=IO.Scenes(cells, poses))


@pytest.fixture(scope="module")
def database(world):
    from text2pos_amd import localize as LZ
    w = world
    return LZ.CellDatabase.build(w["coarse"], w["fine"], w["cells"], w["tf"], PAD)


def _same(a, b):
    from text2pos_amd import localize as LZ
    return (all(torch.equal(getattr(a, k), getattr(b, k)) for k in LZ._TENSORS) and a.cell_ids == b.cell_ids
            and a.scene_names == b.scene_names and a.meta == b.meta)


def test_database_build(world, database):
    from text2pos_amd import localize as LZ
    w, db = world, database
    assert len(db) == 9 and tuple(db.fine.shape) == (9, PAD, 128) and tuple(db.coarse.shape) == (9, 256) and db.coarse.is_cuda
    assert db.meta["pad_size"] == PAD and db.meta["seed"] == SEED and db.meta["n_pts"] == N_PTS
    assert db.meta["precision_fine"] == "f16x3" and len(db.meta["hash_fine"]) == 64
    for per_call in (1, 4, 9):
        assert _same(LZ.CellDatabase.build(w["coarse"], w["fine"], w["cells"], w["tf"], PAD, cells_per_call=per_call), db), per_call
    # the coarse rows are encode_scene_cells', the fine tokens forward_packed's object encodings of samples packed with the per-cell keys
    sc = w["scene"]
    with torch.no_grad():
        assert torch.equal(db.coarse, w["coarse"].encode_scene_cells(sc, w["tf"], 0, 9))
        ids = sc.padded_object_ids(PAD)
        pick = np.array([7, 2, 2, 8, 0])
        keys = w["tf"].keys(pick[:, None], np.arange(PAD)[None, :])
        packed = sc.pack(ids[pick].reshape(-1), keys.reshape(-1), N_PTS)
        out = w["fine"].forward_packed(*packed, np.arange(len(pick) + 1, dtype=np.int32) * PAD, [w["hints"][0]] * len(pick))
    assert torch.equal(out.object_encodings, db.fine[torch.from_numpy(pick).to(_dev())])
    assert torch.isfinite(db.fine).all() and (db.fine.norm(dim=-1) - 1).abs().max().item() < 1e-5
    cos = (db.coarse @ db.coarse.T).cpu().numpy()[np.triu_indices(9, 1)]
    assert cos.max() < 0.999, "calibrated embeddings should be spread out"
    # the geometry
    assert np.array_equal(db.center_xy.cpu().numpy(), sc.center64[ids][:, :, 0:2])
    assert np.array_equal(db.bbox_xy.cpu().numpy(), np.array([c.bbox_w[0:2] for c in w["cells"]])) and bool((db.cell_size == 30.0).all())
    assert db.cell_ids == [c.id for c in w["cells"]] and db.scene_names == ["toy1"] * 9
    # extend over the last 4 cells equals the fresh build
    part = LZ.CellDatabase.build(w["coarse"], w["fine"], w["cells"][:5], w["tf"], PAD)
    assert len(part) == 5 and part.extend(w["coarse"], w["fine"], w["cells"][5:], cells_per_call=3) is part
    assert _same(part, db)
    with pytest.raises(ValueError, match="cell_ids repeat"):
        part.extend(w["coarse"], w["fine"], w["cells"][8:])


def _composed(w, db, hints, k):
    """The straightforward composition: encode_text + retrieve_topk, then forward_packed on samples packed from the scene with the
    database's per-cell keys, evaluation.positions_in_cell on host copies."""
    import text2pos_amd as t2p
    from text2pos_amd import evaluation as E
    sc = w["scene"]
    with torch.no_grad():
        rows, scores = t2p.retrieve_topk(db.coarse, w["coarse"].encode_text([" ".join(h) for h in hints]), k)
        rows_h = rows.cpu().numpy()
        ids = sc.padded_object_ids(PAD)[rows_h.reshape(-1)]
        keys = w["tf"].keys(rows_h.reshape(-1)[:, None], np.arange(PAD)[None, :])
        packed = sc.pack(ids.reshape(-1), keys.reshape(-1), N_PTS)
        hint_enc = w["fine"].encode_hints(hints).repeat_interleave(k, dim=0)
        out = w["fine"].forward_packed(*packed, np.arange(len(ids) + 1, dtype=np.int32) * PAD, hint_enc)
    m0, off = out.matches0.cpu().numpy(), out.offsets.cpu().numpy()
    cxy = sc.center64[ids][:, :, 0:2]
    nq = len(hints)
    conf = (m0 >= 0).sum(axis=1).reshape(nq, k)
    return dict(rows=rows_h, scores=scores.cpu().numpy(), m0=m0, off=off, cxy=cxy, conf=conf, best=np.argmax(conf, axis=1),
                pos_mean=E.positions_in_cell(cxy, m0, np.zeros_like(off)).reshape(nq, k, 2),
                pos_off=E.positions_in_cell(cxy, m0, off).reshape(nq, k, 2))


def _equal_results(a, b):
    from text2pos_amd import localize as LZ
    for f in LZ._RESULT_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), f


def test_localize_end_to_end(world, database, tmp_path):
    from text2pos_amd import evaluation as E, localize as LZ
    w, db, k = world, database, 4
    loc = LZ.Localizer(w["coarse"], w["fine"], db)
    res = loc.localize(w["hints"], top_k=k)
    want = _composed(w, db, w["hints"], k)
    assert np.array_equal(res.cell_rows, want["rows"]) and np.array_equal(res.scores.view(np.int64), want["scores"].view(np.int64))
    assert res.cell_ids == [[db.cell_ids[j] for j in r] for r in want["rows"]]
    assert np.array_equal(res.matched, want["conf"]) and np.array_equal(res.best, want["best"])
    print("matched per candidate:\n", res.matched)
    assert (res.matched > 0).any() and (want["m0"] < 0).any(), "the comparison needs matched and unmatched objects"
    bound = LR.pos_bound(PAD, LR.magnitude(want["cxy"], want["off"]))
    wbound = LR.world_bound(PAD, LR.magnitude(want["cxy"], want["off"]), float(db.bbox_xy.abs().max()), 30.0)
    e_mean, e_off = np.abs(res.pos_in_cell_mean - want["pos_mean"]).max(), np.abs(res.pos_in_cell - want["pos_off"]).max()
    print(f"pos_in_cell_mean {e_mean:.3e}, pos_in_cell {e_off:.3e} (bound {bound:.3e})")
    assert e_mean <= bound and e_off <= bound
    bbox, size = db.bbox_xy.cpu().numpy()[want["rows"]], db.cell_size.cpu().numpy()[want["rows"]]
    assert np.abs(res.world_xy - (bbox + want["pos_off"] * size[..., None])).max() <= wbound
    assert np.abs(res.world_xy_mean - (bbox + want["pos_mean"] * size[..., None])).max() <= wbound
    assert np.array_equal(res.best_world_xy, res.world_xy[np.arange(len(w["hints"])), res.best])
    # queries with 3, 6 and 6 hints in one call equal the per-group calls
    mixed = [w["hints"][0][:3], w["hints"][1], w["hints"][2]]
    both, short, full = loc.localize(mixed, top_k=k), loc.localize(mixed[:1], top_k=k), loc.localize(mixed[1:], top_k=k)
    for f in LZ._RESULT_FIELDS:
        x = getattr(both, f)
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, np.concatenate([getattr(short, f), getattr(full, f)])), f
        else:
            assert x == getattr(short, f) + getattr(full, f), f
    _equal_results(loc.localize(w["hints"], top_k=k, queries_per_call=2), res)              # the memory knob changes nothing
    _equal_results(loc.localize_poses(w["poses"], top_k=k), res)
    # save, load: identical results
    path = str(tmp_path / "db.pt")
    db.save(path)
    again = LZ.CellDatabase.load(path, _dev())
    assert _same(again, db)
    _equal_results(LZ.Localizer(w["coarse"], w["fine"], again).localize(w["hints"], top_k=k), res)
    # the accuracy table from pos_in_cell is the composed path's
    retr = res.cell_ids
    tables = [E.localisation_accuracies(w["poses"], retr, w["scenes"].cells_dict, [1, 2, 4], [5, 10, 15], p)
              for p in (res.pos_in_cell, want["pos_off"])]
    assert tables[0] == tables[1]
    with pytest.raises(ValueError, match="exceeds the 9 cells"):
        loc.localize(w["hints"], top_k=10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        LZ.Localizer(w["coarse"], w["fine"], db.to("cpu")).localize(w["hints"], top_k=k)


def test_refusals_on_the_device(world, database, vocab):
    from text2pos_amd import localize as LZ
    w, db = world, database
    other_c, other_f = _fresh_models(vocab, fine_seed=15)
    with pytest.raises(ValueError, match="hash_fine"):
        LZ.Localizer(w["coarse"], other_f.eval(), db)
    fine = w["fine"]
    fine.train()
    try:
        with pytest.raises(NotImplementedError, match="train"):
            LZ.Localizer(w["coarse"], fine, db)
        with pytest.raises(NotImplementedError, match="eval"):
            with torch.no_grad():
                fine.encode_cell_objects(w["scene"], w["tf"], 0, 2, PAD)
        with pytest.raises(NotImplementedError, match="eval"):
            LZ.CellDatabase.build(w["coarse"], fine, w["cells"], w["tf"], PAD)
    finally:
        fine.eval()
    loc = LZ.Localizer(w["coarse"], fine, db)
    fine.train()
    try:
        with pytest.raises(NotImplementedError, match="train"):
            loc.localize(w["hints"][:1], top_k=2)
    finally:
        fine.eval()
    # an f16x3 guard hit during build: the PointNet++ features of the fine model's object encoder pushed past fp16's range by an
    # exact rescaling (tests/guard_rescale.py, row "f1": lin1 times s, lin2 divided by s - the same function)
    hot = copy.deepcopy(fine)
    sd = fine.state_dict()
    s = 2.0 ** np.floor(np.log2(32768.0 / float(sd[GR.P + "lin1.weight"].abs().max())))
    hot.load_state_dict(GR.apply(sd, None, "f1", float(s))[0], strict=True)
    with pytest.raises(FloatingPointError, match="fp16's range"):
        LZ.CellDatabase.build(w["coarse"], hot.eval(), w["cells"], w["tf"], PAD)
    assert _same(LZ.CellDatabase.build(w["coarse"], fine, w["cells"], w["tf"], PAD), db)      # the guard word was cleared: the next build is clean


# ---- the command ------------------------------------------------------------------------------------------------------------------
def test_build_and_query_commands(world, tmp_path, capsys):
    """`localize build` then `localize query` on plain state_dict checkpoints: the JSON lines are Localizer.localize's results."""
    import json
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
    db = LZ.main(["build", "--base_path", base, "--scenes", "toy1", "--out", out, "--pad_size", str(PAD), "--seed", str(SEED)] + common)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["cells"] == 9
    fresh = LZ.CellDatabase.build(coarse, fine, scenes.all_cells, tf, PAD)
    assert all(torch.equal(getattr(db, k), getattr(fresh, k)) for k in LZ._TENSORS) and db.cell_ids == fresh.cell_ids
    qfile = tmp_path / "queries.txt"
    qfile.write_text(" | ".join(w["hints"][1]) + "\n\n" + "|".join(w["hints"][2][:3]) + "\n")
    LZ.main(["query", "--db", out, "--hints", *w["hints"][0], "--queries_file", str(qfile), "--top_k", "3"] + common)
    lines = [json.loads(s) for s in capsys.readouterr().out.strip().splitlines() if s.startswith("{")]
    want = LZ.Localizer(coarse, fine, LZ.CellDatabase.load(out, _dev())).localize([w["hints"][0], w["hints"][1], w["hints"][2][:3]], top_k=3)
    assert len(lines) == 3
    for q, line in enumerate(lines):
        assert line == json.loads(json.dumps(want.to_json(q))) and len(line["cell_ids"]) == 3 and len(line["best_world_xy"]) == 2
    with pytest.raises(ValueError, match="1024"):
        LZ.main(["query", "--db", out, "--hints", "x", "--top_k", "0"] + common)
