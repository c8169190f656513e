"""Host side of the prior-restricted retrieval and of Localizer.localize's prior (no GPU needed): the refusals of
t2p_sim_topk_prior (nothing is launched: the pointers are never dereferenced), the argument checks of retrieve_topk and localize, the
host post-processing of a restricted result on a hand-made packed array, and the command line.  The GPU side is
tests/test_gpu_prior_topk.py and tests/test_gpu_localize_prior.py; the yardstick's own proof tests/test_topk_ref_host.py."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def _call(**kw):
    """t2p_sim_topk_prior with plausible (never dereferenced: every case here is refused first) arguments."""
    from text2pos_amd import _lib
    fake = C.c_void_p(1 << 20)          # 16-byte aligned, non-null
    a = dict(queries=fake, cells=fake, query_xy=fake, query_radius=fake, cell_box=fake, query_group=fake, cell_group=fake, nq=4, nc=64,
             dim=256, k=10, index_offset=0, out_idx=fake, out_score=fake, workspace=fake, workspace_bytes=1 << 30, stream=C.c_void_p(0))
    a.update(kw)
    lib = _lib.lib()
    rc = lib.t2p_sim_topk_prior(a["queries"], a["cells"], a["query_xy"], a["query_radius"], a["cell_box"], a["query_group"], a["cell_group"],
                                a["nq"], a["nc"], a["dim"], a["k"], a["index_offset"], a["out_idx"], a["out_score"], a["workspace"],
                                a["workspace_bytes"], a["stream"])
    return rc, (lib.t2p_last_error() or b"").decode()


def _same_refusal_as_sim_topk(**kw):
    """(rc, message) of t2p_sim_topk for the same k / dim / nc / workspace."""
    from text2pos_amd import _lib
    fake = C.c_void_p(1 << 20)
    a = dict(nq=4, nc=64, dim=256, k=10, workspace_bytes=1 << 30)
    a.update(kw)
    lib = _lib.lib()
    rc = lib.t2p_sim_topk(fake, fake, a["nq"], a["nc"], a["dim"], a["k"], 0, fake, fake, fake, a["workspace_bytes"], C.c_void_p(0))
    return rc, (lib.t2p_last_error() or b"").decode()


def test_refusals_launch_nothing():
    from text2pos_amd import _lib
    E_ARG = _lib.DEFINES["T2P_E_ARG"]
    null = C.c_void_p(0)
    geo, grp = ("query_xy", "query_radius", "cell_box"), ("query_group", "cell_group")
    # every partial set of the three geometry pointers (with and without the groups), and of the two group pointers
    for given in range(1, 7):
        missing = {n: null for i, n in enumerate(geo) if not given >> i & 1}
        for extra in ({}, {n: null for n in grp}):
            rc, err = _call(**missing, **extra)
            assert rc == E_ARG and "go together" in err and "cell_box" in err, (missing, extra, err)
    for n in grp:
        for extra in ({}, {g: null for g in geo}):
            rc, err = _call(**{n: null}, **extra)
            assert rc == E_ARG and "query_group and cell_group go together" in err, (n, extra, err)
    rc, err = _call(**{n: null for n in geo + grp})
    assert rc == E_ARG and "t2p_sim_topk" in err and "call" in err                 # both sets NULL: the message names the plain call
    rc, err = _call(cell_box=C.c_void_p((1 << 20) + 8))
    assert rc == E_ARG and "cell_box" in err and "16-byte aligned" in err
    # t2p_sim_topk's own refusals apply, with its return codes - with either set alone as with both
    for bad, text in ((dict(k=0), r"\[1,1024\]"), (dict(k=1025), r"\[1,1024\]"), (dict(dim=96), "dim=96"), (dict(nc=2 ** 31 - 1), "nc too large"),
                      (dict(workspace_bytes=16), "workspace")):
        want = _same_refusal_as_sim_topk(**bad)
        assert want[0] < 0 and re.search(text, want[1]), (bad, want)
        for sets in ({}, {n: null for n in geo}, {n: null for n in grp}):
            got = _call(**bad, **sets)
            assert got == want, (bad, sets, got, want)
    assert _same_refusal_as_sim_topk(workspace_bytes=16)[0] == _lib.DEFINES["T2P_E_WORKSPACE"]
    assert _call(nq=-1)[0] == E_ARG and _call(queries=null)[0] == E_ARG
    assert _call(nq=0)[0] == 0                                                       # nothing to do, nothing launched


def test_the_wrapper_is_there_and_refuses_host_tensors():
    from text2pos_amd import ops
    q, c = torch.zeros(3, 256), torch.zeros(8, 256)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sim_topk_prior(q, c, 2, query_group=torch.zeros(3, dtype=torch.int32), cell_group=torch.zeros(8, dtype=torch.int32))


# ---- retrieve_topk ------------------------------------------------------------------------------------------------------
def test_retrieve_topk_wants_the_three_geometry_arrays_together_and_clean_values():
    import text2pos_amd as t2p
    from text2pos_amd import retrieval as R
    c, q = np.zeros((8, 256), np.float32), np.zeros((3, 256), np.float32)
    box, xy, rad = np.zeros((8, 4)), np.zeros((3, 2)), np.zeros(3)
    for kw, missing in ((dict(cell_boxes=box), "query_xy, query_radius"), (dict(query_xy=xy, query_radius=rad), "cell_boxes"),
                        (dict(cell_boxes=box, query_radius=rad), "query_xy")):
        with pytest.raises(ValueError, match="go together.*missing: " + missing):
            t2p.retrieve_topk(c, q, 2, **kw)
    with pytest.raises(ValueError, match="cell_groups and query_groups go together"):             # the existing refusal, with geometry too
        t2p.retrieve_topk(c, q, 2, cell_boxes=box, query_xy=xy, query_radius=rad, cell_groups=np.zeros(8, np.int32))
    cpu = torch.device("cpu")
    assert R._as_device_f64([[1, 2], [3, 4]], (2, 2), "query_xy", cpu).dtype == torch.float64
    assert R._as_device_f64(torch.ones(3, dtype=torch.float32), (3,), "query_radius", cpu).tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match=r"cell_boxes has shape \(8, 2\), expected \(8, 4\)"):
        R._as_device_f64(np.zeros((8, 2)), (8, 4), "cell_boxes", cpu)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    ok = (t([[0.0, 1.0], [2.0, 3.0]]), t([0.0, float("inf")]), t([[0.0, 0.0, 1.0, float("inf")]]))
    R.check_prior(*ok)
    for xy_, rad_, box_, text in ((t([[0.0, 1.0], [float("inf"), 3.0]]), ok[1], ok[2], r"query_xy\[1\].*not finite"),
                                  (t([[float("nan"), 1.0], [2.0, 3.0]]), ok[1], ok[2], r"query_xy\[0\].*not finite"),
                                  (ok[0], t([0.0, -1.0]), ok[2], r"query_radius\[1\] = -1.0"),
                                  (ok[0], t([float("nan"), 1.0]), ok[2], r"query_radius\[0\] = nan"),
                                  (ok[0], ok[1], t([[0.0, 0.0, 1.0, 1.0], [0.0, float("nan"), 1.0, 1.0]]), r"cell_boxes\[1\].*NaN")):
        with pytest.raises(ValueError, match=text):
            R.check_prior(xy_, rad_, box_)


# ---- localize: the argument checks ----------------------------------------------------------------------------------------
def test_check_prior_reads_every_form_and_names_what_it_refuses():
    from text2pos_amd import localize as LZ
    known = ["a", "b"]
    assert LZ.check_prior(3, None, None, None, known) == (None, None, None)
    xy, rad, grp = LZ.check_prior(3, (1, 2.5), 60, None, known)
    assert xy.dtype == np.float64 and xy.tolist() == [[1.0, 2.5]] * 3 and rad.tolist() == [60.0] * 3 and grp is None
    xy, rad, grp = LZ.check_prior(2, [[1, 2], [3, 4]], [0.0, np.inf], ["b", None], known)
    assert xy.tolist() == [[1.0, 2.0], [3.0, 4.0]] and rad.tolist() == [0.0, np.inf] and grp.dtype == np.int32 and grp.tolist() == [1, -1]
    assert xy.flags.c_contiguous and rad.flags.c_contiguous
    xy, rad, grp = LZ.check_prior(2, None, None, "a", known)
    assert xy is None and rad is None and grp.tolist() == [0, 0]
    assert LZ.check_prior(2, np.zeros((2, 2)), np.float64(3), ("a", "b"), known)[2].tolist() == [0, 1]
    for kw, text in ((dict(prior_xy=(1, 2)), "go together.*only prior_xy"), (dict(prior_radius=5), "go together.*only prior_radius"),
                     (dict(prior_xy=(1, 2, 3), prior_radius=5), "shape"), (dict(prior_xy=[[1, 2]] * 2, prior_radius=5), "shape"),
                     (dict(prior_xy=(1, 2), prior_radius=[5, 5]), "shape"),
                     (dict(prior_xy=(1, np.nan), prior_radius=5), "query 0.*finite"), (dict(prior_xy=[[1, 2], [3, 4], [np.inf, 0]], prior_radius=5), "query 2.*finite"),
                     (dict(prior_xy=(1, 2), prior_radius=-1), r"query 0 is -1.0.*>= 0"), (dict(prior_xy=(1, 2), prior_radius=[1, np.nan, 2]), "query 1 is nan"),
                     (dict(prior_xy="here", prior_radius=5), "numbers"),
                     (dict(scenes="c"), r"unknown scene 'c'.*\['a', 'b'\]"), (dict(scenes=["a", "b"]), "3 entries"),
                     (dict(scenes=["a", 3, None]), "3 entries"), (dict(scenes=7), "one name")):
        args = dict(prior_xy=None, prior_radius=None, scenes=None)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            LZ.check_prior(3, args["prior_xy"], args["prior_radius"], args["scenes"], known)


def _cpu_database(n=7, pad=6):
    """A CellDatabase on the host as a container: 30 m cells on a 4-wide grid, two scenes; meta names models that are never run."""
    from text2pos_amd import localize as LZ
    meta = dict(format=LZ.FORMAT, seed=5, n_pts=64, pad_size=pad, dim_coarse=256, dim_fine=128)
    bbox = torch.tensor([[30.0 * (i % 4), 30.0 * (i // 4)] for i in range(n)], dtype=torch.float64)
    return LZ.CellDatabase(torch.zeros(n, 256), torch.zeros(n, pad, 128), torch.zeros(n, pad, 2, dtype=torch.float64), bbox,
                           torch.full((n,), 30.0, dtype=torch.float64), [f"toy_{i:05d}" for i in range(n)], ["s1"] * 4 + ["s0"] * (n - 4), meta)


def test_cell_boxes_and_scene_index():
    db = _cpu_database()
    boxes = db.cell_boxes()
    assert boxes.dtype == torch.float64 and tuple(boxes.shape) == (7, 4) and boxes.is_contiguous() and boxes.device == db.device
    assert boxes[5].tolist() == [30.0, 30.0, 60.0, 60.0] and torch.equal(boxes[:, :2], db.bbox_xy)
    assert torch.equal(boxes[:, 2], db.bbox_xy[:, 0] + db.cell_size) and torch.equal(boxes[:, 3], db.bbox_xy[:, 1] + db.cell_size)
    names, idx = db.scene_index()
    assert names == ["s0", "s1"] and idx.dtype == torch.int32 and idx.tolist() == [1, 1, 1, 1, 0, 0, 0]


class _Stub:
    """Stands in for a model where only Localizer's bookkeeping runs."""
    training = False
    device = torch.device("cpu")


def _localizer(monkeypatch, db, fake_chunk):
    from text2pos_amd import localize as LZ
    monkeypatch.setattr(LZ, "check_models", lambda *a, **k: None)
    monkeypatch.setattr(LZ.Localizer, "_run_chunk", fake_chunk)
    monkeypatch.setattr(LZ.Localizer, "_require_device", lambda self: None)
    return LZ.Localizer(_Stub(), _Stub(), db)


def test_localize_checks_the_prior_before_anything_runs_and_hands_each_chunk_its_rows(monkeypatch):
    from text2pos_amd import localize as LZ
    k, seen = 2, []

    def fake_chunk(self, hints, top_k, prior=None):
        seen.append((len(hints), prior))
        out = torch.zeros((len(hints), 11 * k + 1), dtype=torch.float64)
        out[:, 1] = 1.0
        return out
    db = _cpu_database()
    loc = _localizer(monkeypatch, db, fake_chunk)
    hints = [["a"], ["b", "c"], ["d"]]
    for kw, text in ((dict(prior_xy=(1, 2)), "go together"), (dict(prior_xy=(1, 2), prior_radius=-2), ">= 0"),
                     (dict(scenes="nowhere"), r"unknown scene 'nowhere'.*\['s0', 's1'\]"), (dict(scenes=["s0"]), "3 entries")):
        with pytest.raises(ValueError, match=text):
            loc.localize(hints, top_k=k, **kw)
    with pytest.raises(ValueError, match="exceeds the 7 cells"):
        loc.localize(hints, top_k=8, prior_xy=(1, 2), prior_radius=3)
    with pytest.raises(TypeError):
        loc.localize(hints, k, None, (1, 2), 3)                                  # keyword-only
    assert seen == []
    # unrestricted: the chunk call of before (two arguments); n_valid is K
    res = loc.localize(hints, top_k=k)
    assert [p for _, p in seen] == [None, None] and res.n_valid.tolist() == [k] * 3 and res.n_valid.dtype == np.int32 and not res.restricted
    assert set(res.to_json(0)) == set(LZ._RESULT_FIELDS)
    # restricted: every chunk gets the prior rows of its own queries, in the chunk's order (queries 0 and 2 have one hint, query 1 two)
    del seen[:]
    loc.localize(hints, top_k=k, prior_xy=[[0, 1], [10, 11], [20, 21]], prior_radius=[1, 2, np.inf], scenes=["s1", None, "s0"])
    (n0, (xy0, r0, g0)), (n1, (xy1, r1, g1)) = seen
    assert (n0, n1) == (2, 1)
    assert xy0.tolist() == [[0, 1], [20, 21]] and r0.tolist() == [1, np.inf] and g0.tolist() == [1, 0]
    assert xy1.tolist() == [[10, 11]] and r1.tolist() == [2] and g1.tolist() == [-1]
    del seen[:]
    loc.localize(hints, top_k=k, scenes="s0", queries_per_call=1)
    assert [(n, p[0].tolist(), p[1].tolist(), p[2].tolist()) for n, p in seen] == [(1, [[0.0, 0.0]], [np.inf], [0])] * 3   # a scene alone
    assert all(isinstance(t, torch.Tensor) and t.device == db.device for _, p in seen for t in p)        # uploaded before the chunks run
    # the tables: cached, and computed again after the database grew
    boxes, names, idx = loc.prior_tables()
    assert loc.prior_tables()[0] is boxes and names == ["s0", "s1"] and tuple(boxes.shape) == (7, 4)
    db.cell_ids.append("toy_new")
    db.scene_names.append("s2")
    for name in ("coarse", "fine", "center_xy", "bbox_xy", "cell_size"):
        t = getattr(db, name)
        setattr(db, name, torch.cat([t, t[:1]]))
    boxes2, names2, idx2 = loc.prior_tables()
    assert tuple(boxes2.shape) == (8, 4) and names2 == ["s0", "s1", "s2"] and idx2.tolist()[-1] == 2


# ---- localize: the host post-processing ---------------------------------------------------------------------------------------
def _packed(k, rows, scores, matched, best):
    """One packed row per query: cell rows | scores | four position blocks (distinct finite values) | matched | best."""
    nq = len(rows)
    out = np.zeros((nq, 11 * k + 1))
    out[:, :k], out[:, k: 2 * k] = rows, scores
    out[:, 2 * k: 10 * k] = 100.0 + np.arange(nq)[:, None] * 1000.0 + np.arange(8 * k)[None, :]
    out[:, 10 * k: 11 * k], out[:, 11 * k] = matched, best
    return out


def test_unpack_a_restricted_result():
    from text2pos_amd import localize as LZ
    k, ninf = 4, -np.inf
    ids = [f"c{i}" for i in range(9)]
    #            rows            scores                     matched          device best
    cases = [([5, 2, 7, 0], [0.9, 0.5, 0.1, -0.3], [1, 3, 3, 0], 1),             # all valid: the device's best stands (first on ties)
             ([4, 1, 0, 2], [0.8, 0.2, ninf, ninf], [2, 2, 6, 6], 2),            # the device's best is a masked column: recomputed, tie -> first
             ([0, 1, 2, 3], [ninf] * 4, [5, 0, 0, 0], 0),                        # nothing qualified
             ([8, 0, 1, 2], [-0.7, ninf, ninf, ninf], [0, 4, 4, 4], 1),          # one valid candidate with no matched object is still the best
             ([3, 6, 0, 1], [0.3, 0.2, 0.1, ninf], [0, 1, 2, 9], 3)]
    res_in = _packed(k, *(np.array([c[i] for c in cases], dtype=np.float64) for i in range(4)))
    r = LZ.unpack_result(res_in, k, ids, True)
    assert r.restricted and r.n_valid.dtype == np.int32 and r.n_valid.tolist() == [4, 2, 0, 1, 3]
    assert r.best.dtype == np.int32 and r.best.tolist() == [1, 0, -1, 0, 2]
    assert r.cell_rows.dtype == np.int64 and r.cell_rows.tolist() == [[5, 2, 7, 0], [4, 1, -1, -1], [-1] * 4, [8, -1, -1, -1], [3, 6, 0, -1]]
    assert r.cell_ids == [["c5", "c2", "c7", "c0"], ["c4", "c1", None, None], [None] * 4, ["c8", None, None, None], ["c3", "c6", "c0", None]]
    assert r.matched.dtype == np.int32 and r.matched.tolist() == [[1, 3, 3, 0], [2, 2, 0, 0], [0] * 4, [0, 0, 0, 0], [0, 1, 2, 0]]
    valid = np.arange(k)[None, :] < r.n_valid[:, None]
    assert np.array_equal(np.isneginf(r.scores), ~valid) and np.array_equal(r.scores[valid], res_in[:, k: 2 * k][valid])
    for j, name in enumerate(("pos_in_cell_mean", "pos_in_cell", "world_xy_mean", "world_xy")):
        a = getattr(r, name)
        assert a.shape == (5, k, 2) and np.array_equal(np.isnan(a), np.repeat(~valid[:, :, None], 2, axis=2)), name
        assert np.array_equal(a[valid], res_in[:, (2 + 2 * j) * k: (4 + 2 * j) * k].reshape(5, k, 2)[valid]), name
    assert np.array_equal(r.best_world_xy[[0, 1, 3, 4]], r.world_xy[[0, 1, 3, 4], [1, 0, 0, 2]]) and np.isnan(r.best_world_xy[2]).all()
    # the same array unrestricted: today's reading, n_valid = K, the device's best
    u = LZ.unpack_result(res_in, k, ids, False)
    assert not u.restricted and u.n_valid.tolist() == [k] * 5 and u.best.tolist() == [1, 2, 0, 1, 3] and np.isfinite(u.world_xy).all()
    assert u.cell_rows.tolist() == [c[0] for c in cases] and np.array_equal(u.scores, res_in[:, k: 2 * k])
    assert np.array_equal(u.best_world_xy, u.world_xy[np.arange(5), u.best])
    # a sample the kernels marked still raises, restricted or not
    bad = res_in.copy()
    bad[1, 10 * k + 1] = -1.0
    with pytest.raises(IndexError, match="query 1, candidate 1"):
        LZ.unpack_result(bad, k, ids, True)
    # no queries
    e = LZ.unpack_result(np.zeros((0, 11 * k + 1)), k, ids, True)
    assert e.n_valid.shape == (0,) and e.best_world_xy.shape == (0, 2) and e.cell_ids == []

    # ---- the JSON line: strict, no NaN, the valid prefix ----
    def strict(line):
        return json.loads(line, parse_constant=lambda name: pytest.fail(f"{name} in the JSON line"))
    for q in range(5):
        line = json.dumps(r.to_json(q), allow_nan=False)
        d = strict(line)
        n = int(r.n_valid[q])
        assert set(d) == set(LZ._RESULT_FIELDS) | {"n_valid"} and d["n_valid"] == n
        assert all(len(d[f]) == n for f in LZ._RESULT_FIELDS[:-2])
        assert d["cell_ids"] == [f"c{j}" for j in cases[q][0][:n]] and d["scores"] == cases[q][1][:n]
        if n:
            assert d["best"] == int(r.best[q]) and d["best_world_xy"] == r.world_xy[q, r.best[q]].tolist()
        else:
            assert d["best"] is None and d["best_world_xy"] is None
    d = u.to_json(1)
    assert set(d) == set(LZ._RESULT_FIELDS) and len(d["cell_ids"]) == k                  # the unrestricted line is what it was


# ---- the command line -----------------------------------------------------------------------------------------------------
def test_query_flags_and_read_queries(tmp_path, capsys):
    from text2pos_amd import localize as LZ
    common = ["query", "--db", "db.pt", "--path_coarse", "c.pth", "--path_fine", "f.pth", "--hints", "The pose is north of a gray road."]
    a = LZ.parse_args(common)
    assert a.prior is None and a.radius is None and a.scene is None and a.top_k == 10
    a = LZ.parse_args(common + ["--prior", "1042.5", "-3310", "--radius", "60", "--scene", "2013_05_28_drive_0010_sync", "--top_k", "3"])
    assert a.prior == [1042.5, -3310.0] and a.radius == 60.0 and a.scene == "2013_05_28_drive_0010_sync" and a.top_k == 3
    assert LZ.parse_args(common + ["--scene", "s"]).scene == "s" and LZ.parse_args(common + ["--prior", "0", "0", "--radius", "inf"]).radius == np.inf
    for bad in (["--prior", "1", "2"], ["--radius", "5"], ["--prior", "1", "--radius", "5"], ["--prior", "1", "2", "--radius", "far"]):
        with pytest.raises(SystemExit):
            LZ.parse_args(common + bad)
    assert "go together" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        LZ.parse_args(["build", "--base_path", "b", "--out", "o", "--path_coarse", "c", "--path_fine", "f", "--prior", "1", "2", "--radius", "3"])
    # what the flags become: one prior for every query of the invocation
    qfile = tmp_path / "q.txt"
    qfile.write_text("a | b\n\nc\n")
    queries = LZ.check_hints(LZ.read_queries(["x ", " y"], str(qfile)))
    assert queries == [["x", "y"], ["a", "b"], ["c"]]
    xy, rad, grp = LZ.check_prior(len(queries), a.prior, a.radius, a.scene, ["2013_05_28_drive_0010_sync"])
    assert xy.tolist() == [[1042.5, -3310.0]] * 3 and rad.tolist() == [60.0] * 3 and grp.tolist() == [0, 0, 0]
    assert "--prior" in LZ.__doc__ and "--radius" in LZ.__doc__ and "--scene" in LZ.__doc__    # the module's usage text shows the flags
