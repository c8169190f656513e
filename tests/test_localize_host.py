"""Host side of the serving path (no GPU): the C ABI of t2p_match_indexed / t2p_localize_poses (declaration, binding, refusals that
need no device), the float64 reference tests/localize_ref.py against exact rational arithmetic and against the package's two host
implementations of get_pos_in_cell, localize.CellDatabase as a container (round trips, refusals) and Localizer.localize's argument
checks and grouping.  The GPU side is tests/test_gpu_localize.py."""
import ctypes as C
import os
import sys
import zipfile
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localize_ref as LR  # noqa: E402

NEW = ("t2p_match_indexed_workspace_bytes", "t2p_match_indexed", "t2p_localize_poses")


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_built():
    import importlib
    from text2pos_amd import _lib
    build = importlib.import_module("text2pos-cvpr2022_amd.build")
    assert "localize.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "localize.hip"))
    assert _lib.ABI_VERSION == _lib.lib().t2p_abi_version()
    assert all(name in _lib.SYMBOLS and hasattr(_lib.lib(), name) for name in NEW)   # (signatures: tests/test_abi_host.py)


def test_refusals_before_any_launch():
    """Every argument check of the two launchers sits in front of the first HIP call: they answer without a device."""
    from text2pos_amd import _lib
    lib = _lib.lib()
    one = C.c_void_p(256)           # (a non-NULL, 16-byte aligned stand-in: refused calls never dereference it)
    w = _lib.MatchWeights()

    def match(n_cells=5, n_queries=3, batch=2, m=16, n=6, d=128, obj=one, ws_bytes=1 << 30):
        return lib.t2p_match_indexed(obj, n_cells, one, n_queries, one, one, batch, m, n, d, C.byref(w), 50, 0.2, one, one, one, one, one,
                                     one, one, ws_bytes, None)
    assert match(obj=C.c_void_p(0)) == -1 and b"NULL" in lib.t2p_last_error()
    assert match(m=64) == -1 and match(n=0) == -1 and b"63" in lib.t2p_last_error()
    assert match(d=96) == -3
    assert match(n_cells=0) == -1 and match(n_queries=2 ** 30) == -1
    assert match(obj=C.c_void_p(260)) == -1 and b"aligned" in lib.t2p_last_error()
    assert match(batch=-1) == -1
    assert match(batch=0) == 0                                                   # nothing to do, nothing launched
    assert match(ws_bytes=1024) == -2 and b"workspace" in lib.t2p_last_error()
    a = lib.t2p_match_indexed_workspace_bytes(12, 16, 6, 128)
    assert a == lib.t2p_match_workspace_bytes(12, 16, 6, 128) + 12 * 16 * 128 * 4 + 12 * 6 * 128 * 4     # (both multiples of 256)
    assert lib.t2p_match_indexed_workspace_bytes(0, 16, 6, 128) == 256

    def poses(q=2, k=4, m=16, n=6, n_cells=5, first=one):
        return lib.t2p_localize_poses(first, one, one, q, k, m, n, one, one, one, n_cells, one, one, one, one, one, one, None)
    assert poses(first=C.c_void_p(0)) == -1 and b"NULL" in lib.t2p_last_error()
    assert poses(k=0) == -1 and poses(k=1025) == -1 and b"1024" in lib.t2p_last_error()
    assert poses(m=64) == -1 and poses(n=0) == -1
    assert poses(n_cells=0) == -1 and poses(q=-1) == -1
    assert poses(q=0) == 0


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _case(seed, q, k, m, n, n_cells, world=True):
    rng = np.random.default_rng(seed)
    m0 = rng.integers(-1, n, size=(q * k, m)).astype(np.int64)
    m0[0] = -1                                                                   # nothing matched
    if q * k > 1:
        m0[1] = rng.integers(0, n, size=m)                                       # every slot matched
    off = rng.uniform(-0.5, 0.5, size=(q * k, n, 2)).astype(np.float32)
    row = rng.integers(0, n_cells, size=q * k).astype(np.int32)
    center = rng.uniform(-0.3, 1.4, size=(n_cells, m, 2))
    bbox = rng.uniform(0, 3000.0, size=(n_cells, 2)) if world else np.zeros((n_cells, 2))
    size = np.full(n_cells, 30.0) + rng.integers(0, 3, size=n_cells)
    return m0, off, row, center, bbox, size


@pytest.mark.parametrize("q,k,m,n", [(2, 3, 5, 4), (1, 1, 1, 1), (2, 2, 16, 6), (1, 2, 63, 63)])
def test_reference_is_exact_to_its_bound(q, k, m, n):
    m0, off, row, center, bbox, size = _case(7 + m, q, k, m, n, 4)
    got = LR.poses(m0, off, row, q, k, center, bbox, size)
    want = LR.poses_exact(m0, off, row, q, k, center, bbox, size)
    a = LR.magnitude(center, off)
    pb = LR.pos_bound(m, a, sides=1)
    wb = LR.world_bound(m, a, float(np.abs(bbox).max()), float(np.abs(size).max()), sides=1)
    assert 0 < pb < 1e-13 and pb < wb < 1e-11
    worst = {}
    for name, bound in (("pos_mean", pb), ("pos_offset", pb), ("world_mean", wb), ("world_offset", wb)):
        err = max(abs(Fraction(float(got[name][i, c, d])) - want[name][i, c, d]) for i in range(q) for c in range(k) for d in range(2))
        worst[name] = float(err)
        assert err <= Fraction(bound), (name, float(err), bound)
    print(worst, pb, wb)
    assert (got["pos_mean"][0, 0] == 0.5).all() and (got["pos_offset"][0, 0] == 0.5).all() and got["matched"][0, 0] == 0
    if q * k > 1:
        assert got["matched"].reshape(-1)[1] == m
    assert np.array_equal(got["matched"].reshape(-1), (m0 >= 0).sum(axis=1))
    assert np.array_equal(got["best"], np.argmax(got["matched"], axis=1))


def test_reference_agrees_with_the_package():
    from text2pos_amd.evaluation import _sample_hits, positions_in_cell
    from text2pos_amd.superglue_matcher import get_pos_in_cell
    q, k, m, n = 3, 4, 6, 5
    m0, off, row, center, bbox, size = _case(3, q, k, m, n, 7)
    got = LR.poses(m0, off, row, q, k, center, bbox, size)
    bound = LR.pos_bound(m, LR.magnitude(center, off))
    cxy = center[row]
    assert np.abs(positions_in_cell(cxy, m0, off).reshape(q, k, 2) - got["pos_offset"]).max() <= bound
    assert np.abs(positions_in_cell(cxy, m0, np.zeros_like(off)).reshape(q, k, 2) - got["pos_mean"]).max() <= bound

    class Obj:
        def __init__(self, c):
            self.c = c

        def get_center(self):
            return np.array([self.c[0], self.c[1], 0.0])
    for s in range(q * k):
        want = get_pos_in_cell([Obj(c) for c in cxy[s]], m0[s], off[s])
        assert np.abs(want - got["pos_offset"].reshape(-1, 2)[s]).max() <= bound
    # the world step is _sample_hits' statement
    assert np.array_equal(got["world_offset"], bbox[row].reshape(q, k, 2) + got["pos_offset"] * size[row].reshape(q, k)[..., None])
    pose_xy = got["world_offset"][:, 0, :]
    hits = _sample_hits(pose_xy, ["a"] * q, bbox[row].reshape(q, k, 2), size[row].reshape(q, k), [["a"] * k] * q, got["pos_offset"], [k], [0.0])
    assert hits[k][0.0] == 1.0


def test_reference_marks_bad_samples():
    q, k, m, n = 2, 3, 4, 3
    m0, off, row, center, bbox, size = _case(5, q, k, m, n, 4)
    clean = LR.poses(m0, off, row, q, k, center, bbox, size)
    for what in ("row", "row_neg", "m0", "m0_low", "nan"):
        a, b, r = m0.copy(), off.copy(), row.copy()
        if what == "row":
            r[4] = 4
        elif what == "row_neg":
            r[4] = -1
        elif what == "m0":
            a[4, 2] = n
        elif what == "m0_low":
            a[4, 2] = -2
        else:
            b[4, 1, 0] = np.nan
        got = LR.poses(a, b, r, q, k, center, bbox, size)
        assert got["matched"][1, 1] == -1 and np.isnan(got["pos_offset"][1, 1]).all() and np.isnan(got["world_mean"][1, 1]).all()
        keep = np.ones((q, k), bool)
        keep[1, 1] = False
        for name in ("pos_mean", "pos_offset", "world_mean", "world_offset", "matched"):
            assert np.array_equal(got[name][keep], clean[name][keep]), (what, name)
        assert got["best"][0] == clean["best"][0] and got["best"][1] != 1
    allbad = LR.poses(m0, off, np.full_like(row, 9), q, k, center, bbox, size)
    assert (allbad["best"] == -1).all() and (allbad["matched"] == -1).all()
    # ties: the first candidate
    tie = np.full((k, m), -1, dtype=np.int64)
    tie[1, :2] = 0
    tie[2, :2] = 1
    assert LR.poses(tie, off[:k], row[:k], 1, k, center, bbox, size)["best"][0] == 1


# ---- CellDatabase -------------------------------------------------------------------------------------------------------------------
def _cpu_models(vocab, seed=14, d_fine=128):
    import weights as W
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    from text2pos_amd.pipeline import _model_args
    coarse = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args()).eval()
    fine = t2p.SuperGlueMatch(vocab["classes"], vocab["colors"], vocab["words"], _model_args(d_fine, num_layers=1)).eval()
    W.fill_state_dict(coarse, 11)
    W.fill_state_dict(fine, seed)
    return coarse, fine


def _cpu_db(coarse, fine, n=7, pad=6, seed=0):
    from text2pos_amd import localize as LZ
    g = torch.Generator().manual_seed(seed)
    meta = dict(format=LZ.FORMAT, seed=5, n_pts=64, pad_size=pad, **LZ.model_meta(coarse, fine))
    return LZ.CellDatabase(torch.randn(n, coarse.embed_dim, generator=g), torch.randn(n, pad, fine.embed_dim, generator=g),
                           torch.rand(n, pad, 2, generator=g, dtype=torch.float64), torch.rand(n, 2, generator=g, dtype=torch.float64) * 100,
                           torch.full((n,), 30.0, dtype=torch.float64), [f"toy1_{i:05d}" for i in range(n)], ["toy1"] * n, meta)


@pytest.fixture(scope="module")
def cpu_models(vocab):
    return _cpu_models(vocab)


def test_database_round_trips(cpu_models, tmp_path):
    import text2pos_amd as t2p
    from text2pos_amd import localize as LZ
    assert t2p.CellDatabase is LZ.CellDatabase and t2p.Localizer is LZ.Localizer
    db = _cpu_db(*cpu_models)
    path = str(tmp_path / "db.pt")
    db.save(path)
    for other in (LZ.CellDatabase.load(path), LZ.CellDatabase.load(path, "cpu").to("cpu"), db.to("cpu")):
        for k in LZ._TENSORS:
            a, b = getattr(db, k), getattr(other, k)
            assert a.dtype == b.dtype and torch.equal(a, b), k
        assert other.cell_ids == db.cell_ids and other.scene_names == db.scene_names and other.meta == db.meta
        assert len(other) == 7
    # no pickled classes: the weights-only loader accepts the file, and its pickle names nothing of this package
    raw = torch.load(path, weights_only=True)
    assert set(raw) == set(LZ._TENSORS) | {"cell_ids", "scene_names", "meta"}
    assert all(type(v) in (str, int, float, list) for v in raw["meta"].values())
    with zipfile.ZipFile(path) as z:
        pkl = [z.read(n) for n in z.namelist() if n.endswith("data.pkl")]
    assert len(pkl) == 1 and b"text2pos" not in pkl[0] and b"localize" not in pkl[0] and b"CellDatabase" not in pkl[0]


def test_database_refusals_name_the_field(cpu_models, vocab):
    from text2pos_amd import localize as LZ
    coarse, fine = cpu_models
    db = _cpu_db(coarse, fine)
    LZ.Localizer(coarse, fine, db)                                                # the matching pair is accepted
    other_c, other_f = _cpu_models(vocab, seed=15)
    with torch.no_grad():
        next(other_c.lin.parameters()).add_(1.0)
    with pytest.raises(ValueError, match="hash_fine"):
        LZ.Localizer(coarse, other_f, db)
    with pytest.raises(ValueError, match="hash_coarse"):
        LZ.Localizer(other_c, fine, db)
    _, fine64 = _cpu_models(vocab, d_fine=64)
    with pytest.raises(ValueError, match="dim_fine"):
        LZ.Localizer(coarse, fine64, db)
    fp32 = _cpu_models(vocab)[1]
    fp32.precision = "fp32"
    with pytest.raises(ValueError, match="precision_fine"):
        LZ.Localizer(coarse, fp32, db)
    with pytest.raises(ValueError, match="pad_size"):
        LZ.CellDatabase(db.coarse, db.fine, db.center_xy, db.bbox_xy, db.cell_size, db.cell_ids, db.scene_names, dict(db.meta, pad_size=5))
    with pytest.raises(ValueError, match="coarse"):
        LZ.CellDatabase(db.coarse[:, :100], db.fine, db.center_xy, db.bbox_xy, db.cell_size, db.cell_ids, db.scene_names, db.meta)
    with pytest.raises(ValueError, match="center_xy"):
        LZ.CellDatabase(db.coarse, db.fine, db.center_xy.float(), db.bbox_xy, db.cell_size, db.cell_ids, db.scene_names, db.meta)
    with pytest.raises(ValueError, match="cell_ids repeat"):
        LZ.CellDatabase(db.coarse, db.fine, db.center_xy, db.bbox_xy, db.cell_size, [db.cell_ids[0]] * 7, db.scene_names, db.meta)

    class Cell:
        def __init__(self, i):
            self.id, self.scene_name = i, "toy1"
    with pytest.raises(ValueError, match="cell_ids repeat.*toy1_00003"):
        db.extend(coarse, fine, [Cell("toy1_00099"), Cell("toy1_00003")])
    with pytest.raises(ValueError, match="cell_ids repeat.*toy1_00099"):
        db.extend(coarse, fine, [Cell("toy1_00099"), Cell("toy1_00099")])
    with pytest.raises(ValueError, match="hash_fine"):
        db.extend(coarse, other_f, [Cell("toy1_00099")])
    assert db.extend(coarse, fine, []) is db and len(db) == 7
    coarse.train()
    try:
        with pytest.raises(NotImplementedError, match="train"):
            LZ.Localizer(coarse, fine, db)
    finally:
        coarse.eval()
    with pytest.raises(TypeError, match="PerCellTransform"):
        from text2pos_amd.pipeline import default_transform
        LZ.CellDatabase.build(coarse, fine, [Cell("a")], default_transform(64, 0))


# ---- Localizer.localize -------------------------------------------------------------------------------------------------------------
def test_localize_argument_checks_precede_any_launch(cpu_models, monkeypatch):
    from text2pos_amd import localize as LZ
    coarse, fine = cpu_models
    loc = LZ.Localizer(coarse, fine, _cpu_db(coarse, fine))
    monkeypatch.setattr(LZ.Localizer, "_run_chunk", lambda *a, **k: pytest.fail("a launch"))
    h = ["The pose is north of a gray road."]
    with pytest.raises(ValueError, match="query 1 has 0 hints"):
        loc.localize([h, []])
    with pytest.raises(ValueError, match="has 64 hints"):
        loc.localize([h * 64])
    with pytest.raises(TypeError):
        loc.localize([h[0]])
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="1024"):
            loc.localize([h], top_k=bad)
    with pytest.raises(ValueError, match="exceeds the 7 cells"):
        loc.localize([h], top_k=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loc.localize([h], top_k=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loc.localize([h * 63], top_k=7)


def test_grouping_returns_the_callers_order(cpu_models, monkeypatch):
    """A stand-in for the device calls: a query's packed row is a function of its own hints alone, so any mix-up of the order shows."""
    from text2pos_amd import localize as LZ
    coarse, fine = cpu_models
    loc = LZ.Localizer(coarse, fine, _cpu_db(coarse, fine))
    k, calls = 3, []

    def tag(h):
        return float(sum(len(s) * (i + 1) for i, s in enumerate(h)))

    def fake_chunk(self, hints, top_k):
        assert len({len(h) for h in hints}) == 1 and top_k == k
        calls.append(len(hints))
        out = torch.zeros((len(hints), 11 * k + 1), dtype=torch.float64)
        for i, h in enumerate(hints):
            out[i, :k] = torch.tensor([len(h) % 7, (len(h) + 1) % 7, (len(h) + 2) % 7], dtype=torch.float64)
            out[i, k: 10 * k] = tag(h) + torch.arange(9 * k, dtype=torch.float64)
            out[i, 10 * k: 11 * k] = torch.tensor([1.0, 2.0, 0.0])
            out[i, 11 * k] = 1.0
        return out
    monkeypatch.setattr(LZ.Localizer, "_run_chunk", fake_chunk)
    monkeypatch.setattr(LZ.Localizer, "_require_device", lambda self: None)
    lens = [3, 6, 1, 6, 3, 3, 63, 6, 3]
    hints = [[f"hint {q} {j} " + "x" * q for j in range(n)] for q, n in enumerate(lens)]
    assert LZ.group_by_hint_count(hints) == {1: [2], 3: [0, 4, 5, 8], 6: [1, 3, 7], 63: [6]}
    res = loc.localize(hints, top_k=k, queries_per_call=3)
    assert calls == [1, 3, 1, 3, 1]                                               # groups in ascending hint count, 3 queries a call
    for q, h in enumerate(hints):
        assert res.scores[q, 0] == tag(h) and res.scores[q, 2] == tag(h) + 2
        assert res.pos_in_cell_mean[q, 0, 0] == tag(h) + k and res.pos_in_cell[q, 0, 0] == tag(h) + 3 * k
        assert res.world_xy_mean[q, 1, 1] == tag(h) + 5 * k + 3 and res.world_xy[q, 2, 1] == tag(h) + 7 * k + 5
        assert res.cell_rows[q].tolist() == [len(h) % 7, (len(h) + 1) % 7, (len(h) + 2) % 7]
        assert res.cell_ids[q] == [f"toy1_{j:05d}" for j in res.cell_rows[q]]
        assert res.matched[q].tolist() == [1, 2, 0] and res.best[q] == 1 and np.array_equal(res.best_world_xy[q], res.world_xy[q, 1])
    assert res.cell_rows.dtype == np.int64 and res.matched.dtype == np.int32 and res.best.dtype == np.int32
    assert set(res.to_json(0)) == set(LZ._RESULT_FIELDS)
    assert LZ.read_queries(["a ", " b"], None) == [["a", "b"]]
    # a marked sample becomes an IndexError naming the caller's query and the candidate
    def marked(self, hints, top_k):
        out = fake_chunk(self, hints, top_k)
        for i, h in enumerate(hints):
            if len(h) == 63:
                out[i, 10 * k + 2] = -1.0
        return out
    monkeypatch.setattr(LZ.Localizer, "_run_chunk", marked)
    with pytest.raises(IndexError, match="query 6, candidate 2"):
        loc.localize(hints, top_k=k)
