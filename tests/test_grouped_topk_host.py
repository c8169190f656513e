"""Host side of the evaluation's oracle switches (no GPU needed): the C ABI of t2p_sim_topk_grouped and its refusals (nothing is
launched, so nothing needs a device), retrieve_topk's group arguments, evaluation.street_groups against a brute-force loop, the
street-centre file format, run_fine_oracle on a hand-made scene, run_coarse's three modes with a stand-in model and a NumPy ranking,
the per-rank slicing of the query groups, and the command line's conflict checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from test_topk_any_host import _StubCoarse, _toy_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_binding_binds_abi_stays_32():
    import text2pos_amd  # noqa: F401
    from text2pos_amd import _lib
    header = open(os.path.join(ROOT, "include", "t2p.h")).read()
    assert len(_lib.SYMBOLS["t2p_sim_topk_grouped"][1]) == 14       # (types and layouts: tests/test_abi_host.py)
    assert "const int32_t* query_group, const int32_t* cell_group," in header
    assert "evaluation/pipeline.py:93-108" in header and "t2p_sim_topk_workspace_bytes(nq, nc, k)" in header
    assert _lib.ABI_VERSION == _lib.lib().t2p_abi_version()
    assert hasattr(_lib.lib(), "t2p_sim_topk_grouped")
    from text2pos_amd import ops
    assert callable(ops.sim_topk_grouped)


def _call(**kw):
    """t2p_sim_topk_grouped with plausible (never dereferenced: every case here is refused first) arguments."""
    import text2pos_amd  # noqa: F401
    from text2pos_amd import _lib
    fake = C.c_void_p(1 << 20)          # 16-byte aligned, non-null
    a = dict(queries=fake, cells=fake, query_group=fake, cell_group=fake, nq=4, nc=64, dim=256, k=10, index_offset=0,
             out_idx=fake, out_score=fake, workspace=fake, workspace_bytes=1 << 30, stream=C.c_void_p(0))
    a.update(kw)
    lib = _lib.lib()
    rc = lib.t2p_sim_topk_grouped(a["queries"], a["cells"], a["query_group"], a["cell_group"], a["nq"], a["nc"], a["dim"], a["k"],
                                  a["index_offset"], a["out_idx"], a["out_score"], a["workspace"], a["workspace_bytes"], a["stream"])
    return rc, (lib.t2p_last_error() or b"").decode()


def test_refusals_launch_nothing():
    null = C.c_void_p(0)
    for bad, text in ((dict(query_group=null), "NULL group"), (dict(cell_group=null), "NULL group"),
                      (dict(k=0), r"\[1,1024\]"), (dict(k=1025), r"\[1,1024\]"), (dict(k=-3), r"\[1,1024\]"),
                      (dict(queries=null), "NULL argument"), (dict(nq=-1), "negative size"), (dict(dim=300), "dim=300")):
        rc, err = _call(**bad)
        assert rc == -1, bad
        assert re.search(text, err), (bad, err)
    # a null group array AND a bad k: still refused; an empty side needs no array; nq == 0 is no error and launches nothing
    assert _call(query_group=null, k=0)[0] == -1
    assert _call(nq=0, query_group=null, queries=null)[0] == 0


def test_retrieve_topk_wants_both_group_arrays_or_neither():
    import text2pos_amd as t2p
    c, q = np.zeros((8, 256), np.float32), np.zeros((3, 256), np.float32)
    with pytest.raises(ValueError, match="go together"):
        t2p.retrieve_topk(c, q, 2, cell_groups=np.zeros(8, np.int32))
    with pytest.raises(ValueError, match="go together"):
        t2p.retrieve_topk(c, q, 2, query_groups=torch.zeros(3, dtype=torch.int32))
    from text2pos_amd import retrieval as R
    cpu = torch.device("cpu")
    assert R._as_device_groups(np.array([5, -2 ** 31, 2 ** 31 - 1], np.int64), 3, "g", cpu).dtype == torch.int32
    assert R._as_device_groups(torch.tensor([1, 2, 3]), 3, "g", cpu).tolist() == [1, 2, 3]
    assert R._as_device_groups(np.array([7, 9], np.uint8), 2, "g", cpu).tolist() == [7, 9]
    for bad in (np.array([0, 2 ** 31], np.int64), np.array([-2 ** 31 - 1, 0], np.int64), np.array([2 ** 40, 0], np.uint64),
                torch.tensor([0, 2 ** 31])):
        with pytest.raises(ValueError, match="outside int32"):
            R._as_device_groups(bad, 2, "g", cpu)
    with pytest.raises(TypeError, match="integers"):
        R._as_device_groups(np.zeros(2, np.float32), 2, "g", cpu)
    with pytest.raises(ValueError, match="shape"):
        R._as_device_groups(np.zeros(3, np.int32), 2, "g", cpu)


# ---- street assignment --------------------------------------------------------------------------------------------------
def _grid_scene(name, n_cells, n_poses, seed, x0=0.0):
    from text2pos_amd import data as D
    rng = np.random.default_rng(seed)
    cells = [D.Cell(i, name, [], 30.0, np.array([x0 + 30.0 * (i % 5), 30.0 * (i // 5), 0.0, x0 + 30.0 * (i % 5) + 30.0, 30.0 * (i // 5) + 30.0, 10.0]))
             for i in range(n_cells)]
    poses = []
    for _ in range(n_poses):
        c = cells[int(rng.integers(0, n_cells))]
        poses.append(D.Pose(rng.random(3), c.bbox_w[0:3] + rng.random(3) * np.array([30.0, 30.0, 10.0]), c.id, name, []))
    return cells, poses


def _brute_force(items_xyz, centers):
    out = []
    for x in items_xyz:
        best, best_d = -1, None
        for s, ctr in enumerate(centers):
            d = float(np.sqrt(sum((float(x[a]) - float(ctr[a])) ** 2 for a in range(3))))
            if best_d is None or d < best_d:          # strict: the first minimum wins
                best, best_d = s, d
        out.append(best)
    return out


def test_street_groups_vs_brute_force_tie_and_two_scenes():
    import text2pos_amd  # noqa: F401
    from text2pos_amd import evaluation as E
    cells, poses = _grid_scene("sceneA", 20, 37, seed=1)
    # cell 0's centre is (15, 15, 5): streets 1 and 2 are equidistant from it (exactly: +-8 in x), street 0 is farther
    centers = np.array([[100.0, 100.0, 5.0], [23.0, 15.0, 5.0], [7.0, 15.0, 5.0], [75.0, 45.0, 5.0]])
    cg, qg = E.street_groups(cells, poses, centers)
    assert cg.dtype == np.int32 and qg.dtype == np.int32 and cg.shape == (20,) and qg.shape == (37,)
    assert cg[0] == 1                                                               # the first of the two minima
    assert cg.tolist() == _brute_force([c.get_center() for c in cells], centers)
    assert qg.tolist() == _brute_force([p.pose_w for p in poses], centers)
    assert len(set(cg.tolist())) >= 3
    # two scenes: an id range per scene, in the dict's order; cells of the other scene never match
    cells_b, poses_b = _grid_scene("sceneB", 10, 12, seed=2, x0=15.0)                # overlaps sceneA's ground
    centers_b = np.array([[30.0, 20.0, 5.0], [120.0, 40.0, 5.0]])
    cg2, qg2 = E.street_groups(cells + cells_b, poses + poses_b, {"sceneA": centers, "sceneB": centers_b})
    assert cg2[:20].tolist() == cg.tolist() and qg2[:37].tolist() == qg.tolist()
    assert cg2[20:].tolist() == [4 + s for s in _brute_force([c.get_center() for c in cells_b], centers_b)]
    assert qg2[37:].tolist() == [4 + s for s in _brute_force([p.pose_w for p in poses_b], centers_b)]
    assert set(cg2[:20].tolist()) <= {0, 1, 2, 3} and set(cg2[20:].tolist()) <= {4, 5}
    assert not (set(qg2[37:].tolist()) & set(cg2[:20].tolist()))
    with pytest.raises(ValueError, match="sceneB"):
        E.street_groups(cells + cells_b, poses, {"sceneA": centers})
    with pytest.raises(ValueError, match=r"\[S, 3\]"):
        E.street_groups(cells, poses, np.zeros((4, 2)))


def test_street_centers_round_trip(tmp_path):
    import text2pos_amd  # noqa: F401
    from text2pos_amd import io as IO
    centers = np.random.default_rng(0).random((11, 3)).astype(np.float32) * 100
    IO.save_street_centers(str(tmp_path), "2013_05_28_drive_0010_sync", centers)
    assert os.path.isfile(os.path.join(str(tmp_path), "street_centers", "2013_05_28_drive_0010_sync.pkl"))
    back = IO.load_street_centers(str(tmp_path), "2013_05_28_drive_0010_sync")
    assert back.dtype == np.float64 and np.array_equal(back, centers.astype(np.float64))
    with pytest.raises(RuntimeError, match=r"\[S, 3\]"):
        IO.save_street_centers(str(tmp_path), "bad", np.zeros((3, 2)))
    with pytest.raises(FileNotFoundError):
        IO.load_street_centers(str(tmp_path), "absent")


# ---- fine oracle --------------------------------------------------------------------------------------------------------
def test_run_fine_oracle_on_three_cells():
    """Cells A (0..30), B (30..60), C (60..90) along x.  Pose 0 lies in A at (10, 20): exact in A, clipped to B's edge (30, 20) -> 20 m,
    to C's edge -> 50 m.  Pose 1 belongs to B but lies 4 m outside it, at (64, 5): the clip leaves a residual of 4 m in B, and C holds
    it exactly."""
    import text2pos_amd  # noqa: F401
    from text2pos_amd import data as D, io as IO, pipeline as PL
    cells = [D.Cell(i, "s", [], 30.0, np.array([30.0 * i, 0.0, 0.0, 30.0 * i + 30.0, 30.0, 10.0])) for i in range(3)]
    a, b, c = (x.id for x in cells)
    poses = [D.Pose(np.zeros(3), np.array([10.0, 20.0, 1.0]), a, "s", []), D.Pose(np.zeros(3), np.array([64.0, 5.0, 1.0]), b, "s", [])]
    sc = IO.Scenes(cells, poses)
    threshs = [3, 5, 25, 60]
    acc = PL.run_fine_oracle([[b, c, a], [b, a, c]], sc, [1, 2, 3], threshs)
    # pose 0: distances 20, 50, 0 -> best 20 / 20 / 0.   pose 1: distances 4, 34 (clipped to (30, 5)), 0 -> best 4 / 4 / 0
    assert acc == {1: {3: 0.0, 5: 0.5, 25: 1.0, 60: 1.0}, 2: {3: 0.0, 5: 0.5, 25: 1.0, 60: 1.0}, 3: {3: 1.0, 5: 1.0, 25: 1.0, 60: 1.0}}
    r1 = PL.run_fine_oracle([[b, c, a], [b, a, c]], sc, [1, 3], threshs, random_oracle=True, seed=5)
    r2 = PL.run_fine_oracle([[b, c, a], [b, a, c]], sc, [1, 3], threshs, random_oracle=True, seed=5)
    assert r1 == r2 and set(r1) == {1, 3} and r1[3][60] == 1.0
    # the random positions are the generator's own stream: [n_cells, 2] per pose, in pose order
    rng = np.random.default_rng(5)
    d0 = np.linalg.norm(np.array([10.0, 20.0]) - (np.array([[30.0, 0.0], [60.0, 0.0], [0.0, 0.0]]) + rng.random((3, 2)) * 30.0), axis=1)
    d1 = np.linalg.norm(np.array([64.0, 5.0]) - (np.array([[30.0, 0.0], [0.0, 0.0], [60.0, 0.0]]) + rng.random((3, 2)) * 30.0), axis=1)
    assert r1[1][25] == np.mean([d0[0] <= 25, d1[0] <= 25]) and r1[3][25] == np.mean([d0.min() <= 25, d1.min() <= 25])
    with pytest.raises(ValueError, match="retrieval lists"):
        PL.run_fine_oracle([[a]], sc, [1], threshs)


# ---- run_coarse's modes -------------------------------------------------------------------------------------------------
def _np_grouped_topk(seen):
    """The injected ranking of the street mode: float64 on the host, called as topk_fn(queries, cells, k, cell_groups, query_groups)."""
    def fn(q, c, k, cell_groups, query_groups):
        seen.append((q.numpy().copy(), c.numpy().copy(), np.array(cell_groups), np.array(query_groups)))
        c64, q64 = c.numpy().astype(np.float64), q.numpy().astype(np.float64)
        idx, sc = np.zeros((len(q64), k), np.int64), np.zeros((len(q64), k))
        for i in range(len(q64)):
            s = np.where(np.asarray(cell_groups) == query_groups[i], c64 @ q64[i], -np.inf)
            idx[i] = np.argsort(-s, kind="stable")[:k]
            sc[i] = s[idx[i]]
        return torch.from_numpy(idx), torch.from_numpy(sc)
    return fn


def test_run_coarse_modes_on_the_cpu():
    import text2pos_amd  # noqa: F401
    from text2pos_amd import evaluation as E, io as IO, pipeline as PL
    cells, poses = _toy_scene()                      # 13 cells on a 4-wide grid of 30 m, 21 poses
    sc = IO.Scenes(cells, poses)
    tf, threshs = PL.PerCellTransform(64, 3), (5, 10, 15)
    ids = [c.id for c in cells]

    # oracle
    model = _StubCoarse()
    with pytest.raises(ValueError, match="must be 1"):
        PL.run_coarse(model, sc, tf, [1, 5], threshs, coarse_mode="oracle")
    retr, acc = PL.run_coarse(None, sc, tf, [1], threshs, coarse_mode="oracle")
    assert retr == [[p.cell_id] for p in poses] and acc["hit"] == {1: 1.0} and set(acc) == {"hit", "close", "localisation"}

    # random
    r1, a1 = PL.run_coarse(None, sc, tf, [1, 5], threshs, coarse_mode="random", seed=11)
    r2, a2 = PL.run_coarse(None, sc, tf, [1, 5], threshs, coarse_mode="random", seed=11)
    r3, _ = PL.run_coarse(None, sc, tf, [1, 5], threshs, coarse_mode="random", seed=12)
    assert r1 == r2 and a1 == a2 and r1 != r3
    assert len(r1) == len(poses) and all(len(r) == 5 and set(r) <= set(ids) for r in r1)
    draws = np.random.default_rng(11).choice(len(cells), size=(len(poses), 5), replace=True)
    assert r1 == [[ids[j] for j in row] for row in draws]
    assert model.calls == 0                           # neither mode encodes anything

    # street
    streets = np.array([[30.0, 45.0, 5.0], [100.0, 30.0, 5.0], [60.0, 100.0, 5.0]])
    cg, qg = E.street_groups(cells, poses, streets)
    assert len(set(cg.tolist())) == 3
    seen = []
    retr, acc = PL.run_coarse(model, sc, tf, [1, 5, 8], threshs, coarse_mode="street", street_centers=streets, topk_fn=_np_grouped_topk(seen))
    assert model.calls > 0 and len(seen) == 1
    q_emb, c_emb, cg_seen, qg_seen = seen[0]
    assert np.array_equal(cg_seen, cg) and np.array_equal(qg_seen, qg) and len(q_emb) == len(poses) and len(c_emb) == len(cells)
    want = []
    for i in range(len(poses)):                       # the restatement: float64 C @ q, masked to -inf, stable descending argsort
        s = c_emb.astype(np.float64) @ q_emb[i].astype(np.float64)
        s[cg != qg[i]] = -np.inf
        want.append([ids[j] for j in np.argsort(-1.0 * s, kind="stable")[:8]])
    assert retr == want and set(acc["hit"]) == {1, 5, 8}
    for i, r in enumerate(retr):                      # own street first, then masked cells in ascending database order
        n_own = int((cg == qg[i]).sum())
        assert all(cg[ids.index(cid)] == qg[i] for cid in r[:min(8, n_own)])
        tail = [ids.index(cid) for cid in r[n_own:]]
        assert tail == sorted(tail) and all(cg[j] != qg[i] for j in tail)
    with pytest.raises(ValueError, match="street_centers"):
        PL.run_coarse(model, sc, tf, [1], threshs, coarse_mode="street")
    with pytest.raises(ValueError, match="coarse_mode"):
        PL.run_coarse(model, sc, tf, [1], threshs, coarse_mode="streets")

    # evaluate: the fine oracle's table under `fine_oracle`, no fine model
    out = PL.evaluate(None, None, sc, tf, top_k=(1,), threshs=threshs, coarse_mode="oracle", fine_mode="oracle")
    assert set(out) >= {"hit", "close", "localisation", "retrievals", "fine_oracle"} and "fine_mean" not in out
    assert out["fine_oracle"] == {1: {5: 1.0, 10: 1.0, 15: 1.0}}     # every pose of this scene lies inside its own cell
    with pytest.raises(ValueError, match="fine_mode"):
        PL.evaluate(None, None, sc, tf, top_k=(1,), coarse_mode="oracle", fine_mode="perfect")


def test_default_mode_is_unchanged_by_the_new_arguments():
    """coarse_mode=None with the three-argument topk_fn of today: same call, same result as before the switches existed."""
    import text2pos_amd  # noqa: F401
    from text2pos_amd import io as IO, pipeline as PL
    from test_topk_any_host import _topk
    cells, poses = _toy_scene()
    sc = IO.Scenes(cells, poses)
    a = PL.run_coarse(_StubCoarse(), sc, PL.PerCellTransform(64, 3), (1, 5), (5, 10, 15), topk_fn=_topk)
    b = PL.run_coarse(_StubCoarse(), sc, PL.PerCellTransform(64, 3), (1, 5), (5, 10, 15), topk_fn=_topk, coarse_mode=None, seed=9)
    assert a == b


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2), (2, 3)])
def test_query_groups_are_sliced_to_the_ranks_block(rank, world):
    import text2pos_amd  # noqa: F401
    from text2pos_amd import distributed as TD, pipeline as PL
    nq = 37
    qg = np.random.default_rng(4).integers(-5, 5, nq).astype(np.int32)
    cg = np.arange(50, dtype=np.int32) % 7
    got = []
    fn = PL.grouped_rank_fn(lambda q, c, k, cell_groups, query_groups: got.append((len(q), k, cell_groups, query_groups)) or "result",
                            cg, qg, rank, world)
    lo, hi = TD.shard_range(nq, rank, world)
    assert fn(torch.zeros(hi - lo, 4), torch.zeros(50, 4), 3) == "result"
    n, k, cg_seen, qg_seen = got[0]
    assert (n, k) == (hi - lo, 3) and np.array_equal(cg_seen, cg) and np.array_equal(qg_seen, qg[lo:hi]) and len(qg_seen) == hi - lo
    blocks = [TD.shard_range(nq, r, world) for r in range(world)]       # the ranks' blocks tile the queries
    assert blocks[0][0] == 0 and blocks[-1][1] == nq and all(blocks[i][1] == blocks[i + 1][0] for i in range(world - 1))


# ---- command line -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,text", [(["--coarse_oracle"], "top_k 1"),                                   # default top_k is 1 5 10
                                        (["--coarse_oracle", "--top_k", "1", "5"], "top_k 1"),
                                        (["--coarse_random", "--coarse_oracle", "--top_k", "1"], "coarse_random"),
                                        (["--coarse_random", "--street_oracle"], "coarse_random"),
                                        (["--fine_random", "--fine_oracle"], "fine_random"),
                                        (["--fine_random", "--coarse_oracle", "--top_k", "1"], "fine_random"),
                                        (["--coarse_oracle", "--street_oracle", "--top_k", "1"], "street_oracle"),
                                        (["--street_oracle"], "path_coarse")])
def test_cli_conflicts_raise_before_any_file_is_opened(flags, text, monkeypatch):
    import text2pos_amd  # noqa: F401
    from text2pos_amd import io as IO, pipeline as PL

    def no_files(*a, **k):
        raise AssertionError("a file was opened before the switches were checked")
    monkeypatch.setattr(IO, "load_scenes", no_files)
    monkeypatch.setattr(IO, "load_pickle", no_files)
    monkeypatch.setattr(IO, "load_reference_checkpoint", no_files)
    monkeypatch.setattr(torch.cuda, "set_device", no_files)
    argv = ["--base_path", "/nonexistent"] + ([] if text == "path_coarse" else ["--path_coarse", "/nonexistent"]) + flags
    with pytest.raises(ValueError, match=text):
        PL.main(argv)
