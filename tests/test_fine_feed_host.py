"""Host side of the fine stage's training feed: the C ABI of t2p_fine_step_stats (declaration, binding, refusals that need no device),
training.SceneFineFeed's item tables against a restatement of the reference's load_pose_and_cell and against a fixture the reference
function itself wrote, its construction refusals, its determinism and the layout of its device batches.  The GPU side is
tests/test_gpu_fine_stats.py and tests/test_gpu_fine_feed.py."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fine_scene import make_fine_scene  # noqa: E402

from text2pos_amd import _lib, data as D, io as IO, ops, training as T  # noqa: E402
from text2pos_amd.scene import DeviceScene  # noqa: E402

NAME = "t2p_fine_step_stats"
COMBOS = [(c, l) for c in ("pose", "best") for l in ("center", "closest")]
PAD, HINTS = 8, 6


# ---- header, binding, exports, refusals -------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    header = open(_lib.HEADER).read()
    assert NAME in _lib.SYMBOLS and len(_lib.SYMBOLS[NAME][1]) == 16       # (types and layouts: tests/test_abi_host.py)
    assert hasattr(_lib.lib(), NAME) and callable(ops.fine_step_stats)
    assert _lib.ABI_VERSION == _lib.lib().t2p_abi_version()
    assert ops.FINE_STATS_MAX_BATCH == _lib.DEFINES["T2P_FINE_STATS_MAX_BATCH"] == 1024
    for cite in ("training/losses.py:33-62", "training/losses.py:81-123", "models/superglue_matcher.py:139-161"):
        assert cite in header, cite
    from text2pos_amd import build
    assert "fine_stats.hip" in build.SOURCES


def _call(batch=2, n_obj=5, n_hints=6, n_rows=4, null=None, loss=True):
    """The entry point with recognisable non-NULL host addresses: every case below is refused before a launch."""
    buf = (C.c_uint8 * 64)()
    a = C.addressof(buf)
    names = ("matches0", "matches1", "offsets", "pose_idx", "gt_hint", "pose_xy", "slot_center_xy", "sample_stats", "step_row")
    p = {k: C.c_void_p(0 if k == null else a) for k in names}
    l = C.c_void_p(a if loss else 0)
    rc = _lib.lib().t2p_fine_step_stats(p["matches0"], p["matches1"], p["offsets"], p["pose_idx"], batch, n_obj, n_hints, p["gt_hint"],
                                        p["pose_xy"], p["slot_center_xy"], n_rows, l, l, p["sample_stats"], p["step_row"], C.c_void_p(0))
    return rc, _lib.lib().t2p_last_error().decode()


def test_entry_point_refuses_up_front():
    for name in ("matches0", "matches1", "offsets", "pose_idx", "gt_hint", "pose_xy", "slot_center_xy", "sample_stats", "step_row"):
        rc, msg = _call(null=name)
        assert rc != 0 and "NULL" in msg, name
    for kw in (dict(batch=0), dict(n_obj=0), dict(n_hints=0)):
        rc, msg = _call(**kw)
        assert rc != 0 and ">= 1" in msg, kw
    for kw in (dict(n_obj=64), dict(n_hints=64)):
        rc, msg = _call(**kw)
        assert rc != 0 and "63" in msg, kw
    rc, msg = _call(batch=ops.FINE_STATS_MAX_BATCH + 1)
    assert rc != 0 and str(ops.FINE_STATS_MAX_BATCH) in msg and "LDS" in msg
    rc, msg = _call(n_rows=0)
    assert rc != 0 and "n_rows" in msg


def test_wrapper_has_no_cpu_path():
    z = lambda *s, dt=torch.int64: torch.zeros(s, dtype=dt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fine_step_stats(z(2, 5), z(2, 6), z(2, 6, 2, dt=torch.float32), z(2, dt=torch.int32), z(4, 5, dt=torch.int32),
                            z(4, 2, dt=torch.float64), z(4, 5, 2, dt=torch.float64))


# ---- the item tables --------------------------------------------------------------------------------------------------------------
def _restated_item(pose, cell, pad_size, num_mentioned, regressor_cell, regressor_learn):
    """dataloading/kitti360pose/poses.py:32-139 said again, statement by statement, on this package's classes: the object list
    (without the padding objects: None stands for one), matches, all_matches, offsets, offsets_best_center."""
    descriptions = pose.descriptions
    by_id = {obj.id: obj for obj in cell.objects}
    matched_ids = [d.object_id for d in descriptions if d.is_matched]
    assert len(descriptions) == num_mentioned
    if regressor_cell == "pose":
        offsets = np.array([getattr(d, "offset_" + regressor_learn) for d in descriptions])[:, 0:2]
    else:
        offsets = [getattr(d, "best_offset_" + regressor_learn)[0:2] if d.is_matched else getattr(d, "offset_" + regressor_learn)[0:2]
                   for d in descriptions]
    offsets = np.array(offsets)
    best_center = [d.best_offset_center[0:2] if d.is_matched else d.offset_center[0:2] for d in descriptions]
    objects, matches = [], []
    for i_descr, d in enumerate(descriptions):
        if d.is_matched:
            hint_obj = by_id[d.object_id]
            assert hint_obj.instance_id == d.object_instance_id
            objects.append(hint_obj)
            matches.append((len(objects) - 1, i_descr))
    for obj in cell.objects:
        if obj.id not in matched_ids:
            objects.append(obj)
    assert len(objects) == len(cell.objects)
    if len(objects) > pad_size:
        objects = objects[0:pad_size]
    while len(objects) < pad_size:
        objects.append(None)
    all_matches = matches.copy()
    for i_descr, d in enumerate(descriptions):
        if not d.is_matched:
            all_matches.append((len(objects), i_descr))
    for obj_idx, obj in enumerate(objects):
        if obj is None or obj.id not in matched_ids:
            all_matches.append((obj_idx, len(descriptions)))
    matches, all_matches = np.array(matches), np.array(all_matches)
    # the reference's closing assertions (poses.py:132-139)
    assert len(matches) == len(matched_ids)
    assert len(all_matches) == len(objects) + len(descriptions) - len(matches)
    assert np.sum(all_matches[:, 1] == len(descriptions)) == len(objects) - len(matched_ids)
    assert np.sum(all_matches[:, 0] == len(objects)) == len(descriptions) - len(matched_ids)
    return objects, matches.reshape(-1, 2), all_matches, offsets, np.array(best_center)


@pytest.fixture(scope="module")
def toy():
    cells, poses = make_fine_scene(9, 36, 13, PAD, HINTS)
    return IO.Scenes(cells, poses)


def test_the_scene_has_the_cases_on_purpose(toy):
    n_match = [sum(d.is_matched for d in p.descriptions) for p in toy.all_poses]
    sizes = [len(c.objects) for c in toy.all_cells]
    assert 0 in n_match and HINTS in n_match and any(0 < k < HINTS for k in n_match)
    assert max(sizes) > PAD and PAD in sizes and min(sizes) < PAD
    for p in toy.all_poses:
        ids = [d.object_id for d in p.descriptions if d.is_matched]
        assert len(set(ids)) == len(ids)
    # a matched object that sits behind the cut in cell order comes to the front
    assert any(max([[o.id for o in toy.cells_dict[p.cell_id].objects].index(d.object_id) for d in p.descriptions if d.is_matched],
                   default=-1) >= PAD for p in toy.all_poses)


@pytest.mark.parametrize("combo", COMBOS)
def test_item_tables_are_the_restated_reference(toy, combo):
    feed = T.SceneFineFeed(toy, None, 8, 3, 5, pad_size=PAD, num_mentioned=HINTS, regressor_cell=combo[0], regressor_learn=combo[1])
    feed.set_epoch(0)
    seen = 0
    for b in feed:
        assert sorted(b) == sorted(["poses", "cells", "objects", "object_points", "hint_descriptions", "texts", "matches", "all_matches",
                                    "offsets", "offsets_best_center", "pose_indices"])
        for i, p in enumerate(b["pose_indices"]):
            pose = toy.all_poses[int(p)]
            cell = toy.cells_dict[pose.cell_id]
            objects, matches, all_matches, offsets, best_center = _restated_item(pose, cell, PAD, HINTS, *combo)
            assert b["poses"][i] is pose and b["cells"][i] is cell and len(b["objects"][i]) == PAD
            for got, want in zip(b["objects"][i], objects):
                assert (got is want) if want is not None else (got.label == "pad" and got.id == -1 and len(got.xyz) == 8)
            assert np.array_equal(b["matches"][i], matches) and np.array_equal(b["all_matches"][i], all_matches)
            assert b["matches"][i].dtype == np.int64 and b["all_matches"][i].shape[1] == 2
            assert np.array_equal(b["offsets"][i], offsets) and b["offsets"][i].shape == (HINTS, 2)
            assert np.array_equal(b["offsets_best_center"][i], best_center)
            hints = [f"The pose is {d.direction} of a {d.object_color_text} {d.object_label}." for d in pose.descriptions]
            assert b["hint_descriptions"][i] == hints and b["texts"][i] == " ".join(hints)
            assert b["object_points"][i].pos.shape == (PAD * 8, 3)
            # the feed's resident tables say the same
            gt = np.full(PAD, -1)
            gt[matches[:, 0].astype(np.int64)] = matches[:, 1]          # (np.array([]) of a pose without matches is float)
            assert np.array_equal(feed.gt_hint[int(p)], gt) and np.array_equal(feed.pose_xy[int(p)], pose.pose[0:2])
            seen += 1
    assert seen == len(toy.all_poses)
    # the padding of slot j is the same object in every item, and DeviceScene's draw
    pads = DeviceScene(toy.all_cells[:1], "cpu", n_pad=PAD, pad_seed=3)
    for j, o in enumerate(feed._pads):
        assert np.array_equal(o.xyz, pads._flat[int(pads.pad_ids[j])].xyz)


def test_feed_against_the_reference_fixture(golden_dir):
    """tests/golden/fine_feed.npz: written by the reference's own load_pose_and_cell (tests/golden/make_golden_fine_feed.py)."""
    g = np.load(os.path.join(golden_dir, "fine_feed.npz"))
    load = lambda k: IO._SceneUnpickler(io.BytesIO(g[k].tobytes())).load()
    scenes = IO.Scenes(load("cells_pkl"), load("poses_pkl"))
    pad, hints = int(g["pad_size"]), int(g["num_mentioned"])
    n = len(scenes.all_poses)
    assert n == 14 and isinstance(scenes.all_cells[0], D.Cell) and isinstance(scenes.all_poses[0].descriptions[0], D.DescriptionBestCell)
    for cell_mode, learn in COMBOS:
        feed = T.SceneFineFeed(scenes, None, 8, 0, n, pad_size=pad, num_mentioned=hints, regressor_cell=cell_mode, regressor_learn=learn)
        b = next(iter(feed))
        assert np.array_equal(np.stack(b["offsets"]), g[f"offsets_{cell_mode}_{learn}"])
        for i in range(n):
            assert [o.id for o in b["objects"][i]] == g[f"ids_{i}"].tolist(), i
            assert np.array_equal(b["matches"][i], g[f"matches_{i}"]) and np.array_equal(b["all_matches"][i], g[f"all_matches_{i}"])
            assert np.array_equal(b["offsets_best_center"][i], g[f"best_center_{i}"])
    assert any((g[f"ids_{i}"] == -1).any() for i in range(n)) and any(len(g[f"matches_{i}"]) == 0 for i in range(n))


# ---- construction refusals --------------------------------------------------------------------------------------------------------
def _broken(change):
    cells, poses = make_fine_scene(5, 10, 21, PAD, HINTS)
    victim = next(i for i, p in enumerate(poses) if sum(d.is_matched for d in p.descriptions) >= 2)
    change(cells, poses, poses[victim])
    return IO.Scenes(cells, poses), victim


def test_construction_refusals():
    mk = lambda scenes, **kw: T.SceneFineFeed(scenes, None, 8, 0, 4, pad_size=kw.pop("pad_size", PAD), num_mentioned=HINTS, **kw)
    matched = lambda p: [d for d in p.descriptions if d.is_matched]
    cases = {
        "descriptions": lambda c, ps, p: p.descriptions.pop(),
        "does not hold": lambda c, ps, p: setattr(matched(p)[0], "object_id", 4242),
        "one object": lambda c, ps, p: setattr(matched(p)[1], "object_id", matched(p)[0].object_id),
        "NaN": lambda c, ps, p: setattr(p.descriptions[2], "offset_center", np.array([np.nan, 0.0])),
        "a cell the scene does not hold": lambda c, ps, p: setattr(p, "cell_id", "toy1_00099"),
    }
    for needle, change in cases.items():
        scenes, victim = _broken(change)
        with pytest.raises(ValueError, match=needle) as e:
            mk(scenes)
        assert f"pose {victim} " in str(e.value), (needle, str(e.value))
    # the instance the description names is the cell's object's (poses.py:87)
    scenes, victim = _broken(lambda c, ps, p: setattr(matched(p)[0], "object_instance_id", 77777))
    with pytest.raises(ValueError, match="instance"):
        mk(scenes)
    # more matched objects than pad_size
    scenes, _ = _broken(lambda c, ps, p: None)
    most = max(sum(d.is_matched for d in p.descriptions) for p in scenes.all_poses)
    with pytest.raises(ValueError, match="more than pad_size") as e:
        mk(scenes, pad_size=most - 1)
    assert "pose " in str(e.value)
    # the NaN counts only among the CHOSEN offsets
    scenes, _ = _broken(lambda c, ps, p: setattr(p.descriptions[2], "offset_closest", np.array([np.nan, 0.0])))
    mk(scenes)
    with pytest.raises(ValueError, match="NaN"):
        mk(scenes, regressor_learn="closest")
    # not built
    with pytest.raises(NotImplementedError, match="flip_pose"):
        mk(scenes, flip_pose=True)
    with pytest.raises(NotImplementedError, match="no_pc_augment"):
        mk(scenes, no_pc_augment=True)
    # a DeviceScene without enough padding objects, or without the poses' cells
    with pytest.raises(RuntimeError, match="n_pad"):
        T.SceneFineFeed(scenes, DeviceScene(scenes.all_cells, "cpu", n_pad=PAD - 1), 8, 0, 4, pad_size=PAD, num_mentioned=HINTS)
    with pytest.raises(ValueError, match="DeviceScene does not hold"):
        T.SceneFineFeed(scenes, DeviceScene(scenes.all_cells[:1], "cpu", n_pad=PAD), 8, 0, 4, pad_size=PAD, num_mentioned=HINTS)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def _items(feed, epoch):
    feed.set_epoch(epoch)
    items, sizes = {}, []
    for b in feed:
        sizes.append(len(b["texts"]))
        for i, p in enumerate(b["pose_indices"]):
            p = int(p)
            assert p not in items
            si = feed.sample_index(p, epoch)
            items[p] = (b["texts"][i], b["object_points"][i].pos.clone(), feed.transform.keys(si, np.arange(PAD)),
                        feed.transform.rotations(si, np.arange(PAD)), b["all_matches"][i])
    return items, sizes


def test_items_depend_on_seed_epoch_and_pose_only(toy):
    n = len(toy.all_poses)
    mk = lambda bs, sh: T.SceneFineFeed(toy, None, 8, 7, bs, shuffle=sh, pad_size=PAD, num_mentioned=HINTS)
    feeds = [mk(1, True), mk(3, True), mk(n, False), mk(5, True)]
    for epoch in (0, 1):
        runs = [_items(f, epoch) for f in feeds]
        ref, _ = runs[0]
        assert sorted(ref) == list(range(n))                       # with shuffle, an epoch visits every pose once
        for items, _ in runs[1:]:
            assert sorted(items) == list(range(n))
            for p in range(n):
                a, b = ref[p], items[p]
                assert a[0] == b[0] and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
                assert np.array_equal(a[4], b[4])
        assert runs[0][1] == [1] * n and runs[1][1] == [3] * (n // 3) and runs[2][1] == [n]
        assert runs[3][1] == [5] * (n // 5) + [n % 5] and len(feeds[3]) == n // 5 + 1        # the last short batch is kept
    e0, _ = _items(feeds[1], 0)
    e1, _ = _items(feeds[1], 1)
    assert all(not np.array_equal(e0[p][2], e1[p][2]) and not np.array_equal(e0[p][3], e1[p][3]) for p in range(n))
    assert not np.array_equal(feeds[1].epoch_order(0), feeds[1].epoch_order(1))
    assert np.array_equal(feeds[2].epoch_order(1), np.arange(n))
    cs = feeds[0].transform.rotations(feeds[0].sample_index(np.arange(n), 0)[:, None], np.arange(PAD)[None, :]).astype(np.float64)
    assert np.abs(np.degrees(np.arctan2(cs[..., 1], cs[..., 0]))).max() <= 120.0 + 1e-4          # the training default
    val = T.SceneFineFeed(toy, None, 8, 7, 4, pad_size=PAD, num_mentioned=HINTS, rotate_degrees=None)
    assert val.transform.rotations(0, np.arange(PAD)) is None


# ---- the device batch -------------------------------------------------------------------------------------------------------------
def test_device_batch_layout_matches_the_host_batch(toy):
    """A DeviceScene on the CPU (no kernel runs): object ids, keys and angles slot by slot, and the targets' gathers."""
    sc = DeviceScene(toy.all_cells, "cpu", n_pad=PAD + 2, pad_seed=7)
    kw = dict(pad_size=PAD, num_mentioned=HINTS, shuffle=True, regressor_cell="best", regressor_learn="closest")
    dev_feed = T.SceneFineFeed(toy, sc, 8, 7, 5, **kw)
    host_feed = T.SceneFineFeed(toy, sc, 8, 7, 5, host=True, **kw)
    assert dev_feed.scene is sc and not dev_feed.host and host_feed.host
    for epoch in (0, 2):
        dev_feed.set_epoch(epoch), host_feed.set_epoch(epoch)
        for bd, bh in zip(dev_feed, host_feed):
            assert bd["texts"] == bh["texts"] and bd["hint_descriptions"] == bh["hint_descriptions"]
            assert np.array_equal(bd["pose_indices"], bh["pose_indices"]) and "objects" not in bd and "scene_batch" not in bh
            sb, ft = bd["scene_batch"], bd["fine_targets"]
            b = len(bd["texts"])
            assert sb["flip"] is None and sb["n_pts"] == 8 and np.array_equal(sb["cell_ptr"], np.arange(b + 1) * PAD)
            assert sb["cell_ptr"].dtype == np.int32 and sb["obj_ids"].shape == (b * PAD,) and sb["rot"].shape == (b * PAD, 2)
            for i, p in enumerate(bd["pose_indices"]):
                si = dev_feed.sample_index(int(p), epoch)
                lo = i * PAD
                for s, o in enumerate(bh["objects"][i]):
                    assert sc._flat[int(sb["obj_ids"][lo + s])] is o            # the host twin's object of that slot
                    assert (o.label == "pad") == (int(sb["obj_ids"][lo + s]) == int(sc.pad_ids[s]))     # slot j pads with pad_ids[j]
                assert np.array_equal(sb["keys"][lo: lo + PAD], dev_feed.transform.keys(si, np.arange(PAD)))
                assert np.array_equal(sb["rot"][lo: lo + PAD], dev_feed.transform.rotations(si, np.arange(PAD)))
                # what the host twin's for_cell(sample) consumes: the same draws
                want = D.batch_object_points(bh["objects"][i], dev_feed.transform.for_cell(int(si)))
                assert torch.equal(want.pos, bh["object_points"][i].pos)
            assert all(not isinstance(v, (list, tuple)) and isinstance(v, torch.Tensor) for v in ft.values())
            assert ft["pose_idx"].dtype == torch.int32 and ft["pose_idx"].tolist() == bd["pose_indices"].tolist()
            assert ft["gt_hint"].dtype == torch.int32 and tuple(ft["gt_hint"].shape) == (len(toy.all_poses), PAD)
            assert ft["pose_xy"].dtype == torch.float64 and ft["slot_center_xy"].dtype == torch.float64
            assert ft["target_offsets"].dtype == torch.float32
            assert np.array_equal(ft["target_offsets"].numpy(), np.stack(bh["offsets"]).astype(np.float32))
            assert ft["idx"].dtype == torch.int32 and ft["entry_ptr"].dtype == torch.int32 and ft["idx"].is_contiguous()
            ptr = ft["entry_ptr"].numpy()
            assert ptr[0] == 0 and ptr.shape == (b + 1,) and ptr[-1] == ft["idx"].shape[0]
            for i, p in enumerate(bd["pose_indices"]):
                assert np.array_equal(ft["idx"].numpy()[ptr[i]: ptr[i + 1]], bh["all_matches"][i])
                centres = np.array([o.get_center()[0:2] for o in bh["objects"][i]])
                assert np.abs(ft["slot_center_xy"].numpy()[int(p)] - centres).max() < 1e-14
                assert np.array_equal(ft["slot_center_xy"].numpy()[int(p)], sc.center64[sb["obj_ids"][i * PAD: (i + 1) * PAD]][:, 0:2])
                assert np.array_equal(ft["pose_xy"].numpy()[int(p)], np.asarray(bh["poses"][i].pose)[0:2])
