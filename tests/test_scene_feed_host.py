"""Host side of the on-device training feed: the C ABI of t2p_pack_scene_objects_aug (declaration, binding, refusals that need no
device), data.flip_cell, the mirror tables of a DeviceScene, and the determinism and draw sanity of training.SceneCoarseFeed.  The GPU
side is tests/test_gpu_scene_feed.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from text2pos_amd import _lib, data as D, io as IO, synthetic as S, training as T
from text2pos_amd.scene import DeviceScene

NAME = "t2p_pack_scene_objects_aug"
DIRS = ["north", "south", "east", "west", "on-top"]


def _toy_scene(n_cells=16, n_poses=40, seed=5, max_pts=60):
    """A small raw scene in the package's data model: cells of 2-5 objects with coordinates in [-0.3, 1.4], 6 hints per pose."""
    rng = np.random.default_rng(seed)
    cells, poses = [], []
    for i in range(n_cells):
        objs = []
        for j in range(int(rng.integers(2, 6))):
            n = int(rng.integers(10, max_pts))     # (NormalizeScale of a resampled single point is 0 / 0, in the reference too)
            objs.append(D.Object3d(j, 1000 * i + j, rng.uniform(-0.3, 1.4, (n, 3)), np.clip(rng.random((n, 3)), 0, 1),
                                   S.LABELS[int(rng.integers(0, len(S.LABELS)))]))
        x, y = 30.0 * (i % 4), 30.0 * (i // 4)
        cells.append(D.Cell(i, "toy1", objs, 30.0, np.array([x, y, 0.0, x + 30.0, y + 30.0, 10.0])))
    for q in range(n_poses):
        c = cells[q % n_cells]
        descs = [D.DescriptionBestCell(DIRS[int(rng.integers(0, 5))], o.get_color_text(), o.label, o.id, True)
                 for o in [c.objects[int(k)] for k in rng.integers(0, len(c.objects), 6)]]
        poses.append(D.Pose(rng.random(3), c.bbox_w[0:3] + rng.random(3) * 30.0, c.id, "toy1", descs))
    return cells, poses


# ---- header, binding, exports, refusals -------------------------------------------------------------------------------------------
def test_aug_entry_point_is_declared_bound_and_exported():
    header = open(_lib.HEADER).read()
    assert NAME in _lib.SYMBOLS and len(_lib.SYMBOLS[NAME][1]) == 19       # (types and layouts: tests/test_abi_host.py)
    assert hasattr(_lib.lib(), NAME)
    assert _lib.ABI_VERSION == _lib.lib().t2p_abi_version()
    for cite in ("cells.py:79-91", "utils.py:13-86", "training/coarse.py:192-198"):
        assert cite in header, cite


def _call(n_out=1, n_pts=8, key=True, flip=False, mirror=False, center=False, center_mirror=False):
    """The entry point with recognisable non-NULL host addresses: every case below is refused (or returns) before a launch."""
    buf = (C.c_uint8 * 64)()
    a = C.addressof(buf)
    p = lambda on: C.c_void_p(a if on else 0)
    rc = _lib.lib().t2p_pack_scene_objects_aug(p(True), p(True), p(mirror), p(True), p(True), p(key), p(flip), p(False), p(True),
                                               p(center_mirror), p(True), n_out, n_pts, p(True), p(False), p(center), p(False),
                                               p(False), C.c_void_p(0))
    return rc, _lib.lib().t2p_last_error().decode()


def test_aug_entry_point_refuses_up_front():
    rc, msg = _call(flip=True, mirror=False)
    assert rc != 0 and "mirror" in msg
    rc, msg = _call(flip=True, mirror=True, center=True, center_mirror=False)
    assert rc != 0 and "scene_center_mirror_xy" in msg
    rc, msg = _call(n_pts=1025)
    assert rc != 0 and "1024" in msg
    rc, msg = _call(key=False)
    assert rc != 0 and "NULL" in msg
    rc, _ = _call(n_out=0)
    assert rc == 0
    rc, _ = _call(n_out=0, key=False)
    assert rc == 0


# ---- flip_cell --------------------------------------------------------------------------------------------------------------------
TEXT = "The pose is east of a gray pole. The pose is west of a green box. It is north of x, south of y and on-top of z."


def test_flip_cell_text():
    cells, _ = _toy_scene(2, 2)
    h = D.flip_cell(cells[0], TEXT, 1)[1]
    v = D.flip_cell(cells[0], TEXT, -1)[1]
    assert h == "The pose is west of a gray pole. The pose is east of a green box. It is north of x, south of y and on-top of z."
    assert v == "The pose is east of a gray pole. The pose is west of a green box. It is south of x, north of y and on-top of z."
    both = D.flip_cell(cells[0], h, -1)[1]
    assert both == "The pose is west of a gray pole. The pose is east of a green box. It is south of x, north of y and on-top of z."
    assert D.flip_cell_code(cells[0], TEXT, 3)[1] == both
    assert D.flip_cell(cells[0], h, 1)[1] == TEXT and D.flip_cell(cells[0], v, -1)[1] == TEXT
    plain = "The pose is on-top of a gray road."
    assert D.flip_cell(cells[0], plain, 1)[1] == plain and D.flip_cell(cells[0], plain, -1)[1] == plain
    with pytest.raises(ValueError):
        D.flip_cell(cells[0], TEXT, 0)


def test_flip_cell_points_and_original():
    cells, _ = _toy_scene(3, 3)
    cell = cells[1]
    before = [(o.xyz.copy(), o.rgb.copy()) for o in cell.objects]
    for direction, axis in ((1, 0), (-1, 1)):
        flipped, _ = D.flip_cell(cell, "", direction)
        assert flipped is not cell and flipped.id == cell.id and len(flipped.objects) == len(cell.objects)
        for o, q, (xyz0, rgb0) in zip(cell.objects, flipped.objects, before):
            assert q is not o and q.xyz is not o.xyz and q.xyz.dtype == np.float64
            want = xyz0.copy()
            want[:, axis] = 1 - xyz0[:, axis]
            assert np.array_equal(q.xyz, want)
            assert np.array_equal(q.rgb, rgb0) and q.label == o.label
            assert np.array_equal(o.xyz, xyz0) and np.array_equal(o.rgb, rgb0)      # the original, bit-unchanged
    twice = D.flip_cell_code(cell, "", 3)[0]
    for q, (xyz0, _) in zip(twice.objects, before):
        assert np.array_equal(q.xyz[:, :2], 1 - xyz0[:, :2]) and np.array_equal(q.xyz[:, 2], xyz0[:, 2])


# ---- mirror tables ----------------------------------------------------------------------------------------------------------------
def test_mirror_tables_are_the_float64_mirror_cast():
    rng = np.random.default_rng(3)
    objs = [D.Object3d(j, j, rng.uniform(-0.3, 1.4, (n, 3)), rng.random((n, 3)), "pole") for j, n in enumerate((1, 2, 63, 3000))]
    cell = D.Cell(0, "toy1", objs, 30.0, np.array([0.0, 0.0, 0.0, 30.0, 30.0, 10.0]))
    plain = DeviceScene([cell], "cpu")
    assert plain.raw_mirror_xy is None and plain.center_mirror_xy is None
    sc = DeviceScene([cell], "cpu", mirror=True)
    xyz64 = np.concatenate([o.xyz for o in objs], 0)
    assert sc.raw_mirror_xy.dtype == torch.float32 and tuple(sc.raw_mirror_xy.shape) == (xyz64.shape[0], 2)
    assert np.array_equal(sc.raw_mirror_xy.numpy(), (1.0 - xyz64[:, :2]).astype(np.float32))
    assert np.array_equal(sc.raw_xyz.numpy(), xyz64.astype(np.float32))          # the plain image is what it was
    got = sc.center_mirror_xy.numpy()
    assert got.dtype == np.float32 and got.shape == (4, 2)
    for i, o in enumerate(objs):
        for a in (0, 1):
            assert got[i, a] == np.float32(np.mean(1.0 - o.xyz[:, a])), (i, a)
        flipped = D.flip_cell_code(cell, "", 3)[0].objects[i]
        assert np.array_equal(got[i], flipped.get_center()[:2].astype(np.float32))
    assert np.array_equal(sc.center.numpy(), plain.center.numpy())
    with pytest.raises(RuntimeError, match="mirror"):
        T.SceneCoarseFeed(IO.Scenes([cell], []), plain, 8, 0, 4)


# ---- the feed ---------------------------------------------------------------------------------------------------------------------
def _items(feed, epoch):
    """{pose index: (text, flip code, angles, sampled points)} of one pass over `feed` (host batches) in `epoch`."""
    feed.set_epoch(epoch)
    items, sizes = {}, []
    for b in feed:
        sizes.append(len(b["texts"]))
        for i, p in enumerate(b["pose_indices"]):
            p = int(p)
            assert p not in items
            n = len(b["objects"][i])
            si = feed.sample_index(p, epoch)
            items[p] = (b["texts"][i], int(feed.flip_codes(p, epoch)[0]), feed.transform.rotations(si, np.arange(n)),
                        b["object_points"][i].pos.clone(), feed.transform.keys(si, np.arange(n)), b["cell_ids"][i])
    return items, sizes


def test_feed_items_depend_on_seed_epoch_and_pose_only():
    cells, poses = _toy_scene(16, 40)
    scenes = IO.Scenes(cells, poses)
    mk = lambda bs, sh: T.SceneCoarseFeed(scenes, None, 8, 7, bs, shuffle=sh, host=True)
    feeds = [mk(4, True), mk(7, True), mk(40, False)]
    for epoch in (0, 1):
        runs = [_items(f, epoch) for f in feeds]
        runs.append(_items(feeds[0], epoch))                 # a second pass after set_epoch(epoch) was set again
        ref, _ = runs[0]
        assert sorted(ref) == list(range(40))                # an epoch visits every pose once
        for items, _ in runs[1:]:
            assert sorted(items) == list(range(40))
            for p in range(40):
                a, b = ref[p], items[p]
                assert a[0] == b[0] and a[1] == b[1] and a[5] == b[5] == poses[p].cell_id
                assert np.array_equal(a[2], b[2]) and torch.equal(a[3], b[3]) and np.array_equal(a[4], b[4])
        assert runs[1][1] == [7, 7, 7, 7, 7, 5]              # the last short batch is kept
        assert runs[0][1] == [4] * 10 and runs[2][1] == [40] and len(feeds[1]) == 6 and len(feeds[0]) == 10
    e0, _ = _items(feeds[0], 0)
    e1, _ = _items(feeds[0], 1)
    assert all(not np.array_equal(e0[p][4], e1[p][4]) for p in range(40))       # epochs differ in keys
    o0, o1 = feeds[0].epoch_order(0), feeds[0].epoch_order(1)
    assert not np.array_equal(o0, o1) and np.array_equal(feeds[2].epoch_order(1), np.arange(40))
    # the flipped copies are what the host batch hands over
    feeds[2].set_epoch(0)
    b = next(iter(feeds[2]))
    for i, p in enumerate(b["pose_indices"]):
        want = D.flip_cell_code(scenes.cells_dict[poses[int(p)].cell_id], "", int(feeds[2].flip_codes(int(p), 0)[0]))[0]
        assert all(np.array_equal(x.xyz, y.xyz) for x, y in zip(b["objects"][i], want.objects))


def test_feed_draws_are_sane():
    cells, poses = _toy_scene(16, 40)
    scenes = IO.Scenes(cells, poses)
    feed = T.SceneCoarseFeed(scenes, None, 8, 11, 8, host=True)
    codes, angles = [], []
    for epoch in range(50):
        codes.append(feed.flip_codes(np.arange(40), epoch))
        for p in range(40):
            order = feed.hint_order(p, epoch)
            assert sorted(order.tolist()) == list(range(6))
            cs = feed.transform.rotations(feed.sample_index(p, epoch), np.arange(3)).astype(np.float64)
            assert cs.shape == (3, 2) and np.abs((cs ** 2).sum(1) - 1).max() < 1e-6
            angles.append(np.degrees(np.arctan2(cs[:, 1], cs[:, 0])))
    codes = np.concatenate(codes)
    assert codes.shape == (2000,) and codes.dtype == np.uint8 and codes.max() <= 3
    share = np.bincount(codes, minlength=4) / 2000.0
    assert (share > 0.20).all() and (share < 0.30).all(), share
    angles = np.concatenate(angles)
    assert np.abs(angles).max() <= 120.0 + 1e-4 and angles.min() < -60 and angles.max() > 60
    assert any(not np.array_equal(feed.hint_order(p, 0), np.arange(6)) for p in range(40))


def test_no_cell_augment_is_the_plain_text_and_no_flip():
    cells, poses = _toy_scene(16, 40)
    scenes = IO.Scenes(cells, poses)
    feed = T.SceneCoarseFeed(scenes, None, 8, 7, 16, shuffle=False, shuffle_hints=False, flip_poses=False, host=True)
    assert not feed.flip_codes(np.arange(40), 3).any()
    seen = 0
    for b in feed:
        for i, p in enumerate(b["pose_indices"]):
            assert b["texts"][i] == scenes.texts[int(p)]
            cell = scenes.cells_dict[poses[int(p)].cell_id]
            assert all(np.array_equal(x.xyz, y.xyz) for x, y in zip(b["objects"][i], cell.objects))
            seen += 1
    assert seen == 40


def test_device_batch_layout_matches_the_host_batch():
    """The scene batch of a DeviceScene on the CPU (no kernel runs): object ids, slots' keys, per-slot flip codes, cell_ptr."""
    cells, poses = _toy_scene(16, 40)
    scenes = IO.Scenes(cells, poses)
    sc = DeviceScene(cells, "cpu", mirror=True)
    dev_feed = T.SceneCoarseFeed(scenes, sc, 8, 7, 7, shuffle=True)
    host_feed = T.SceneCoarseFeed(scenes, sc, 8, 7, 7, shuffle=True, host=True)
    for bd, bh in zip(dev_feed, host_feed):
        assert bd["texts"] == bh["texts"] and bd["cell_ids"] == bh["cell_ids"] and "objects" not in bd
        sb = bd["scene_batch"]
        counts = [len(o) for o in bh["objects"]]
        assert np.array_equal(sb["cell_ptr"], np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
        a = 0
        for i, p in enumerate(bd["pose_indices"]):
            row, n = sc.row_of[poses[int(p)].cell_id], counts[i]
            assert np.array_equal(sb["obj_ids"][a: a + n], np.arange(sc.cell_ptr[row], sc.cell_ptr[row] + n))
            si = dev_feed.sample_index(int(p))
            assert np.array_equal(sb["keys"][a: a + n], dev_feed.transform.keys(si, np.arange(n)))
            assert np.array_equal(sb["rot"][a: a + n], dev_feed.transform.rotations(si, np.arange(n)))
            assert (sb["flip"][a: a + n] == dev_feed.flip_codes(int(p))[0]).all()
            a += n
