"""GPU side of the on-device training feed (-m gpu): t2p_pack_scene_objects_aug against the host twin of the augmentation
(data.flip_cell in float64 -> KeyedFixedPoints [-> RotateZ] -> NormalizeScale), against the plain entry point and against
t2p_pack_objects; CellRetrievalNetwork.encode_scene_batch, training.train_epoch on training.SceneCoarseFeed, and the train_coarse
command.  The host side is tests/test_scene_feed_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DIRS = ["north", "south", "east", "west", "on-top"]
SEED = 17


def _dev():
    return torch.device("cuda:0")


def _toy_scene(n_cells, n_poses, seed, sizes=None, lo_pts=30, hi_pts=400, scene_name="toy1"):
    """A small raw scene in the package's data model: cells of 2-5 objects (coordinates in [-0.3, 1.4]), 6 hints per pose, pose q
    in cell q % n_cells.  sizes: explicit raw point counts handed out object by object (then repeated)."""
    from text2pos_amd import data as D, synthetic as S
    rng = np.random.default_rng(seed)
    cells, poses, k = [], [], 0
    for i in range(n_cells):
        objs = []
        for j in range(int(rng.integers(2, 6))):
            n = int(sizes[k % len(sizes)]) if sizes is not None else int(rng.integers(lo_pts, hi_pts))
            k += 1
            objs.append(D.Object3d(j, 1000 * i + j, rng.uniform(-0.3, 1.4, (n, 3)), np.clip(rng.random((n, 3)), 0, 1),
                                   S.LABELS[int(rng.integers(0, len(S.LABELS)))]))
        x, y = 30.0 * (i % 4), 30.0 * (i // 4)
        cells.append(D.Cell(i, scene_name, objs, 30.0, np.array([x, y, 0.0, x + 30.0, y + 30.0, 10.0])))
    for q in range(n_poses):
        c = cells[q % n_cells]
        descs = [D.DescriptionBestCell(DIRS[int(rng.integers(0, 5))], o.get_color_text(), o.label, o.id, True)
                 for o in [c.objects[int(k)] for k in rng.integers(0, len(c.objects), 6)]]
        poses.append(D.Pose(rng.random(3), c.bbox_w[0:3] + rng.random(3) * 30.0, c.id, scene_name, descs))
    return cells, poses


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_case():
    """12 cells whose objects have 1 ... 3,000 raw points + 4 padding objects, resident on the GPU with the mirror tables; one
    slot per scene object with flip codes 0-3 in turn, then one 3,000-point object in four slots with the four codes."""
    from text2pos_amd import data as D
    from text2pos_amd.scene import DeviceScene
    sizes = [1, 3000, 2, 63, 64, 65, 7, 255, 256, 257, 1000, 31, 129, 2999, 500, 12]
    cells, _ = _toy_scene(12, 0, 23, sizes=sizes)
    scene = DeviceScene(cells, _dev(), n_pad=4, mirror=True)
    flat = scene._flat
    assert len(scene.pad_ids) == 4 and scene.n_objects == len(flat)
    big = next(i for i, o in enumerate(flat) if len(o.xyz) == 3000)
    ids = np.concatenate([np.arange(scene.n_objects), np.full(4, big)]).astype(np.int64)
    flip = np.concatenate([np.arange(scene.n_objects) % 4, np.arange(4)]).astype(np.uint8)
    assert set(flip.tolist()) == {0, 1, 2, 3} and sorted(len(o.xyz) for o in flat)[0] == 1
    keys = D.sample_keys(SEED, np.arange(len(ids)), 0)
    # the flipped objects of the host twin, once: flip_cell on a one-object cell, in float64
    twins = []
    for o, f in zip([flat[i] for i in ids], flip):
        cell = D.Cell(0, "t", [o], 30.0, np.zeros(6))
        twins.append(D.flip_cell_code(cell, "", int(f))[0].objects[0])
    return dict(scene=scene, flat=flat, ids=ids, flip=flip, keys=keys, twins=twins)


def _host_twin(case, n_pts, rot=None):
    """(xyz, rgb, center, mean_rgb, idx) of the case's slots by the host chain."""
    from text2pos_amd import data as D
    xyz, rgb, center, mean_rgb = [], [], [], []
    for s, q in enumerate(case["twins"]):
        chain = [D.KeyedFixedPoints(n_pts, SEED, s)]
        if rot is not None:
            chain.append(D.RotateZ(rot[s, 0], rot[s, 1]))
        chain.append(D.NormalizeScale())
        d = D.Compose(chain)(D.Data(x=torch.tensor(q.rgb, dtype=torch.float), pos=torch.tensor(q.xyz, dtype=torch.float)))
        xyz.append(d.pos)
        rgb.append(d.x)
        center.append(torch.from_numpy(q.get_center().astype(np.float32)))
        mean_rgb.append(torch.from_numpy(q.get_color_rgb().astype(np.float32)))
    idx = D.keyed_draws(case["keys"], [len(q.xyz) for q in case["twins"]], n_pts)
    return torch.stack(xyz), torch.stack(rgb), torch.stack(center), torch.stack(mean_rgb), torch.from_numpy(idx).int()


@pytest.fixture(scope="module")
def twins_by_npts(kernel_case):
    return {n: _host_twin(kernel_case, n) for n in (8, 100, 256)}


def _raw_call(case, n_pts, flip, rot, want=("xyz", "rgb", "center", "mean_rgb", "idx")):
    """The C entry point on NaN-prefilled (idx: -1) outputs; outputs not in `want` are passed as NULL.  Returns the buffers."""
    from text2pos_amd import _lib
    sc, dev = case["scene"], _dev()
    n = len(case["ids"])
    ids = torch.from_numpy(case["ids"].astype(np.int32)).to(dev)
    keys = torch.from_numpy(case["keys"].view(np.int64)).to(dev)
    f = None if flip is None else torch.from_numpy(np.ascontiguousarray(flip, dtype=np.uint8)).to(dev)
    r = None if rot is None else torch.from_numpy(np.ascontiguousarray(rot, dtype=np.float32)).to(dev)
    out = dict(xyz=torch.full((n, n_pts, 3), float("nan"), device=dev), rgb=torch.full((n, n_pts, 3), float("nan"), device=dev),
               center=torch.full((n, 3), float("nan"), device=dev), mean_rgb=torch.full((n, 3), float("nan"), device=dev),
               idx=torch.full((n, n_pts), -1, dtype=torch.int32, device=dev))
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    o = lambda name: p(out[name] if name in want else None)
    rc = _lib.lib().t2p_pack_scene_objects_aug(p(sc.raw_xyz), p(sc.raw_rgb), p(sc.raw_mirror_xy), p(sc.obj_ptr), p(ids), p(keys), p(f),
                                               p(r), p(sc.center), p(sc.center_mirror_xy), p(sc.color), n, n_pts, o("xyz"), o("rgb"),
                                               o("center"), o("mean_rgb"), o("idx"),
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "t2p_pack_scene_objects_aug")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _same_xyz(got, want, one_point_slots):
    """torch.equal, except that a resampled ONE-point object is 0 / 0 in NormalizeScale - NaN on the host as on the GPU, and NaN
    equals nothing: there the NaNs must sit where the host twin has them (and nowhere else may one be left)."""
    nan_w = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan_w)
    assert not nan_w.any() or set(torch.nonzero(nan_w.flatten(1).any(1)).flatten().tolist()) <= set(one_point_slots)
    return torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))


@pytest.mark.parametrize("n_pts", [8, 100, 256])
def test_flips_are_the_host_twin_bit_for_bit(kernel_case, twins_by_npts, n_pts):
    got = _raw_call(kernel_case, n_pts, kernel_case["flip"], None)
    xyz, rgb, center, mean_rgb, idx = twins_by_npts[n_pts]
    one = [s for s, q in enumerate(kernel_case["twins"]) if len(q.xyz) == 1]
    assert _same_xyz(got["xyz"], xyz, one)
    assert torch.equal(got["rgb"], rgb) and torch.equal(got["center"], center) and torch.equal(got["mean_rgb"], mean_rgb)
    assert torch.equal(got["idx"], idx)
    for k in ("rgb", "center", "mean_rgb"):
        assert not torch.isnan(got[k]).any(), k                     # nothing of the prefill is left
    assert not torch.isnan(got["xyz"][[s for s in range(len(xyz)) if s not in one]]).any()
    # the one object in four slots: four different images of the same draw
    four = got["xyz"][-4:]
    assert not torch.equal(four[0], four[1]) and not torch.equal(four[0], four[2]) and not torch.equal(four[1], four[3])
    # through DeviceScene.pack (the route of the feed): the same arrays
    sc = kernel_case["scene"]
    via = sc.pack(kernel_case["ids"], kernel_case["keys"], n_pts, want_idx=True, flip=kernel_case["flip"])
    for a, k in zip(via, ("xyz", "rgb", "center", "mean_rgb", "idx")):
        assert torch.equal(torch.nan_to_num(a.cpu(), nan=7.0), torch.nan_to_num(got[k], nan=7.0)), k


@pytest.mark.parametrize("n_pts", [8, 100, 256])
def test_no_augmentation_is_the_plain_entry_point(kernel_case, n_pts):
    sc = kernel_case["scene"]
    plain = [t.cpu() for t in sc.pack(kernel_case["ids"], kernel_case["keys"], n_pts, want_idx=True)]
    for flip in (np.zeros(len(kernel_case["ids"]), np.uint8), None):
        got = _raw_call(kernel_case, n_pts, flip, None)
        for a, k in zip(plain, ("xyz", "rgb", "center", "mean_rgb", "idx")):
            assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(got[k], nan=7.0)), (k, flip is None)
            assert torch.equal(torch.isnan(a), torch.isnan(got[k])) if a.is_floating_point() else True


def test_flip_needs_the_mirror_tables(kernel_case):
    from text2pos_amd.scene import DeviceScene
    from text2pos_amd import data as D
    cells, _ = _toy_scene(2, 0, 3)
    sc = DeviceScene(cells, _dev())
    ids = np.arange(sc.n_objects)
    with pytest.raises(RuntimeError, match="mirror"):
        sc.pack(ids, D.sample_keys(0, ids, 0), 8, flip=np.zeros(len(ids), np.uint8))
    with pytest.raises(RuntimeError, match="0..3"):
        kernel_case["scene"].pack(kernel_case["ids"], kernel_case["keys"], 8, flip=np.full(len(kernel_case["ids"]), 4, np.uint8))
    # rotation alone needs no mirror tables
    rot = D.keyed_rotations(D.sample_keys(0, ids, 0), 120.0)
    assert bool(torch.isfinite(sc.pack(ids, D.sample_keys(0, ids, 0), 8, rot=rot)[0]).all())


@pytest.mark.parametrize("n_pts", [8, 100, 256])
def test_rotation(kernel_case, twins_by_npts, n_pts):
    from text2pos_amd import data as D, ops
    case = kernel_case
    n = len(case["ids"])
    one = [s for s, q in enumerate(case["twins"]) if len(q.xyz) == 1]
    keep = [s for s in range(n) if s not in one]
    rot = D.keyed_rotations(case["keys"], 120.0)
    got = _raw_call(case, n_pts, case["flip"], rot)
    # (a) the host twin's RotateZ -> NormalizeScale, at the bound k_pack_objects' rotation is held to (2e-6 on normalised points)
    want = _host_twin(case, n_pts, rot)
    assert (got["xyz"][keep] - want[0][keep]).abs().max().item() < 2e-6
    for a, k in zip(want[1:], ("rgb", "center", "mean_rgb", "idx")):
        assert torch.equal(a, got[k]), k
    assert (got["xyz"][keep] - twins_by_npts[n_pts][0][keep]).abs().max().item() > 1e-2       # (it did rotate)
    # (b) t2p_pack_objects on the slots' (mirrored where flipped) fp32 points with the same draws and angles: the same bits
    sc = case["scene"]
    raw, mir, rgb_all, ptr = sc.raw_xyz.cpu().numpy(), sc.raw_mirror_xy.cpu().numpy(), sc.raw_rgb.cpu().numpy(), sc.obj_ptr.cpu().numpy()
    pts, cols, sizes = [], [], []
    for o, f in zip(case["ids"], case["flip"]):
        a, b = int(ptr[o]), int(ptr[o + 1])
        p = raw[a:b].copy()
        if f & 1:
            p[:, 0] = mir[a:b, 0]
        if f & 2:
            p[:, 1] = mir[a:b, 1]
        pts.append(p)
        cols.append(rgb_all[a:b])
        sizes.append(b - a)
    slot_ptr = np.zeros(n + 1, np.int32)
    slot_ptr[1:] = np.cumsum(sizes)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    ref = ops.pack_objects(to(np.concatenate(pts)), to(np.concatenate(cols)), to(slot_ptr), got["idx"].to(_dev()), to(rot))
    assert torch.equal(torch.nan_to_num(ref[0].cpu(), nan=7.0), torch.nan_to_num(got["xyz"], nan=7.0))
    assert torch.equal(torch.isnan(ref[0].cpu()), torch.isnan(got["xyz"]))
    assert torch.equal(ref[1].cpu(), got["rgb"])
    # (c) the identity rotation is no rotation, bit for bit
    ident = np.tile(np.array([[1.0, 0.0]], np.float32), (n, 1))
    unrot = _raw_call(case, n_pts, case["flip"], ident)
    assert _same_xyz(unrot["xyz"], twins_by_npts[n_pts][0], one)


def test_null_outputs_are_not_written(kernel_case):
    from text2pos_amd import data as D
    case, n_pts = kernel_case, 100
    rot = D.keyed_rotations(case["keys"], 120.0)
    full = _raw_call(case, n_pts, case["flip"], rot)
    names = ("rgb", "center", "mean_rgb", "idx")
    for drop in [(k,) for k in names] + [names]:
        got = _raw_call(case, n_pts, case["flip"], rot, want=tuple(k for k in ("xyz",) + names if k not in drop))
        assert torch.equal(torch.nan_to_num(got["xyz"], nan=7.0), torch.nan_to_num(full["xyz"], nan=7.0)), drop
        for k in names:
            if k in drop:       # still the prefill
                assert bool((got[k] == -1).all()) if k == "idx" else bool(torch.isnan(got[k]).all()), (drop, k)
            else:
                assert torch.equal(got[k], full[k]), (drop, k)


# ---- the model on a scene batch ---------------------------------------------------------------------------------------------------
def _model(vocab, seed=37, **kw):
    import weights as W
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    m = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(**kw))
    W.fill_state_dict(m, seed)
    return m.to(_dev())


def _feeds(n_cells, n_poses, batch, n_pts=256, rotate=None, seed=5, scene_seed=41, **kw):
    from text2pos_amd import io as IO, training as T
    from text2pos_amd.scene import DeviceScene
    cells, poses = _toy_scene(n_cells, n_poses, scene_seed)
    scenes = IO.Scenes(cells, poses)
    sc = DeviceScene(cells, _dev(), mirror=True)
    mk = lambda host: T.SceneCoarseFeed(scenes, sc, n_pts, seed, batch, rotate_degrees=rotate, host=host, **kw)
    return mk(False), mk(True), sc


def test_encode_scene_batch_is_encode_objects_on_the_host_twin(vocab):
    dev_feed, host_feed, sc = _feeds(4, 4, 4)
    bd, bh = next(iter(dev_feed)), next(iter(host_feed))
    assert bd["texts"] == bh["texts"] and "objects" not in bd and "scene_batch" not in bh
    codes = dev_feed.flip_codes(bd["pose_indices"])
    assert codes.any() and len(set(codes.tolist())) > 1            # flips are on, and not all the same
    assert bd["scene_batch"]["rot"] is None
    m1, m2 = _model(vocab), _model(vocab)
    m1.train(), m2.train()
    a, inputs = m1.encode_scene_batch(sc, bd["scene_batch"], want_inputs=True)
    b = m2.encode_objects(bh["objects"], bh["object_points"])
    torch.cuda.synchronize()
    assert a.grad_fn is not None and tuple(a.shape) == (4, 256)
    assert torch.equal(inputs[0].cpu().view(-1, 3), torch.cat([p.pos for p in bh["object_points"]]))      # the packed arrays
    assert torch.equal(a, b)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    moved = 0
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
        moved += int("running_mean" in k)
    assert moved > 0
    m1.eval(), m2.eval()
    with torch.no_grad():
        a = m1.encode_scene_batch(sc, bd["scene_batch"])
        b = m2.encode_objects(bh["objects"], bh["object_points"])
    assert a.grad_fn is None and torch.equal(a, b)
    with pytest.raises(NotImplementedError):
        m1.encode_scene_batch(sc, bd["scene_batch"])               # eval() with autograd: the folded kernels are forward-only


def test_train_epoch_on_the_device_feed(vocab):
    from text2pos_amd import synthetic as S, training as T
    dev_feed, host_feed, sc = _feeds(16, 16, 8, rotate=None)
    crit = T.make_criterion(S.default_args(margin=0.35, ranking_loss="pairwise"))
    results = []
    for feed in (dev_feed, host_feed, host_feed):
        m = _model(vocab)
        opt = torch.optim.SGD(m.parameters(), lr=0.0)      # (the step leaves parameters and gradients as backward() left them)
        feed.set_epoch(0)
        loss, seen = T.train_epoch(m, feed, opt, crit, max_batches=1)
        torch.cuda.synchronize()
        assert len(seen) == 1 and ("scene_batch" in seen[0]) == (feed is dev_feed)
        results.append((loss, {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}))
    print("first-step loss:", [r[0] for r in results])
    assert results[0][0] == results[1][0] == results[2][0], [r[0] for r in results]
    assert results[0][1].keys() == results[1][1].keys() and len(results[0][1]) > 40
    for k, g in results[1][1].items():
        scale = g.abs().max().item() + 1e-30
        noise = (results[2][1][k] - g).abs().max().item() / scale          # the host feed twice: the atomics alone
        diff = (results[0][1][k] - g).abs().max().item() / scale
        print(f"{k}: diff {diff:.3e} noise {noise:.3e}")
        assert diff <= max(10 * noise, 2e-5), (k, diff, noise)
    # rotation on, Adam at the default learning rate: three steps, everything stays finite
    rot_feed, _, _ = _feeds(16, 24, 8, rotate=120.0)
    assert rot_feed.scene is not None and next(iter(rot_feed))["scene_batch"]["rot"].shape[1] == 2
    m = _model(vocab)
    opt = torch.optim.Adam(m.parameters())
    crit_rec = []

    class Rec(torch.nn.Module):
        def forward(self, a, p):
            loss = crit(a, p)
            crit_rec.append(loss.detach())
            return loss
    T.train_epoch(m, rot_feed, opt, Rec(), max_batches=3)
    torch.cuda.synchronize()
    assert len(crit_rec) == 3 and all(bool(torch.isfinite(v)) for v in crit_rec)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ---- the command ------------------------------------------------------------------------------------------------------------------
def test_train_coarse_command(tmp_path):
    from text2pos_amd import io as IO, train_coarse
    base = str(tmp_path / "k360")
    IO.save_scene(base, "toy_train", *_toy_scene(16, 16, 61, scene_name="toy_train"))
    IO.save_scene(base, "toy_val", *_toy_scene(8, 8, 62, scene_name="toy_val"))
    argv = ["--base_path", base, "--scenes_train", "toy_train", "--scenes_val", "toy_val", "--epochs", "2", "--batch_size", "8",
            "--max_batches", "2", "--top_k", "1", "3", "5", "--seed", "3", "--shuffle"]
    out = train_coarse.main(argv + ["--out", str(tmp_path / "ck_dev")])
    assert len(out["loss"]) == 2 and all(np.isfinite(out["loss"])) and [len(s) for s in out["step_losses"]] == [2, 2]
    for table in (out["train_acc"], out["val_acc"], out["val_acc_close"]):
        assert len(table) == 2 and all(sorted(t) == [1, 3, 5] and all(0.0 <= v <= 1.0 for v in t.values()) for t in table)
    assert out["checkpoint"] is not None and out["checkpoint"].startswith(str(tmp_path / "ck_dev"))
    sd, args = IO.load_reference_checkpoint(out["checkpoint"], return_args=True)
    assert args["embed_dim"] == 256 and any(k.startswith("language_encoder.") for k in sd) and any("running_mean" in k for k in sd)
    assert len(list((tmp_path / "ck_dev").iterdir())) == 1            # the superseded checkpoint is gone
    host = train_coarse.main(argv + ["--out", str(tmp_path / "ck_host"), "--host_feed", "--epochs", "1", "--max_batches", "1"])
    print("first-step loss:", out["step_losses"][0][0], host["step_losses"][0][0])
    assert host["step_losses"][0][0] == out["step_losses"][0][0]
