"""GPU side of the fine stage's training feed (-m gpu): SuperGlueMatch.forward_scene_batch on training.SceneFineFeed's device
batches against forward() on the host-twin batches, training.train_fine_epoch / val_fine_epoch on both kinds of batch,
training.fine_conf_score and the train_fine command.  Small model throughout: embed_dim 128, one layer pair, 32 points per object,
pad_size 5, 6 hints, 3 or 4 samples.  The host side is tests/test_fine_feed_host.py, the statistics kernel alone
tests/test_gpu_fine_stats.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fine_scene import make_fine_scene  # noqa: E402

pytestmark = pytest.mark.gpu
PAD, HINTS, N_PTS = 5, 6, 32
SCENE_SEED, WEIGHT_SEED = 41, 14          # (the untrained loss of this pair is finite: asserted through skipped_steps below)
STAT_KEYS = ("recall", "precision", "pose_mid", "pose_mean", "pose_offsets")


def _dev():
    return torch.device("cuda:0")


def _model(vocab, seed=WEIGHT_SEED):
    import weights as W
    import text2pos_amd as t2p
    from text2pos_amd.pipeline import _model_args
    args = _model_args(128, num_layers=1, sinkhorn_iters=50)
    args.pointnet_numpoints = N_PTS
    m = t2p.SuperGlueMatch(vocab["classes"], vocab["colors"], vocab["words"], args)
    W.fill_state_dict(m, seed)
    return m.to(_dev())


def _feeds(n_cells, n_poses, batch, rotate=None, seed=5, scene_seed=SCENE_SEED, **kw):
    from text2pos_amd import io as IO, training as T
    from text2pos_amd.scene import DeviceScene
    cells, poses = make_fine_scene(n_cells, n_poses, scene_seed, PAD, HINTS, lo_pts=20, hi_pts=60)
    scenes = IO.Scenes(cells, poses)
    sc = DeviceScene(cells, _dev(), n_pad=PAD, pad_seed=seed)
    mk = lambda host: T.SceneFineFeed(scenes, sc, N_PTS, seed, batch, pad_size=PAD, num_mentioned=HINTS, rotate_degrees=rotate,
                                      host=host, **kw)
    return mk(False), mk(True), sc


def _stat_bar(feed, offsets_max):
    """64 * 2^-53 * (1 + max|centre| + max|offset| + |pose|): tests/test_gpu_fine_stats.py's derivation."""
    centre = np.abs(feed.scene.center64[:, 0:2]).max()
    return 64 * 2.0 ** -53 * (1.0 + centre + offsets_max + np.abs(feed.pose_xy).max())


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def test_forward_scene_batch_is_forward_on_the_host_twin(vocab):
    dev_feed, host_feed, sc = _feeds(5, 8, 4)
    bd, bh = next(iter(dev_feed)), next(iter(host_feed))
    assert bd["hint_descriptions"] == bh["hint_descriptions"] and bd["scene_batch"]["rot"] is None
    assert any(o.label == "pad" for objs in bh["objects"] for o in objs)                  # padding slots are in the batch
    m1, m2 = _model(vocab), _model(vocab)
    m1.train(), m2.train()
    with torch.no_grad():
        a, inputs = m1.forward_scene_batch(sc, bd["scene_batch"], bd["hint_descriptions"], want_inputs=True)
        b = m2(bh["objects"], bh["hint_descriptions"], bh["object_points"])
    torch.cuda.synchronize()
    assert torch.equal(inputs[0].cpu().view(-1, 3), torch.cat([p.pos for p in bh["object_points"]]))      # the packed xyz
    assert tuple(a.P.shape) == (4, PAD + 1, HINTS + 1) and tuple(a.matches0.shape) == (4, PAD)
    for k in ("P", "offsets", "matches0", "matches1"):
        assert torch.equal(a[k], b[k]), k
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    moved = 0
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
        moved += int("running_mean" in k)
    assert moved > 0
    m1.eval(), m2.eval()
    with torch.no_grad():
        a = m1.forward_scene_batch(sc, bd["scene_batch"], bd["hint_descriptions"])
        b = m2(bh["objects"], bh["hint_descriptions"], bh["object_points"])
    for k in ("P", "offsets", "matches0", "matches1"):
        assert torch.equal(a[k], b[k]), k
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    with pytest.raises(NotImplementedError):
        m1.forward_scene_batch(sc, bd["scene_batch"], bd["hint_descriptions"])            # eval() with autograd: forward-only, as before
    m1.train()
    with pytest.raises(NotImplementedError):
        m1.forward_scene_batch(sc, bd["scene_batch"], bd["hint_descriptions"])            # train() with autograd outside fine_backward()
    with pytest.raises(NotImplementedError, match="flips"):
        with torch.no_grad():
            m1.forward_scene_batch(sc, dict(bd["scene_batch"], flip=np.zeros(4 * PAD, np.uint8)), bd["hint_descriptions"])


def test_forward_scene_batch_with_rotation(vocab):
    """What the pack kernel guarantees with a rotation (tests/test_gpu_scene_feed.py::test_rotation): the host twin's RotateZ ->
    NormalizeScale to 2e-6 on the normalised points, everything else of the packed inputs bit for bit.  No more is asserted."""
    dev_feed, host_feed, sc = _feeds(5, 8, 4, rotate=120.0)
    plain_feed, _, _ = _feeds(5, 8, 4, rotate=None)
    bd, bh, bp = next(iter(dev_feed)), next(iter(host_feed)), next(iter(plain_feed))
    assert bd["scene_batch"]["rot"].shape == (4 * PAD, 2)
    m = _model(vocab).train()
    with torch.no_grad():
        out, inputs = m.forward_scene_batch(sc, bd["scene_batch"], bd["hint_descriptions"], want_inputs=True)
        _, plain = m.forward_scene_batch(sc, bp["scene_batch"], bp["hint_descriptions"], want_inputs=True)
    torch.cuda.synchronize()
    want = torch.cat([p.pos for p in bh["object_points"]])
    assert (inputs[0].cpu().view(-1, 3) - want).abs().max().item() < 2e-6
    assert (inputs[0] - plain[0]).abs().max().item() > 1e-2                                # (it did rotate)
    assert torch.equal(inputs[1].cpu().view(-1, 3), torch.cat([p.x for p in bh["object_points"]]))
    assert torch.equal(inputs[2], plain[2]) and torch.equal(inputs[3], plain[3])           # centres and colours do not turn
    assert torch.isfinite(out.P).all() and torch.isfinite(out.offsets).all()
    assert int(out.matches0.min()) >= -1 and int(out.matches0.max()) < HINTS


# ---- one training step ------------------------------------------------------------------------------------------------------------
def test_train_fine_epoch_on_the_device_feed(vocab):
    from text2pos_amd import training as T
    dev_feed, host_feed, sc = _feeds(5, 8, 4)
    results = []
    for feed in (dev_feed, host_feed, host_feed):
        m = _model(vocab)
        opt = torch.optim.SGD(m.parameters(), lr=0.0)      # (the step leaves parameters and gradients as backward() left them)
        feed.set_epoch(0)
        steps = []
        stats = T.train_fine_epoch(m, feed, opt, max_batches=1, step_losses=steps)
        torch.cuda.synchronize()
        assert set(stats) == set(T.FINE_TRAIN_KEYS) | {"skipped_steps"} and stats["skipped_steps"] == 0 and steps == [stats["loss"]]
        assert np.isfinite(stats["loss"]) and np.isfinite(stats["loss_offsets"])
        results.append((stats, {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}))
    print("first-step loss:", [(r[0]["loss"], r[0]["loss_offsets"]) for r in results])
    assert results[0][0]["loss"] == results[1][0]["loss"] == results[2][0]["loss"]
    assert results[0][0]["loss_offsets"] == results[1][0]["loss_offsets"] == results[2][0]["loss_offsets"]
    assert results[0][1].keys() == results[1][1].keys() and len(results[0][1]) > 40
    for k, g in results[1][1].items():
        scale = g.abs().max().item() + 1e-30
        noise = (results[2][1][k] - g).abs().max().item() / scale          # the host feed twice: the atomics alone
        diff = (results[0][1][k] - g).abs().max().item() / scale
        print(f"{k}: diff {diff:.3e} noise {noise:.3e}")
        assert diff <= max(10 * noise, 2e-5), (k, diff, noise)
    # the five statistics of the device step against fine_batch_stats on the host batch (the host run's)
    m = _model(vocab).train()
    with torch.no_grad():
        bd = dev_feed.batch(dev_feed.epoch_order(0)[:4], 0)
        off_max = float(m.forward_scene_batch(sc, bd["scene_batch"], bd["hint_descriptions"]).offsets.abs().max())
    bar = _stat_bar(dev_feed, off_max)
    for k in STAT_KEYS:
        print(f"{k}: device {results[0][0][k]!r} host {results[1][0][k]!r} (bar {bar:.3e})")
        assert abs(results[0][0][k] - results[1][0][k]) <= bar, k
    assert results[0][0]["recall"] == results[1][0]["recall"] and results[0][0]["precision"] == results[1][0]["precision"]


def test_three_adam_steps_with_rotation(vocab):
    from text2pos_amd import training as T
    rot_feed, _, _ = _feeds(5, 12, 4, rotate=120.0)
    m = _model(vocab)
    opt = torch.optim.Adam(m.parameters())
    steps = []
    stats = T.train_fine_epoch(m, rot_feed, opt, max_batches=3, step_losses=steps)
    torch.cuda.synchronize()
    print("losses:", steps)
    assert len(steps) == 3 and all(np.isfinite(v) for v in steps) and stats["skipped_steps"] == 0
    assert all(np.isfinite(stats[k]) for k in T.FINE_TRAIN_KEYS)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ---- validation, confidence -------------------------------------------------------------------------------------------------------
def test_val_fine_epoch_on_the_device_feed(vocab):
    from text2pos_amd import training as T
    dev_feed, host_feed, sc = _feeds(5, 7, 3)                 # batches of 3, 3 and 1
    m1, m2 = _model(vocab).train(), _model(vocab).train()
    a, b = T.val_fine_epoch(m1, dev_feed), T.val_fine_epoch(m2, host_feed)
    assert m1.training and sorted(a) == sorted(STAT_KEYS) == sorted(b)
    m3 = _model(vocab).train()
    with torch.no_grad():
        off_max = max(float(m3.forward_scene_batch(sc, bd["scene_batch"], bd["hint_descriptions"]).offsets.abs().max()) for bd in dev_feed)
    bar = _stat_bar(dev_feed, off_max)
    for k in STAT_KEYS:
        print(f"{k}: device {a[k]!r} host {b[k]!r} (bar {bar:.3e})")
        assert np.isfinite(a[k]) and abs(a[k] - b[k]) <= bar, k
    # an explicit scene argument is the feed's
    again = T.val_fine_epoch(_model(vocab).train(), list(dev_feed), scene=sc)
    assert again == a
    with pytest.raises(RuntimeError, match="scene"):
        T.val_fine_epoch(_model(vocab).train(), list(dev_feed))


def test_fine_conf_score(vocab):
    from text2pos_amd import training as T
    dev_feed, host_feed, _ = _feeds(5, 8, 4)
    m = _model(vocab).train()
    with pytest.raises(NotImplementedError, match="train"):
        T.fine_conf_score(m, dev_feed, n_trials=2)
    m.eval()
    a = T.fine_conf_score(m, dev_feed, n_trials=6, seed=3)
    b = T.fine_conf_score(m, dev_feed, n_trials=6, seed=3)
    h = T.fine_conf_score(m, host_feed, n_trials=6, seed=3)
    print("conf score:", a, h)
    assert len(a) == 2 and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in a) and a == b == h


# ---- the command ------------------------------------------------------------------------------------------------------------------
def test_train_fine_command(tmp_path):
    from text2pos_amd import io as IO, train_fine, training as T
    base = str(tmp_path / "k360")
    IO.save_scene(base, "toy_train", *make_fine_scene(5, 12, SCENE_SEED, PAD, HINTS, scene_name="toy_train", lo_pts=20, hi_pts=60))
    IO.save_scene(base, "toy_val", *make_fine_scene(3, 6, SCENE_SEED + 1, PAD, HINTS, scene_name="toy_val", lo_pts=20, hi_pts=60))
    argv = ["--base_path", base, "--scenes_train", "toy_train", "--scenes_val", "toy_val", "--epochs", "2", "--batch_size", "4",
            "--max_batches", "2", "--pad_size", str(PAD), "--num_layers", "1", "--pointnet_numpoints", str(N_PTS), "--seed", "3"]
    out = train_fine.main(argv + ["--out", str(tmp_path / "ck_dev")])
    for k in T.FINE_TRAIN_KEYS:
        assert len(out["train"][k]) == 2 and all(np.isfinite(out["train"][k])), k
    for k in T.FINE_VAL_KEYS:
        assert len(out["val"][k]) == 2 and all(np.isfinite(out["val"][k])), k
    assert [len(s) for s in out["step_losses"]] == [2, 2] and out["skipped_steps"] == [0, 0]
    assert out["checkpoint"] is not None and out["checkpoint"].startswith(str(tmp_path / "ck_dev")) and os.path.isfile(out["checkpoint"])
    sd, args = IO.load_reference_checkpoint(out["checkpoint"], return_args=True)
    assert args["num_layers"] == 1 and args["embed_dim"] == 128 and args["pad_size"] == PAD
    assert any(k.startswith("superglue.gnn.") for k in sd) and any("running_mean" in k for k in sd)
    assert len(list((tmp_path / "ck_dev").iterdir())) == 1            # exactly one file
    host = train_fine.main(argv + ["--out", str(tmp_path / "ck_host"), "--host_feed", "--epochs", "1", "--max_batches", "1"])
    print("first-step loss:", out["step_losses"][0][0], host["step_losses"][0][0])
    assert host["step_losses"][0][0] == out["step_losses"][0][0]
