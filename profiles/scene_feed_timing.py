# What the input side of a coarse training step costs, one JSON line per route: milliseconds per step of training.train_epoch (batch
# built + forward + loss + backward + Adam, wall clock around a drained device) and the share of it spent building the batch, on
#   (a) the host-twin feed - per item flip_cell copies + one Data -> FixedPoints -> RotateZ -> NormalizeScale chain per object + the
#       float64 means of encode_objects: the route the reference's dataloader takes, and the only one there was before SceneCoarseFeed;
#   (b) the device feed - the batch packed from the resident scene by t2p_pack_scene_objects_aug, same seed, same draws.
# One synthetic raw scene: 512 cells of 6-20 objects with 30-3,000 points, 512 poses; batch 64, warm-up steps first, median of --steps.
# python profiles/scene_feed_timing.py [--steps 20] [--warmup 3]
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import weights as W  # noqa: E402
import text2pos_amd as t2p  # noqa: E402
from text2pos_amd import data as D, io as IO, synthetic as S, training as T  # noqa: E402
from text2pos_amd.scene import DeviceScene  # noqa: E402


def raw_scene(n_cells=512, n_poses=512, seed=20220091):
    rng = np.random.default_rng(seed)
    cells, poses = [], []
    for i in range(n_cells):
        objs = []
        for j in range(int(rng.integers(6, 21))):
            n = int(rng.integers(30, 3001))
            c = rng.random(3) * np.array([1.0, 1.0, 0.3])
            objs.append(D.Object3d(j, 1000 * i + j, c + 0.05 * rng.standard_normal((n, 3)),
                                   np.clip(rng.random(3) + 0.05 * rng.standard_normal((n, 3)), 0, 1),
                                   S.LABELS[int(rng.integers(0, len(S.LABELS)))]))
        x, y = 30.0 * (i % 32), 30.0 * (i // 32)
        cells.append(D.Cell(i, "synth", objs, 30.0, np.array([x, y, 0.0, x + 30.0, y + 30.0, 10.0])))
    for q in range(n_poses):
        c = cells[q % n_cells]
        descs = [D.DescriptionBestCell(S.DIRECTIONS[int(rng.integers(0, 5))], o.get_color_text(), o.label, o.id, True)
                 for o in [c.objects[int(k)] for k in rng.choice(len(c.objects), 6, replace=False)]]
        poses.append(D.Pose(rng.random(3), c.bbox_w[0:3] + rng.random(3) * 30.0, c.id, "synth", descs))
    return cells, poses


class _OneBatch(list):
    """A one-batch loader that hands train_epoch the scene, as the feed does."""
    scene = None


def run(feed, steps, warmup, dev):
    model = t2p.CellRetrievalNetwork(S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words(), S.default_args())
    W.fill_state_dict(model, 37)
    model = model.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = T.make_criterion(S.default_args(margin=0.35, ranking_loss="pairwise"))
    feed_ms, step_ms, losses = [], [], []
    epoch, it = 0, None
    for i in range(warmup + steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        batch = next(it, None) if it is not None else None
        if batch is None:
            feed.set_epoch(epoch)
            epoch += 1
            it = iter(feed)
            t0 = time.perf_counter()
            batch = next(it)
        t1 = time.perf_counter()
        one = _OneBatch([batch])
        one.scene = feed.scene
        loss, _ = T.train_epoch(model, one, opt, crit)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        if i >= warmup:
            feed_ms.append(1e3 * (t1 - t0))
            step_ms.append(1e3 * (t2 - t0))
        losses.append(loss)
    med = lambda v: round(float(np.median(v)), 3)
    return dict(step_ms=med(step_ms), step_min_ms=round(min(step_ms), 3), step_max_ms=round(max(step_ms), 3), feed_ms=med(feed_ms),
                feed_share=round(float(np.median(feed_ms)) / float(np.median(step_ms)), 4), steps=steps, first_loss=losses[0],
                last_loss=losses[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    cells, poses = raw_scene()
    scenes = IO.Scenes(cells, poses)
    t1 = time.perf_counter()
    scene = DeviceScene(cells, dev, mirror=True)
    torch.cuda.synchronize(dev)
    print(json.dumps(dict(what="scene", cells=len(cells), objects=scene.n_objects, raw_points=int(scene.rows.sum()),
                          generate_s=round(t1 - t0, 2), upload_with_mirror_s=round(time.perf_counter() - t1, 2))), flush=True)
    for what, host in (("(a) host-twin feed", True), ("(b) device feed", False)):
        feed = T.SceneCoarseFeed(scenes, scene, 256, 3, a.batch, host=host)
        r = run(feed, a.steps, a.warmup, dev)
        print(json.dumps(dict(what=what + ": train_epoch step incl. batch construction", batch=a.batch, **r)), flush=True)


if __name__ == "__main__":
    main()
