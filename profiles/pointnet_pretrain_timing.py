# Stage-one (PointNet++ pre-training) timings on one GPU, one JSON line each: milliseconds per classifier training step
# (forward, cross-entropy, backward, Adam) at batch 32 and 512, next to the coarse cell branch's encode_objects_train + backward on the
# same objects in a few cells (the same trunk: the nearest thing the coarse stage has; two cells of 16 / four of 128 - one cell would leave the
# cell head's BatchNorm a single row, which train() refuses as nn.BatchNorm1d does, and t2p_knn takes cells of up to 192 objects), and objects/s of val_pointnet_epoch at batch 512
# on both arithmetic paths.  Device events around synchronised work, warm-up first, median of --steps.
# python profiles/pointnet_pretrain_timing.py [--steps 20] [--warmup 5]
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import weights as W  # noqa: E402
import pretrain_pointnet as PP  # noqa: E402
import text2pos_amd as t2p  # noqa: E402
from text2pos_amd import synthetic as S, training as T  # noqa: E402


def timed(fn, steps, warmup, dev):
    """Median / min / max milliseconds of fn() between two device events; the stream is drained before the first event."""
    ms = []
    for i in range(warmup + steps):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    classes, colors, words = S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words()
    for batch in (32, 512):
        b = PP.object_batch(PP.TRAIN_SEED, 0, batch)
        xyz, rgb = (t.view(batch, 256, 3).to(dev) for t in (b.pos, b.x))
        y = b.y.to(dev)
        # -- the classifier step as train_pointnet_epoch runs it (host-resident batch, loss.item() included)
        model = PP.fresh_model()
        opt = torch.optim.Adam(model.parameters(), lr=10 ** -2.5)
        crit = t2p.CrossEntropyLoss()
        r = timed(lambda: T.train_pointnet_epoch(model, [b], opt, crit), a.steps, a.warmup, dev)
        print(json.dumps(dict(what="train_pointnet_epoch, one batch", batch=batch, **r)), flush=True)

        # -- the same arithmetic on device-resident inputs
        def step():
            opt.zero_grad()
            loss = crit(model.forward_packed(xyz, rgb).class_pred, y)
            loss.backward()
            opt.step()
        model.train()
        r = timed(step, a.steps, a.warmup, dev)
        print(json.dumps(dict(what="classifier step, device-resident inputs", batch=batch, **r)), flush=True)
        # -- orientation: the coarse cell branch in train() on the same objects in cells of min(batch / 2, 128), forward + backward + Adam
        cm = t2p.CellRetrievalNetwork(classes, colors, words, S.default_args())
        W.fill_state_dict(cm, 23)
        cm = cm.to(dev).train()
        copt = torch.optim.Adam(cm.parameters(), lr=1e-3)
        center = torch.rand(batch, 3, device=dev)
        mean_rgb = rgb.mean(1)
        cell_ptr = np.arange(0, batch + 1, min(batch // 2, 128))
        coef = torch.randn(len(cell_ptr) - 1, 256, device=dev)

        def cell_step():
            copt.zero_grad()
            (cm.encode_objects_packed(xyz, rgb, center, mean_rgb, cell_ptr) * coef).sum().backward()
            copt.step()
        r = timed(cell_step, a.steps, a.warmup, dev)
        print(json.dumps(dict(what="encode_objects_train on the same objects + backward + Adam", batch=batch, cells=len(cell_ptr) - 1, **r)), flush=True)
        del cm, copt
    # -- validation throughput at batch 512
    val = PP.batches(PP.VAL_SEED, 4096, 512)
    for precision in ("f16x3", "fp32"):
        model = PP.fresh_model(precision)
        W.fill_state_dict(model, 11)             # (golden weights: inside the f16x3 range, no fp32 recomputation in the figure)
        r = timed(lambda: T.val_pointnet_epoch(model, val), max(3, a.steps // 4), 2, dev)
        print(json.dumps(dict(what="val_pointnet_epoch, 8 host-resident batches of 512", precision=precision,
                              objects_per_s=round(4096 / (r["median_ms"] * 1e-3)), **r)), flush=True)
        dval = [tuple(t.view(512, 256, 3).to(dev) for t in (b.pos, b.x)) for b in val]
        model.eval()

        def fwd():
            with torch.no_grad():
                for xyz_, rgb_ in dval:
                    model.forward_packed(xyz_, rgb_)
        r = timed(fwd, max(3, a.steps // 4), 2, dev)
        print(json.dumps(dict(what="eval forward_packed, 8 device-resident batches of 512", precision=precision,
                              objects_per_s=round(4096 / (r["median_ms"] * 1e-3)), **r)), flush=True)


if __name__ == "__main__":
    main()
