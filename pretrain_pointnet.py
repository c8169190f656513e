#!/usr/bin/env python
"""pretrain_pointnet.py -- stage one of the reference's training: PointNet++ pre-trained as an object classifier.

The reference trains in three stages; the first (training/pointcloud/pointnet2.py) trains models/pointcloud/pointnet2.py::PointNet2
to classify single objects and writes `torch.save(model.state_dict(), path)` (:158).  Every ObjectEncoder of the later stages loads
that file (models/object_encoder.py:46, `args.pointnet_path`).  This script is that loop on the HIP path
(text2pos_amd.training.train_pointnet_epoch / val_pointnet_epoch): Adam at lr = np.logspace(-2, -4, 5)[lr_idx] (:116, :133),
nn.CrossEntropyLoss -> text2pos_amd.CrossEntropyLoss (:134), ExponentialLR(lr_gamma) stepped per epoch (:135, :147), batches of 32
(training/args.py:12), the checkpoint of the best validation accuracy of the second half of the epochs kept (:154-159).
KITTI360Pose is not available, so the objects are synthetic (synthetic.make_objects) and the label is the generator's shape
class (synthetic.object_attributes: planar patch / pole / box surface) - a task the geometry alone decides.

    python pretrain_pointnet.py --out pointnet_pretrained.pth          # needs cuda:0 (the training path is HIP)

The file it writes is what `args.pointnet_path` names: CellRetrievalNetwork(..., args) with args.pointnet_path = that file starts
from the pre-trained trunk (and with args.pointnet_freeze keeps it fixed), as the reference's coarse and fine stages do;
`train_checkpoint.py --pointnet-path` is the coarse stage of this repository started that way.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TRAIN_SEED = 20220177      # the training objects' stream
VAL_SEED = 20220178        # held-out objects
NUM_CLASSES, NUM_COLORS = 22, 8    # the reference's heads (KITTI360Pose: 22 classes, 8 colour names); labels 0-2 are used
DEFAULTS = dict(epochs=4, batch=32, train_objects=2048, val_objects=512, lr_idx=1, lr_gamma=1.0, numpoints=256)


def object_batch(seed, lo, hi, n_pts=256):
    """Objects [lo, hi) of the `seed` stream as ONE batch in the shape the reference's DataLoader hands to the loop
    (torch_geometric Batch of Kitti360ObjectsDataset items): .x (rgb), .pos, .batch, .y (class index)."""
    import torch
    from text2pos_amd import data as D, synthetic as S
    xyz, rgb, _, _ = S.make_objects(seed, lo, hi, n_pts)
    shape, _, _ = S.object_attributes(seed, lo, hi)
    b = D.Batch(x=torch.from_numpy(rgb.reshape(-1, 3)), pos=torch.from_numpy(xyz.reshape(-1, 3)),
                batch=torch.arange(hi - lo).repeat_interleave(n_pts))
    b.y = torch.from_numpy(shape.astype(np.int64))
    return b


def batches(seed, n_objects, batch, n_pts=256):
    return [object_batch(seed, lo, min(lo + batch, n_objects), n_pts) for lo in range(0, n_objects, batch)]


def fresh_model(precision="f16x3", device="cuda:0", numpoints=256):
    import torch
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    torch.manual_seed(4321)
    return t2p.PointNet2(NUM_CLASSES, NUM_COLORS, S.default_args(pointnet_numpoints=numpoints), precision=precision,
                         on_overflow="fp32").to(device)   # (a barely trained trunk may leave the f16x3 range: recompute, do not stop)


def pretrain(model, path=None, epochs=DEFAULTS["epochs"], batch=DEFAULTS["batch"], train_objects=DEFAULTS["train_objects"],
             val_objects=DEFAULTS["val_objects"], lr_idx=DEFAULTS["lr_idx"], lr_gamma=DEFAULTS["lr_gamma"], max_batches=None,
             log=None):
    """training/pointcloud/pointnet2.py:125-159 for one learning rate.  Writes the state_dict of the best validation accuracy
    among the epochs from epochs // 2 on to `path` (when given).  Returns the per-epoch records."""
    import torch
    import text2pos_amd as t2p
    from text2pos_amd import training as T
    n_pts = int(getattr(model.args, "pointnet_numpoints", 256))
    train_b = batches(TRAIN_SEED, train_objects, batch, n_pts)
    val_b = batches(VAL_SEED, val_objects, batch, n_pts)
    lr = float(np.logspace(-2, -4.0, 5)[lr_idx])
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    criterion = t2p.CrossEntropyLoss()
    scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, lr_gamma)
    rng = np.random.default_rng(TRAIN_SEED)
    records, best = [], -1.0
    for epoch in range(epochs):
        order = rng.permutation(len(train_b))          # --shuffle
        loss, acc_train = T.train_pointnet_epoch(model, [train_b[i] for i in order], optimizer, criterion, max_batches)
        acc_val = T.val_pointnet_epoch(model, val_b)
        scheduler.step()
        records.append(dict(epoch=epoch, loss=round(loss, 4), acc_train=round(acc_train, 4), acc_val=round(acc_val, 4)))
        if log:
            log(f"\t lr {lr:0.6f} epoch {epoch} loss {loss:0.3f} acc-train {acc_train:0.2f} acc-val {acc_val:0.2f}")
        if epoch >= epochs // 2 and acc_val > best and path is not None:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            torch.save(model.state_dict(), path)                     # training/pointcloud/pointnet2.py:158
            best = acc_val
    return records


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "pointnet_pretrained.pth"),
                    help="where the state_dict goes: the file args.pointnet_path names")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "fp32"], help="arithmetic of the validation passes")
    ap.add_argument("--max-batches", type=int, default=None, help="training/args.py:14")
    for k, v in DEFAULTS.items():
        ap.add_argument("--" + k.replace("_", "-"), type=type(v), default=v)
    args = ap.parse_args()
    log = lambda m: print(m, file=sys.stderr, flush=True)
    model = fresh_model(args.precision, numpoints=args.numpoints)
    t0 = time.perf_counter()
    records = pretrain(model, args.out, max_batches=args.max_batches, log=log,
                       **{k: getattr(args, k) for k in DEFAULTS if k != "numpoints"})
    print(json.dumps(dict(out=args.out, train_s=round(time.perf_counter() - t0, 1), epochs=records,
                          bytes=os.path.getsize(args.out) if os.path.exists(args.out) else None)))


if __name__ == "__main__":
    main()
