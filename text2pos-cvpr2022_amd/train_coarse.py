"""Coarse training from on-disk KITTI360Pose scenes (the reference's training/coarse.py:170-335) on the MI355X path.

    python -m text2pos_amd.train_coarse --base_path ./data/k360_30-10_scG_pd10_pc4_spY_all/ \\
        --scenes_train 2013_05_28_drive_0000_sync ... --scenes_val 2013_05_28_drive_0010_sync --out ./checkpoints/

The training scenes are uploaded once (scene.DeviceScene with the mirror tables); every step's batch - hint shuffle, cell flips,
FixedPoints -> RandomRotate(120) -> NormalizeScale per object (training/coarse.py:192-198, dataloading/kitti360pose/cells.py:65-107)
- is packed from it by one kernel launch (training.SceneCoarseFeed, t2p_pack_scene_objects_aug); --host_feed builds the same batches
with the host chain instead.  Per epoch: training.train_epoch, then the retrieval accuracies of the training and the validation
poses (pipeline.run_coarse with the evaluation transform), the reference's progress line, and from epoch epochs // 2 on the best
model by validation accuracy at the largest k is written the reference's way (torch.save of the whole module), replacing the one
it supersedes.  Not built: --no_pc_augment, sample_close_cell, the triplet loss, plots, multi-rank training.
"""
import argparse
import copy
import os
from typing import List, Optional

import numpy as np
import torch

from . import data as D
from . import io as IO
from . import training as T
from .pipeline import PerCellTransform, _model_args, run_coarse

# datapreparation/kitti360pose/utils.py: SCENE_NAMES_TRAIN / SCENE_NAMES_VAL
SCENE_NAMES_TRAIN = ["2013_05_28_drive_0000_sync", "2013_05_28_drive_0002_sync", "2013_05_28_drive_0004_sync",
                     "2013_05_28_drive_0006_sync", "2013_05_28_drive_0007_sync"]
SCENE_NAMES_VAL = ["2013_05_28_drive_0010_sync"]


class _RecordedCriterion(torch.nn.Module):
    """The criterion, keeping every step's loss (train_epoch returns the epoch's mean only)."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.steps = inner, []

    def forward(self, anchor, positive):
        loss = self.inner(anchor, positive)
        self.steps.append(loss.detach())
        return loss


def parse_arguments(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base_path", required=True)
    ap.add_argument("--scenes_train", nargs="+", default=SCENE_NAMES_TRAIN)
    ap.add_argument("--scenes_val", nargs="+", default=SCENE_NAMES_VAL)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=16)
    ap.add_argument("--learning_rate", type=float, default=1e-3)
    ap.add_argument("--lr_gamma", type=float, default=1.0)
    ap.add_argument("--embed_dim", type=int, default=256)
    ap.add_argument("--margin", type=float, default=0.35)
    ap.add_argument("--ranking_loss", default="pairwise", choices=["pairwise", "hardest"])
    ap.add_argument("--top_k", type=int, nargs="+", default=[1, 3, 5])
    ap.add_argument("--use_features", nargs="+", default=["class", "color", "position"])
    ap.add_argument("--variation", type=int, default=0)
    ap.add_argument("--pointnet_numpoints", type=int, default=256)
    ap.add_argument("--pointnet_path", default=None, help="start from a pre-trained PointNet++ (pretrain_pointnet.py's file)")
    ap.add_argument("--pointnet_freeze", action="store_true")
    ap.add_argument("--continue_path", default=None, help="a coarse checkpoint (whole module or state_dict) to continue from")
    ap.add_argument("--shuffle", action="store_true", help="a new order of the poses every epoch")
    ap.add_argument("--no_cell_augment", action="store_true", help="no hint shuffle and no cell flips")
    ap.add_argument("--rotate_degrees", type=float, default=120.0, help="range of the per-object rotation about z")
    ap.add_argument("--max_batches", type=int, default=None, help="stop every epoch after this many steps")
    ap.add_argument("--seed", type=int, default=0, help="seed of the model's initialisation and of every draw of the feed")
    ap.add_argument("--host_feed", action="store_true", help="build the training batches with the host chain")
    ap.add_argument("--out", default="./checkpoints", help="directory the best checkpoint is written to")
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


def build_model(a, scenes_train: IO.Scenes, device):
    """training/coarse.py:261-270: a fresh model over the training scenes' vocabulary, or --continue_path's weights in one."""
    from . import CellRetrievalNetwork
    ma = _model_args(a.embed_dim, use_features=a.use_features)
    ma.variation, ma.pointnet_numpoints = a.variation, a.pointnet_numpoints
    ma.pointnet_path, ma.pointnet_freeze = a.pointnet_path, bool(a.pointnet_freeze)
    torch.manual_seed(a.seed)
    # (an evaluation in the middle of a training must not stop the run when a half-trained model leaves fp16's range)
    # (plain str words: get_known_words hands out NumPy strings, which would travel into the pickled module as NumPy scalars)
    words = [str(w) for w in scenes_train.get_known_words()]
    model = CellRetrievalNetwork(scenes_train.get_known_classes(), D.COLOR_NAMES, words, ma, on_overflow="fp32")
    if a.continue_path:
        sd, ck = IO.load_reference_checkpoint(a.continue_path, return_args=True)
        for key in ("embed_dim", "variation", "pointnet_features", "pointnet_numpoints"):
            if key in ck and ck[key] is not None and getattr(ma, key) != ck[key]:
                raise RuntimeError(f"{a.continue_path} was trained with {key}={ck[key]!r}, the command line says {getattr(ma, key)!r}")
        model.load_state_dict(sd, strict=True)
    return model.to(device)


def save_reference_style(model, path: str):
    """training/coarse.py:323-324: torch.save(model, model_path) - the whole module, on the CPU."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(copy.deepcopy(model).cpu(), path)


def main(argv: Optional[List[str]] = None) -> dict:
    from .scene import DeviceScene
    a = parse_arguments(argv)
    dev = torch.device(a.device)
    if dev.type != "cuda":
        raise RuntimeError("train_coarse: the training path is HIP; --device must be a GPU")
    torch.cuda.set_device(dev)
    train, val = IO.load_scenes(a.base_path, a.scenes_train), IO.load_scenes(a.base_path, a.scenes_val)
    print(f"train: {len(train.all_cells)} cells, {len(train.all_poses)} poses; val: {len(val.all_cells)} cells, {len(val.all_poses)} poses")
    print("Words-diff:", set(train.get_known_words()).difference(set(val.get_known_words())))
    model = build_model(a, train, dev)
    augment = not a.no_cell_augment
    scene_train = DeviceScene(train.all_cells, dev, mirror=augment and not a.host_feed)
    scene_val = DeviceScene(val.all_cells, dev)
    feed = T.SceneCoarseFeed(train, None if a.host_feed else scene_train, a.pointnet_numpoints, a.seed, a.batch_size, shuffle=a.shuffle,
                             shuffle_hints=augment, flip_poses=augment, rotate_degrees=a.rotate_degrees, host=a.host_feed)
    eval_transform = PerCellTransform(a.pointnet_numpoints, a.seed)
    optimizer = torch.optim.Adam(model.parameters(), lr=a.learning_rate)
    scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, a.lr_gamma)
    criterion = _RecordedCriterion(T.make_criterion(a))
    out = dict(loss=[], step_losses=[], train_acc=[], val_acc=[], val_acc_close=[], checkpoint=None)
    best, last_path = -1.0, None
    for epoch in range(1, a.epochs + 1):
        feed.set_epoch(epoch - 1)
        criterion.steps = []
        loss, _ = T.train_epoch(model, feed, optimizer, criterion, max_batches=a.max_batches)
        out["step_losses"].append([float(v) for v in torch.stack(criterion.steps).cpu()] if criterion.steps else [])
        model.eval()
        _, acc_t = run_coarse(model, train, eval_transform, a.top_k, [], scene_dev=scene_train)
        _, acc_v = run_coarse(model, val, eval_transform, a.top_k, [], scene_dev=scene_val)
        scheduler.step()
        train_acc, val_acc, val_close = acc_t["hit"], acc_v["hit"], acc_v["close"]
        out["loss"].append(loss)
        out["train_acc"].append(train_acc)
        out["val_acc"].append(val_acc)
        out["val_acc_close"].append(val_close)
        line = f"\t lr {a.learning_rate:0.4} loss {loss:0.2f} epoch {epoch} train-acc: "
        line += "".join(f"{k}-{v:0.2f} " for k, v in train_acc.items())
        line += "val-acc: " + "".join(f"{k}-{v:0.2f} " for k, v in val_acc.items())
        line += "val-acc-close: " + "".join(f"{k}-{v:0.2f} " for k, v in val_close.items())
        print(line + "\n", flush=True)
        if epoch >= a.epochs // 2:      # the best model, with early stopping (training/coarse.py:314-335)
            acc = val_acc[max(a.top_k)]
            if acc > best:
                path = os.path.join(a.out, f"coarse_cont{'Y' if a.continue_path else 'N'}_acc{acc:0.2f}_p{a.pointnet_numpoints}"
                                           f"_nca{int(a.no_cell_augment)}.pth")
                print(f"Saving model at {acc:0.2f} to {path}")
                save_reference_style(model, path)
                if last_path is not None and last_path != path and os.path.isfile(last_path):
                    print("Removing", last_path)
                    os.remove(last_path)
                best, last_path = acc, path
    out["checkpoint"] = last_path
    return out


if __name__ == "__main__":
    main()
