"""Fine training from on-disk KITTI360Pose scenes (the reference's training/fine.py:211-378) on the MI355X path.

    python -m text2pos_amd.train_fine --base_path ./data/k360_30-10_scG_pd10_pc4_spY_all/ \\
        --scenes_train 2013_05_28_drive_0000_sync ... --scenes_val 2013_05_28_drive_0010_sync --out ./checkpoints/

The training and the validation scenes are uploaded once (scene.DeviceScene with pad_size padding objects); every step's batch - the
pose's cell with the matched objects first, cut or padded to pad_size, FixedPoints -> RandomRotate(120) -> NormalizeScale per object
(training/fine.py:228-239, dataloading/kitti360pose/poses.py:32-174) - is packed from it by one kernel launch, the targets are
gathers of tables resident on the device and the step's statistics come from one launch and one 56-byte copy
(training.SceneFineFeed, training.train_fine_epoch, t2p_fine_step_stats); --host_feed builds the same batches with the host chain and
takes the loop's host path.  The reference's schedule: Adam at 1e-5 for epochs 0-2, a fresh Adam at the chosen rate from epoch 3,
ExponentialLR per epoch, validation after every epoch in the mode the training left the model in, and from epoch epochs // 2 on the
best model by mean(recall, precision) on validation is written the reference's way (torch.save of the whole module), replacing the one
it supersedes.  Not built: --no_pc_augment, flips, plots, multi-rank training.
"""
import argparse
import os
from typing import List, Optional

import numpy as np
import torch

from . import data as D
from . import io as IO
from . import training as T
from .pipeline import _model_args
from .train_coarse import SCENE_NAMES_TRAIN, SCENE_NAMES_VAL, save_reference_style


def parse_arguments(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base_path", required=True)
    ap.add_argument("--scenes_train", nargs="+", default=SCENE_NAMES_TRAIN)
    ap.add_argument("--scenes_val", nargs="+", default=SCENE_NAMES_VAL)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=16)
    ap.add_argument("--learning_rate", type=float, default=1e-3)
    ap.add_argument("--lr_idx", type=int, default=None, help="pick the rate from logspace(-3, -4, 3) (training/fine.py:276-279)")
    ap.add_argument("--lr_gamma", type=float, default=1.0)
    ap.add_argument("--embed_dim", type=int, default=128)
    ap.add_argument("--num_layers", type=int, default=6)
    ap.add_argument("--sinkhorn_iters", type=int, default=50)
    ap.add_argument("--num_mentioned", type=int, default=6)
    ap.add_argument("--pad_size", type=int, default=16)
    ap.add_argument("--regressor_cell", default="pose", choices=list(T.REGRESSOR_CELLS))
    ap.add_argument("--regressor_learn", default="center", choices=list(T.REGRESSOR_LEARNS))
    ap.add_argument("--use_features", nargs="+", default=["class", "color", "position"])
    ap.add_argument("--variation", type=int, default=0)
    ap.add_argument("--class_embed", action="store_true")
    ap.add_argument("--color_embed", action="store_true")
    ap.add_argument("--pointnet_numpoints", type=int, default=256)
    ap.add_argument("--pointnet_path", default=None, help="start from a pre-trained PointNet++ (pretrain_pointnet.py's file)")
    ap.add_argument("--pointnet_freeze", action="store_true")
    ap.add_argument("--continue_path", default=None, help="a fine checkpoint (whole module or state_dict) to continue from")
    ap.add_argument("--shuffle", action="store_true", help="a new order of the poses every epoch")
    ap.add_argument("--rotate_degrees", type=float, default=120.0, help="range of the per-object rotation about z")
    ap.add_argument("--max_batches", type=int, default=None, help="stop every training epoch after this many steps")
    ap.add_argument("--seed", type=int, default=0, help="seed of the model's initialisation and of every draw of the feeds")
    ap.add_argument("--host_feed", action="store_true", help="build the batches with the host chain")
    ap.add_argument("--out", default="./checkpoints", help="directory the best checkpoint is written to")
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


def build_model(a, scenes_train: IO.Scenes, device):
    """training/fine.py:300-309: a fresh SuperGlueMatch over the training scenes' vocabulary (the classes with "pad", as
    train_coarse.build_model and pipeline take them), or --continue_path's weights in one."""
    from . import SuperGlueMatch
    ma = _model_args(a.embed_dim, a.num_layers, a.sinkhorn_iters, a.use_features)
    ma.variation, ma.class_embed, ma.color_embed = a.variation, bool(a.class_embed), bool(a.color_embed)
    ma.pointnet_numpoints, ma.pointnet_path, ma.pointnet_freeze = a.pointnet_numpoints, a.pointnet_path, bool(a.pointnet_freeze)
    ma.num_mentioned, ma.pad_size = a.num_mentioned, a.pad_size
    ma.regressor_cell, ma.regressor_learn = a.regressor_cell, a.regressor_learn
    torch.manual_seed(a.seed)
    words = [str(w) for w in scenes_train.get_known_words()]     # (plain str: see train_coarse.build_model)
    model = SuperGlueMatch(scenes_train.get_known_classes(), D.COLOR_NAMES, words, ma)
    if a.continue_path:
        sd, ck = IO.load_reference_checkpoint(a.continue_path, return_args=True)
        for key in ("embed_dim", "num_layers", "variation", "pointnet_features", "pointnet_numpoints"):
            if key in ck and ck[key] is not None and getattr(ma, key) != ck[key]:
                raise RuntimeError(f"{a.continue_path} was trained with {key}={ck[key]!r}, the command line says {getattr(ma, key)!r}")
        model.load_state_dict(sd, strict=True)
    return model.to(device)


def main(argv: Optional[List[str]] = None) -> dict:
    from .scene import DeviceScene
    a = parse_arguments(argv)
    dev = torch.device(a.device)
    if dev.type != "cuda":
        raise RuntimeError("train_fine: the training path is HIP; --device must be a GPU")
    torch.cuda.set_device(dev)
    train, val = IO.load_scenes(a.base_path, a.scenes_train), IO.load_scenes(a.base_path, a.scenes_val)
    print(f"train: {len(train.all_cells)} cells, {len(train.all_poses)} poses; val: {len(val.all_cells)} cells, {len(val.all_poses)} poses")
    print("Words-diff:", set(train.get_known_words()).difference(set(val.get_known_words())))
    model = build_model(a, train, dev)
    lr = float(np.logspace(-3.0, -4.0, 3)[a.lr_idx]) if a.lr_idx is not None else a.learning_rate
    scene_of = lambda s: None if a.host_feed else DeviceScene(s.all_cells, dev, n_pad=a.pad_size, pad_seed=a.seed)
    feed_kw = dict(n_pts=a.pointnet_numpoints, seed=a.seed, batch_size=a.batch_size, pad_size=a.pad_size, num_mentioned=a.num_mentioned,
                   regressor_cell=a.regressor_cell, regressor_learn=a.regressor_learn, host=a.host_feed, pad_seed=a.seed)
    feed = T.SceneFineFeed(train, scene_of(train), shuffle=a.shuffle, rotate_degrees=a.rotate_degrees, **feed_kw)
    feed_val = T.SceneFineFeed(val, scene_of(val), shuffle=False, rotate_degrees=None, **feed_kw)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-5)           # warm-up (training/fine.py:316-323)
    scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, a.lr_gamma)
    out = dict(train={k: [] for k in T.FINE_TRAIN_KEYS}, val={k: [] for k in T.FINE_VAL_KEYS}, step_losses=[], skipped_steps=[],
               conf=[], checkpoint=None)
    cont, feats = "Y" if a.continue_path else "N", "all" if len(a.use_features) == 3 else "-".join(a.use_features)
    best, last_path = -1.0, None
    for epoch in range(a.epochs):
        if epoch == 3:
            optimizer = torch.optim.Adam(model.parameters(), lr=lr)
            scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, a.lr_gamma)
        feed.set_epoch(epoch)
        steps = []
        train_out = T.train_fine_epoch(model, feed, optimizer, max_batches=a.max_batches, step_losses=steps)
        val_out = T.val_fine_epoch(model, feed_val)         # (in the mode the training left: training/fine.py:121)
        for k in T.FINE_TRAIN_KEYS:
            out["train"][k].append(train_out[k])
        for k in T.FINE_VAL_KEYS:
            out["val"][k].append(val_out[k])
        out["step_losses"].append(steps)
        out["skipped_steps"].append(train_out["skipped_steps"])
        if model.training:
            print("Conf score: skipped, the model is in train() mode (fine_conf_score makes single-sample calls)")
            out["conf"].append(None)
        else:
            out["conf"].append(T.fine_conf_score(model, feed_val, seed=a.seed))
            print("Conf score:", *out["conf"][-1])
        scheduler.step()
        print(f"\t lr {lr:0.6} epoch {epoch} loss {train_out['loss']:0.3f} "
              f"t-recall {train_out['recall']:0.2f} t-precision {train_out['precision']:0.2f} t-mean {train_out['pose_mean']:0.2f} "
              f"t-offset {train_out['pose_offsets']:0.2f} v-recall {val_out['recall']:0.2f} v-precision {val_out['precision']:0.2f} "
              f"v-mean {val_out['pose_mean']:0.2f} v-offset {val_out['pose_offsets']:0.2f} ", flush=True)
        if epoch >= a.epochs // 2:      # the best model by validation (training/fine.py:358-378)
            acc = float(np.mean((val_out["recall"], val_out["precision"])))
            if acc > best:
                path = os.path.join(a.out, f"fine_cont{cont}_acc{acc:0.2f}_lr{a.lr_idx}_obj-{a.num_mentioned}-{a.pad_size}"
                                           f"_ecl{int(a.class_embed)}_eco{int(a.color_embed)}_p{a.pointnet_numpoints}_npa0_nca0_f-{feats}.pth")
                print("Saving model to", path)
                save_reference_style(model, path)
                if last_path is not None and last_path != path and os.path.isfile(last_path):
                    print("Removing", last_path)
                    os.remove(last_path)
                best, last_path = acc, path
    out["checkpoint"] = last_path
    return out


if __name__ == "__main__":
    main()
