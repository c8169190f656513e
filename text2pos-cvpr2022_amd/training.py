"""Host loops of the reference's PointNet++ pre-training (training/pointcloud/pointnet2.py:24-67, `train_epoch` / `val_epoch`:
train_pointnet_epoch, val_pointnet_epoch below) and of the reference's coarse training (training/coarse.py:31-62, `train_epoch`) on the HIP path: same batch
dictionary (`texts`, `objects`, `object_points` as the reference's Kitti360CoarseDataset.collate_fn yields them), same
order of calls; the arithmetic is docs/notebook.md 4.8.  val_fine_epoch is the validation pass of the fine stage
(training/fine.py:119-170, `eval_epoch`), which the reference runs in train() mode; train_fine_epoch is its training pass
(training/fine.py:36-116, `train_epoch`), inside the opt-in fine_backward().  SceneCoarseFeed is the coarse stage's training set
(Kitti360CoarseDataset, dataloading/kitti360pose/cells.py:36-110: hint shuffle, cell flips, the rotating transform) with every draw
counter-based, packed from a scene resident in HBM or built by the host chain; SceneFineFeed is the fine stage's
(Kitti360FineDataset, dataloading/kitti360pose/poses.py:32-210) in the same two forms, its device batches scored by
t2p_fine_step_stats; fine_conf_score is training/fine.py:173-208 (`eval_conf`).  The plots stay with the caller."""
import contextlib
from typing import Iterable, Optional

import numpy as np
import torch

from . import data as D
from . import ops
from .losses import HardestRankingLoss, MatchingLoss, MSELoss, PairwiseRankingLoss, calc_pose_error, calc_recall_precision


def make_criterion(args) -> torch.nn.Module:
    """training/coarse.py:279-284: --ranking_loss pairwise (the default, training/args.py:48) or hardest.  `triplet` is not
    built: it needs the dataset's negative cells, and the reference's own branch cannot run as written - it calls
    `model.encode_objects(negative_cell_objects)` without the `object_points` argument the method requires
    (training/coarse.py:48-51 against models/cell_retrieval.py:77)."""
    kind = getattr(args, "ranking_loss", "pairwise")
    margin = getattr(args, "margin", 0.35)
    if kind == "pairwise":
        return PairwiseRankingLoss(margin=margin)
    if kind == "hardest":
        return HardestRankingLoss(margin=margin)
    raise NotImplementedError(f"ranking_loss={kind!r}: 'pairwise' and 'hardest' are built")


_TEXT_STREAMS = {}    # device -> the text branch's stream (picked once: ops.concurrent_stream probes the hardware queues)


def train_epoch(model, dataloader: Iterable[dict], optimizer, criterion, max_batches: Optional[int] = None,
                overlap_text: bool = True):
    """One pass over `dataloader` (training/coarse.py:31-62).  Returns (mean loss, the batches seen).
    overlap_text: the text branch runs on a second HIP stream beside the cell branch - the two meet only in the loss, and autograd
    runs a node's backward on the stream of its forward, so the biLSTM's step-by-step recurrence (a chain of small latency-bound
    kernels, ~3 ms of a 64 + 64 step) runs beside the cell branch's matrix kernels in both directions.  Same kernels, same
    arithmetic: the loss of a step is bit-identical to overlap_text=False, its gradients agree to the rounding noise that the
    float atomics of the scatter-backward kernels have from run to run anyway (tested).  Worth 0.4 ms of 27.8 on one MI355X: the
    step is paced by the host's launch / size-read-back ping-pong, not by the GPU."""
    model.train()
    epoch_losses, batches = [], []
    dev = model.device
    side = None
    if overlap_text and dev.type == "cuda":
        if str(dev) not in _TEXT_STREAMS:
            _TEXT_STREAMS[str(dev)] = ops.concurrent_stream(dev)
        side = _TEXT_STREAMS[str(dev)]
    scene = getattr(dataloader, "scene", None)           # SceneCoarseFeed hands over the DeviceScene its batches index

    def encode_positive(batch):
        if "scene_batch" in batch:                       # packed on the GPU from the resident scene (SceneCoarseFeed)
            if scene is None:
                raise RuntimeError("train_epoch: a batch carries `scene_batch` but the dataloader has no `scene` (scene.DeviceScene)")
            return model.encode_scene_batch(scene, batch["scene_batch"])
        return model.encode_objects(batch["objects"], batch["object_points"])

    for i_batch, batch in enumerate(dataloader):
        if max_batches is not None and i_batch >= max_batches:
            break
        optimizer.zero_grad()
        if side is not None:
            main = torch.cuda.current_stream(dev)
            side.wait_stream(main)                       # zero_grad / the previous optimizer step
            with torch.cuda.stream(side):
                anchor = model.encode_text(batch["texts"])
            positive = encode_positive(batch)
            main.wait_stream(side)
            anchor.record_stream(main)                   # allocated on the side stream's pool, consumed by the loss on the main one
        else:
            anchor = model.encode_text(batch["texts"])
            positive = encode_positive(batch)
        loss = criterion(anchor, positive)
        loss.backward()
        optimizer.step()
        epoch_losses.append(loss.item())
        batches.append(batch)
    return float(np.mean(epoch_losses)) if epoch_losses else float("nan"), batches


_ITEM_SALT = 0x6974656D5F6B6579      # SceneCoarseFeed: the per-item draws (flips, hint order) hash apart from the sampling keys
_FLIP_SALT = np.uint64(0x666C69705F626974)
_HINT_SALT = np.uint64(0x68696E745F6F7264)


class SceneCoarseFeed:
    """The coarse stage's training batches (Kitti360CoarseDataset.__getitem__ + collate_fn, dataloading/kitti360pose/cells.py:65-110,
    behind a DataLoader): one item per pose - the pose's own cell, its hint sentences (evaluation.create_hint_description) shuffled
    and joined with spaces, the cell flipped horizontally and / or vertically with probability 1/2 each (the text with it), every
    object resampled to n_pts points, rotated about z by an angle in +-rotate_degrees and normalised (training/coarse.py:192-198).
    Everything random about the item of pose p in epoch e is a function of (seed, e, p) alone - the sampling keys and angles of
    sample index e * n_poses + p (pipeline.PerCellTransform), the two flip bits, the hint permutation - never of the batch size, the
    batch order or what was drawn before; the epoch's order is a permutation seeded by (seed, e) when `shuffle`; the last short
    batch is kept (DataLoader's default).
    With `scene` (scene.DeviceScene of scenes.all_cells, built with mirror=True when flip_poses) a batch is {"texts", "cell_ids",
    "pose_indices", "scene_batch"}: scene_batch = {obj_ids, keys, flip, rot, cell_ptr, n_pts}, which
    CellRetrievalNetwork.encode_scene_batch packs with one kernel launch (train_epoch does that).  Without one, or with host=True,
    a batch is the reference's dictionary {"texts", "objects" (the flipped copies), "object_points", "cell_ids", "pose_indices"} built
    by the host chain (data.flip_cell, PerCellTransform.for_cell) from the same draws: the same packed arrays, bit for bit.
    Not built: sample_close_cell."""

    def __init__(self, scenes, scene=None, n_pts: int = 256, seed: int = 0, batch_size: int = 64, shuffle: bool = True,
                 shuffle_hints: bool = True, flip_poses: bool = True, rotate_degrees: Optional[float] = 120.0, host: bool = False):
        from .evaluation import create_hint_description
        from .pipeline import PerCellTransform
        self.scenes, self.scene, self.host = scenes, scene, bool(host) or scene is None
        self.n_pts, self.seed, self.batch_size = int(n_pts), int(seed), int(batch_size)
        self.shuffle, self.shuffle_hints, self.flip_poses = bool(shuffle), bool(shuffle_hints), bool(flip_poses)
        self.transform = PerCellTransform(self.n_pts, self.seed, rotate_degrees)
        self.poses = scenes.all_poses
        self.hints = [create_hint_description(p) for p in self.poses]
        self.epoch = 0
        if self.batch_size < 1:
            raise ValueError("SceneCoarseFeed: batch_size must be at least 1")
        missing = [p.cell_id for p in self.poses if p.cell_id not in scenes.cells_dict]
        if missing:
            raise ValueError(f"SceneCoarseFeed: {len(missing)} poses lie in cells the scene does not hold (first: {missing[0]})")
        if not self.host:
            if self.flip_poses and scene.raw_mirror_xy is None:
                raise RuntimeError("SceneCoarseFeed: flip_poses needs a DeviceScene built with mirror=True")
            if len(scene.cell_ids) < len(scenes.all_cells) or any(a != c.id for a, c in zip(scene.cell_ids, scenes.all_cells)):
                raise RuntimeError("SceneCoarseFeed: the DeviceScene does not hold scenes.all_cells in order")
            self._row = np.array([scene.row_of[p.cell_id] for p in self.poses], dtype=np.int64)

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return (len(self.poses) + self.batch_size - 1) // self.batch_size

    # ---- the draws of one item: functions of (seed, epoch, pose index) -----------------------------------------------------------
    def sample_index(self, pose_index, epoch: Optional[int] = None):
        """epoch * n_poses + pose: the PerCellTransform sample whose keys draw the item's points and angles."""
        e = self.epoch if epoch is None else int(epoch)
        return e * len(self.poses) + np.asarray(pose_index, dtype=np.int64)

    def _item_key(self, pose_index, epoch=None) -> np.ndarray:
        return D.sample_keys(self.seed ^ _ITEM_SALT, self.sample_index(pose_index, epoch), 0)

    def flip_codes(self, pose_index, epoch: Optional[int] = None) -> np.ndarray:
        """uint8 codes of the poses' items: bit 0 = horizontal flip, bit 1 = vertical flip; two independent fair draws."""
        idx = np.atleast_1d(np.asarray(pose_index, dtype=np.int64))
        if not self.flip_poses:
            return np.zeros(idx.shape[0], dtype=np.uint8)
        return (D.mix64(self._item_key(idx, epoch) ^ _FLIP_SALT) >> np.uint64(62)).astype(np.uint8)

    def _hint_orders(self, idx: np.ndarray, item: np.ndarray) -> list:
        """hint_order of the poses `idx` with item keys `item`, one hash matrix for all of them."""
        counts = [len(self.hints[int(p)]) for p in idx]
        if not self.shuffle_hints or not counts:
            return [np.arange(c) for c in counts]
        with np.errstate(over="ignore"):
            h = D.mix64(item[:, None] ^ _HINT_SALT ^ (np.arange(max(counts), dtype=np.uint64) * D._KEY_MUL)[None, :])
        if min(counts) == max(counts):
            return list(np.argsort(h, axis=1, kind="stable"))
        return [np.argsort(h[r, :c], kind="stable") for r, c in enumerate(counts)]

    def hint_order(self, pose_index: int, epoch: Optional[int] = None) -> np.ndarray:
        """The order the item's hints are joined in: a permutation (the ranks of one hash per hint), the identity without
        shuffle_hints."""
        idx = np.array([int(pose_index)], dtype=np.int64)
        return self._hint_orders(idx, self._item_key(idx, epoch))[0]

    def _texts(self, idx: np.ndarray, codes: np.ndarray, item: np.ndarray) -> list:
        out = []
        for p, code, order in zip(idx, codes, self._hint_orders(idx, item)):
            hints = self.hints[int(p)]
            text = " ".join(hints[int(j)] for j in order)
            if code & 1:
                text = D._swap_words(text, "east", "west")
            if code & 2:
                text = D._swap_words(text, "north", "south")
            out.append(text)
        return out

    def text(self, pose_index: int, epoch: Optional[int] = None) -> str:
        """The item's description: hints in hint_order joined with spaces (cells.py:79-82), then flipped like the cell."""
        idx = np.array([int(pose_index)], dtype=np.int64)
        return self._texts(idx, self.flip_codes(idx, epoch), self._item_key(idx, epoch))[0]

    def epoch_order(self, epoch: Optional[int] = None) -> np.ndarray:
        e = self.epoch if epoch is None else int(epoch)
        n = len(self.poses)
        return np.random.default_rng([self.seed & 0xFFFFFFFF, e, 0x6F72646572]).permutation(n) if self.shuffle else np.arange(n)

    # ---- batches -----------------------------------------------------------------------------------------------------------------
    def batch(self, pose_indices, epoch: Optional[int] = None) -> dict:
        idx = np.asarray(pose_indices, dtype=np.int64)
        codes, si = self.flip_codes(idx, epoch), self.sample_index(idx, epoch)
        out = dict(texts=self._texts(idx, codes, self._item_key(idx, epoch)), cell_ids=[self.poses[int(p)].cell_id for p in idx],
                   pose_indices=idx)
        if self.host:
            objects, points = [], []
            for p, code, s in zip(idx, codes, si):
                cell, _ = D.flip_cell_code(self.scenes.cells_dict[self.poses[int(p)].cell_id], "", int(code))
                objs = cell.objects if isinstance(cell.objects, list) else list(cell.objects)
                objects.append(objs)
                points.append(D.batch_object_points(objs, self.transform.for_cell(int(s))))
            out.update(objects=objects, object_points=points)
            return out
        cp_all = self.scene.cell_ptr
        rows = self._row[idx]
        n = cp_all[rows + 1] - cp_all[rows]
        cell_ptr = np.zeros(idx.shape[0] + 1, dtype=np.int32)
        np.cumsum(n, out=cell_ptr[1:])
        start = np.repeat(cell_ptr[:-1].astype(np.int64), n)
        slot = np.arange(int(cell_ptr[-1]), dtype=np.int64) - start
        obj_ids = np.repeat(cp_all[rows], n) + slot
        sample = np.repeat(si, n)
        out["scene_batch"] = dict(obj_ids=obj_ids, keys=self.transform.keys(sample, slot),
                                  flip=np.repeat(codes, n) if self.flip_poses else None,
                                  rot=self.transform.rotations(sample, slot), cell_ptr=cell_ptr, n_pts=self.n_pts)
        return out

    def __iter__(self):
        epoch = self.epoch
        order = self.epoch_order(epoch)
        for a in range(0, order.shape[0], self.batch_size):
            yield self.batch(order[a: a + self.batch_size], epoch)


REGRESSOR_CELLS, REGRESSOR_LEARNS = ("pose", "best"), ("center", "closest")


def fine_item_tables(pose, cell, pad_size: int, num_mentioned: int, regressor_cell: str = "pose", regressor_learn: str = "center",
                     name: str = "pose") -> dict:
    """What load_pose_and_cell (dataloading/kitti360pose/poses.py:32-139) decides about one pose before anything random happens:
      order                int64 [<= pad_size] positions in cell.objects: the objects of the matched descriptions in description
                           order, then the cell's remaining objects in cell order, cut to pad_size (poses.py:82-108); the missing
                           slots are padding objects
      matches              int64 [k, 2] (slot, hint); all_matches: matches, then (pad_size, hint) per unmatched hint, then
                           (slot, num_hints) per slot whose object is not matched, padding included (poses.py:114-131)
      offsets              float64 [num_hints, 2] of the regressor_cell x regressor_learn choice (poses.py:49-70)
      offsets_best_center  float64 [num_hints, 2] (poses.py:72-78)
    Raises ValueError naming `name` for what the reference asserts (or fails on)."""
    descriptions = pose.descriptions
    n_hints = len(descriptions)
    if n_hints != num_mentioned:
        raise ValueError(f"SceneFineFeed: {name} has {n_hints} descriptions, num_mentioned is {num_mentioned}")
    objects = cell.objects if isinstance(cell.objects, list) else list(cell.objects)
    position = {o.id: k for k, o in enumerate(objects)}          # poses.py:36
    order, matches, matched_ids = [], [], []
    for j, d in enumerate(descriptions):
        if not d.is_matched:
            continue
        if d.object_id not in position:
            raise ValueError(f"SceneFineFeed: description {j} of {name} is matched to object {d.object_id}, which cell {cell.id} does not hold")
        if d.object_id in matched_ids:     # (the reference's `len(objects) == len(cell.objects)` assertion, poses.py:98-104)
            raise ValueError(f"SceneFineFeed: two descriptions of {name} are matched to one object ({d.object_id})")
        k = position[d.object_id]
        want = getattr(d, "object_instance_id", None)
        if want is not None and objects[k].instance_id != want:                                   # poses.py:87
            raise ValueError(f"SceneFineFeed: description {j} of {name} names instance {want}, object {d.object_id} of cell {cell.id} "
                             f"is instance {objects[k].instance_id}")
        matched_ids.append(d.object_id)
        matches.append((len(order), j))
        order.append(k)
    if len(order) > pad_size:
        raise ValueError(f"SceneFineFeed: {name} has {len(order)} matched objects, more than pad_size = {pad_size}")
    taken = set(matched_ids)
    order += [k for k, o in enumerate(objects) if o.id not in taken]
    order = order[:pad_size]
    all_matches = list(matches)
    all_matches += [(pad_size, j) for j, d in enumerate(descriptions) if not d.is_matched]
    all_matches += [(s, n_hints) for s in range(pad_size) if s >= len(order) or objects[order[s]].id not in taken]
    pick = lambda d, best, plain: np.asarray(getattr(d, best) if d.is_matched else getattr(d, plain), dtype=np.float64)[0:2]
    if regressor_cell not in REGRESSOR_CELLS or regressor_learn not in REGRESSOR_LEARNS:
        raise ValueError(f"SceneFineFeed: regressor_cell / regressor_learn must be one of {REGRESSOR_CELLS} / {REGRESSOR_LEARNS}")
    plain = "offset_" + regressor_learn
    best = "best_offset_" + regressor_learn if regressor_cell == "best" else plain
    offsets = np.array([pick(d, best, plain) for d in descriptions], dtype=np.float64).reshape(n_hints, 2)
    if np.isnan(offsets).any():
        raise ValueError(f"SceneFineFeed: NaN among the {regressor_cell} / {regressor_learn} offsets of {name}")
    best_center = np.array([pick(d, "best_offset_center", "offset_center") for d in descriptions], dtype=np.float64).reshape(n_hints, 2)
    return dict(order=np.asarray(order, dtype=np.int64), matches=np.asarray(matches, dtype=np.int64).reshape(-1, 2),
                all_matches=np.asarray(all_matches, dtype=np.int64).reshape(-1, 2), offsets=offsets, offsets_best_center=best_center)


class SceneFineFeed:
    """The fine stage's batches (Kitti360FineDataset.__getitem__ + collate_fn, dataloading/kitti360pose/poses.py:32-210, behind a
    DataLoader): one item per pose - the pose's cell with the matched objects first, cut or padded to pad_size, the hint sentences
    in description order, matches / all_matches / offsets (fine_item_tables: nothing about them is random, they are built once
    here), every object resampled to n_pts points, rotated about z by an angle in +-rotate_degrees (None: validation) and
    normalised (training/fine.py:228-239).  The draws of pose p in epoch e are those of PerCellTransform sample e * n_poses + p,
    slot = position in the padded object list: never of the batch size or order; the epoch's order is a permutation seeded by
    (seed, e) when `shuffle`; the last short batch is kept.
    With `scene` (scene.DeviceScene holding the poses' cells and n_pad >= pad_size padding objects; slot j's padding is
    scene.pad_ids[j], DeviceScene.padded_object_ids' convention) a batch is {"hint_descriptions", "texts", "pose_indices",
    "scene_batch", "fine_targets"}: scene_batch = {obj_ids, keys, flip: None, rot, cell_ptr, n_pts} for
    SuperGlueMatch.forward_scene_batch, fine_targets = device tensors only - pose_idx int32 [B] and the feed's resident tables
    gt_hint, pose_xy, slot_center_xy (ops.fine_step_stats), target_offsets fp32 [B, num_hints, 2], and the batch's all_matches as
    the CSR idx int32 [E, 2] / entry_ptr int32 [B + 1] of t2p_matching_loss.  With host=True, or without a scene, a batch is the
    reference's dictionary (poses, cells, objects, object_points, hint_descriptions, texts, matches, all_matches, offsets,
    offsets_best_center) built by the host chain from the same draws; the padding objects are the scene's, or drawn from
    default_rng([pad_seed, 0x70616400]) as DeviceScene draws them.
    Not built: flip_pose (the reference trains and validates the fine stage without, training/fine.py:241-251) and no_pc_augment
    (FixedPoints without NormalizeScale)."""

    def __init__(self, scenes, scene=None, n_pts: int = 256, seed: int = 0, batch_size: int = 32, shuffle: bool = False,
                 pad_size: int = 16, num_mentioned: int = 6, regressor_cell: str = "pose", regressor_learn: str = "center",
                 rotate_degrees: Optional[float] = 120.0, host: bool = False, flip_pose: bool = False, no_pc_augment: bool = False,
                 pad_seed: Optional[int] = None):
        from .evaluation import create_hint_description
        from .pipeline import PerCellTransform
        if flip_pose:
            raise NotImplementedError("SceneFineFeed: flip_pose is not built (the reference trains the fine stage without it)")
        if no_pc_augment:
            raise NotImplementedError("SceneFineFeed: no_pc_augment (FixedPoints without NormalizeScale) is not built")
        self.scenes, self.scene, self.host = scenes, scene, bool(host) or scene is None
        self.n_pts, self.seed, self.batch_size, self.shuffle = int(n_pts), int(seed), int(batch_size), bool(shuffle)
        self.pad_size, self.num_mentioned = int(pad_size), int(num_mentioned)
        self.regressor_cell, self.regressor_learn = regressor_cell, regressor_learn
        self.transform = PerCellTransform(self.n_pts, self.seed, rotate_degrees)
        self.poses = scenes.all_poses
        self.epoch = 0
        if self.batch_size < 1 or self.pad_size < 1:
            raise ValueError("SceneFineFeed: batch_size and pad_size must be at least 1")
        n, pad, nh = len(self.poses), self.pad_size, self.num_mentioned
        self.hint_descriptions = [create_hint_description(p) for p in self.poses]
        self.texts = [" ".join(h) for h in self.hint_descriptions]
        self.order = np.full((n, pad), -1, dtype=np.int64)          # position in the cell's object list, -1 = padding
        self.matches, self.all_matches = [], []
        self.offsets = np.zeros((n, nh, 2), dtype=np.float64)
        self.offsets_best_center = np.zeros((n, nh, 2), dtype=np.float64)
        self.gt_hint = np.full((n, pad), -1, dtype=np.int32)
        for i, p in enumerate(self.poses):
            name = f"pose {i} ({p.cell_id})"
            if p.cell_id not in scenes.cells_dict:
                raise ValueError(f"SceneFineFeed: {name} lies in a cell the scene does not hold")
            t = fine_item_tables(p, scenes.cells_dict[p.cell_id], pad, nh, regressor_cell, regressor_learn, name)
            self.order[i, : t["order"].shape[0]] = t["order"]
            self.matches.append(t["matches"])
            self.all_matches.append(t["all_matches"])
            self.offsets[i], self.offsets_best_center[i] = t["offsets"], t["offsets_best_center"]
            self.gt_hint[i, t["matches"][:, 0]] = t["matches"][:, 1]
        self.pose_xy = np.array([np.asarray(p.pose, dtype=np.float64)[0:2] for p in self.poses], dtype=np.float64).reshape(n, 2)
        self.entry_ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([a.shape[0] for a in self.all_matches], out=self.entry_ptr[1:])
        self.obj_ids = None
        if scene is not None:
            if len(scene.pad_ids) < pad:
                raise RuntimeError(f"SceneFineFeed: the DeviceScene was built with n_pad={len(scene.pad_ids)} < pad_size={pad}")
            rows = []
            for i, p in enumerate(self.poses):
                if p.cell_id not in scene.row_of:
                    raise ValueError(f"SceneFineFeed: pose {i} ({p.cell_id}) lies in a cell the DeviceScene does not hold")
                r = scene.row_of[p.cell_id]
                if int(scene.cell_ptr[r + 1] - scene.cell_ptr[r]) != len(scenes.cells_dict[p.cell_id].objects):
                    raise RuntimeError(f"SceneFineFeed: cell {p.cell_id} of the DeviceScene is not the scenes' cell of that id")
                rows.append(r)
            first = scene.cell_ptr[np.asarray(rows, dtype=np.int64)] if n else np.zeros(0, dtype=np.int64)
            self.obj_ids = np.where(self.order >= 0, first[:, None] + self.order, scene.pad_ids[:pad][None, :]).astype(np.int64)
            self._pads = [scene._flat[int(j)] for j in scene.pad_ids[:pad]]
        else:
            rng = np.random.default_rng([int(self.seed if pad_seed is None else pad_seed), 0x7061_6400])
            self._pads = [D.Object3d.create_padding(rng=rng) for _ in range(pad)]
        self.tables = None
        if not self.host:       # uploaded once; a batch's targets are gathers of them
            dev = scene.device
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            flat = np.concatenate(self.all_matches, axis=0) if n else np.zeros((0, 2), dtype=np.int64)
            if n and (flat.min() < 0 or flat[:, 0].max() > pad or flat[:, 1].max() > nh):
                raise ValueError("SceneFineFeed: an all_matches pair outside [0, pad_size] x [0, num_mentioned]")
            self.tables = dict(gt_hint=to(self.gt_hint), pose_xy=to(self.pose_xy),
                               slot_center_xy=to(scene.center64[self.obj_ids][..., 0:2].astype(np.float64)),
                               target_offsets=to(self.offsets.astype(np.float32)), idx=to(flat.astype(np.int32)),
                               entry_ptr=to(self.entry_ptr.astype(np.int32)))

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return (len(self.poses) + self.batch_size - 1) // self.batch_size

    def sample_index(self, pose_index, epoch: Optional[int] = None):
        """epoch * n_poses + pose: the PerCellTransform sample whose keys draw the item's points and angles."""
        e = self.epoch if epoch is None else int(epoch)
        return e * len(self.poses) + np.asarray(pose_index, dtype=np.int64)

    def epoch_order(self, epoch: Optional[int] = None) -> np.ndarray:
        e = self.epoch if epoch is None else int(epoch)
        n = len(self.poses)
        return np.random.default_rng([self.seed & 0xFFFFFFFF, e, 0x6F72646572]).permutation(n) if self.shuffle else np.arange(n)

    def objects(self, pose_index: int) -> list:
        """The item's padded object list (the cell's own Object3d instances, then the padding objects of the missing slots)."""
        p = self.poses[int(pose_index)]
        cell = self.scenes.cells_dict[p.cell_id]
        return [cell.objects[int(k)] if k >= 0 else self._pads[s] for s, k in enumerate(self.order[int(pose_index)])]

    def batch(self, pose_indices, epoch: Optional[int] = None) -> dict:
        idx = np.atleast_1d(np.asarray(pose_indices, dtype=np.int64))
        si = self.sample_index(idx, epoch)
        out = dict(hint_descriptions=[self.hint_descriptions[int(p)] for p in idx], texts=[self.texts[int(p)] for p in idx],
                   pose_indices=idx)
        if self.host:
            objects = [self.objects(int(p)) for p in idx]
            out.update(poses=[self.poses[int(p)] for p in idx], cells=[self.scenes.cells_dict[self.poses[int(p)].cell_id] for p in idx],
                       objects=objects,
                       object_points=[D.batch_object_points(o, self.transform.for_cell(int(s))) for o, s in zip(objects, si)],
                       matches=[self.matches[int(p)] for p in idx], all_matches=[self.all_matches[int(p)] for p in idx],
                       offsets=[self.offsets[int(p)] for p in idx], offsets_best_center=[self.offsets_best_center[int(p)] for p in idx])
            return out
        b, pad = idx.shape[0], self.pad_size
        slot = np.arange(pad, dtype=np.int64)
        out["scene_batch"] = dict(obj_ids=self.obj_ids[idx].reshape(-1), keys=self.transform.keys(si[:, None], slot[None, :]).reshape(-1),
                                  flip=None, rot=self.transform.rotations(np.repeat(si, pad), np.tile(slot, b)),
                                  cell_ptr=np.arange(b + 1, dtype=np.int32) * pad, n_pts=self.n_pts)
        # one upload: the pose indices, the batch's re-based entry pointers and the rows of the resident pair table it gathers
        lo, hi = self.entry_ptr[idx], self.entry_ptr[idx + 1]
        ptr = np.zeros(b + 1, dtype=np.int64)
        np.cumsum(hi - lo, out=ptr[1:])
        gather = np.repeat(lo - ptr[:-1], hi - lo) + np.arange(int(ptr[-1]), dtype=np.int64)
        t = self.tables
        host = np.concatenate([idx, ptr, gather]).astype(np.int32)
        dev = torch.from_numpy(host).to(t["idx"].device, non_blocking=True)
        pose_idx, entry_ptr, rows = dev[:b], dev[b: 2 * b + 1], dev[2 * b + 1:].long()
        out["fine_targets"] = dict(pose_idx=pose_idx, gt_hint=t["gt_hint"], pose_xy=t["pose_xy"], slot_center_xy=t["slot_center_xy"],
                                   target_offsets=t["target_offsets"][pose_idx.long()], idx=t["idx"][rows], entry_ptr=entry_ptr)
        return out

    def __iter__(self):
        epoch = self.epoch
        order = self.epoch_order(epoch)
        for a in range(0, order.shape[0], self.batch_size):
            yield self.batch(order[a: a + self.batch_size], epoch)


def _hits(output, batch, criterion=None):
    """training/pointcloud/pointnet2.py:42 / :60: torch.sum(torch.argmax(class_pred, -1) == batch.y) / len(class_pred).  The
    criterion's kernel has counted the hits of this very call already (losses.CrossEntropyLoss.last_correct); any other
    criterion, and the validation loop, take the line as written."""
    n = len(output.class_pred)
    hits = getattr(criterion, "last_correct", None)
    if hits is not None and hits.shape[0] == n:
        return int(hits.sum().item()) / n
    y = batch.y.to(output.class_pred.device)
    return torch.sum(torch.argmax(output.class_pred.detach(), dim=-1) == y).item() / n


def train_pointnet_epoch(model, dataloader: Iterable, optimizer, criterion, max_batches: Optional[int] = None):
    """One pass of the pre-training loop (training/pointcloud/pointnet2.py:24-49) over `dataloader`: batches with .x, .pos,
    .batch and the class labels .y.  model: pointnet2.PointNet2; criterion: losses.CrossEntropyLoss.  Returns (mean loss, mean
    accuracy) over the batches."""
    model.train()
    epoch_losses, epoch_accs = [], []
    for i_batch, batch in enumerate(dataloader):
        if max_batches is not None and i_batch >= max_batches:
            break
        optimizer.zero_grad()
        output = model(batch)
        loss = criterion(output.class_pred, batch.y.to(output.class_pred.device))
        loss.backward()
        optimizer.step()
        epoch_losses.append(loss.item())
        epoch_accs.append(_hits(output, batch, criterion))
    if not epoch_losses:
        return float("nan"), float("nan")
    return float(np.mean(epoch_losses)), float(np.mean(epoch_accs))


@torch.no_grad()
def val_pointnet_epoch(model, dataloader: Iterable):
    """training/pointcloud/pointnet2.py:52-67: eval() mode, mean accuracy over the batches."""
    model.eval()
    epoch_accs = [_hits(model(batch), batch) for batch in dataloader]
    return float(np.mean(epoch_accs)) if epoch_accs else float("nan")


FINE_VAL_KEYS = ("recall", "precision", "pose_mid", "pose_mean", "pose_offsets")


def fine_batch_stats(batch: dict, output) -> dict:
    """The five figures training/fine.py:134-166 takes from one batch and the model's output for it: recall / precision of the
    matches against batch["matches"], and the pose error with the cell's middle as the estimate (pose_mid), with the mean of the
    matched objects' centres (pose_mean) and with the regressed offsets added (pose_offsets)."""
    m0 = output.matches0.detach().cpu().numpy()
    m1 = output.matches1.detach().cpu().numpy()
    off = output.offsets.detach().cpu().numpy()
    recall, precision = calc_recall_precision(batch["matches"], m0, m1)
    return dict(recall=recall, precision=precision,
                pose_mid=calc_pose_error(batch["objects"], m0, batch["poses"], offsets=off, use_mid_pred=True),
                pose_mean=calc_pose_error(batch["objects"], m0, batch["poses"], offsets=None),
                pose_offsets=calc_pose_error(batch["objects"], m0, batch["poses"], offsets=off))


def _feed_scene(dataloader, scene, who: str):
    """The DeviceScene a batch with `scene_batch` is packed from: the argument, else the feed's own (SceneFineFeed.scene)."""
    scene = getattr(dataloader, "scene", None) if scene is None else scene
    if scene is None:
        raise RuntimeError(f"{who}: a batch carries `scene_batch` but there is no `scene` (scene.DeviceScene), given or on the dataloader")
    return scene


def _device_step_stats(output, targets: dict, loss=None, loss_offsets=None) -> np.ndarray:
    """ops.fine_step_stats on a device batch's targets and the step's ONE device-to-host copy: float64 [7] = loss, loss_offsets
    (NaN when not given) and the five figures of fine_batch_stats."""
    _, row = ops.fine_step_stats(output.matches0, output.matches1, output.offsets.detach().contiguous(), targets["pose_idx"],
                                 targets["gt_hint"], targets["pose_xy"], targets["slot_center_xy"], loss, loss_offsets, check=False)
    return ops.fine_step_row(row)


@torch.no_grad()
def val_fine_epoch(model, dataloader: Iterable[dict], scene=None) -> dict:
    """training/fine.py:119-170 (`eval_epoch`): one pass over `dataloader` (batches as Kitti360FineDataset.collate_fn builds them:
    objects, hint_descriptions, object_points, matches, poses) WITHOUT touching the model's mode - the reference leaves its
    `model.eval()` commented out, so after a training epoch the validation runs in train() mode, with batch statistics in every
    BatchNorm and moving running estimates; the figures in the released checkpoint names come from that mode.  Returns the means
    over the batches of recall, precision, pose_mid, pose_mean, pose_offsets.
    A batch with `scene_batch` (SceneFineFeed on a resident scene; `scene` defaults to dataloader.scene) is packed and scored on the
    device: forward_scene_batch, ops.fine_step_stats, one 56-byte copy."""
    stats = {k: [] for k in FINE_VAL_KEYS}
    for batch in dataloader:
        if "scene_batch" in batch:
            output = model.forward_scene_batch(_feed_scene(dataloader, scene, "val_fine_epoch"), batch["scene_batch"],
                                               batch["hint_descriptions"])
            row = _device_step_stats(output, batch["fine_targets"])
            for i, k in enumerate(FINE_VAL_KEYS):
                stats[k].append(float(row[2 + i]))
            continue
        output = model(batch["objects"], batch["hint_descriptions"], batch["object_points"])
        for k, v in fine_batch_stats(batch, output).items():
            stats[k].append(v)
    return {k: float(np.mean(v)) if v else float("nan") for k, v in stats.items()}


_CONF_SALT = 0x636F6E66      # fine_conf_score: its pose draws hash apart from the feed's


@torch.no_grad()
def fine_conf_score(model, feed, n_trials: int = 100, seed: int = 0):
    """`eval_conf` of training/fine.py:173-208: per trial five single-sample calls on poses drawn at random, each scored by the
    number of objects matches0 assigns; returns the reference's two means - over both argmax readings (first maximum at position 0,
    last maximum at position 0) and over the first alone.  The poses come from default_rng([seed, ...]), not from the global
    np.random, so a score repeats; the items are those of the feed's current epoch (feed.batch).
    eval() mode only: a single-sample call in train() mode would normalise every BatchNorm of the matcher with the statistics of that
    one sample (and move the running estimates by them); train_match.check_token_sets refuses only the degenerate case of a single
    token per set, so the mode is refused here."""
    if model.training:
        raise NotImplementedError("fine_conf_score: single-sample calls in train() mode take their batch statistics from one sample; "
                                  "call model.eval() first")
    picks = np.random.default_rng([int(seed) & 0xFFFFFFFF, _CONF_SALT]).integers(0, len(feed.poses), size=(int(n_trials), 5))
    accs, accs_old = [], []
    for trial in picks:
        confs = []
        for p in trial:
            batch = feed.batch([int(p)])
            if "scene_batch" in batch:
                output = model.forward_scene_batch(_feed_scene(feed, None, "fine_conf_score"), batch["scene_batch"],
                                                   batch["hint_descriptions"])
            else:
                output = model(batch["objects"], batch["hint_descriptions"], batch["object_points"])
            confs.append(output.matches0)
        confs = (torch.cat(confs, 0) >= 0).sum(dim=1).cpu().numpy()       # one read-back per trial
        accs.append(np.argmax(confs) == 0)
        accs.append(np.argmax(np.flip(confs)) == len(confs) - 1)
        accs_old.append(np.argmax(confs) == 0)
    return float(np.mean(accs)), float(np.mean(accs_old))


# ---- the fine stage's backward: opt-in ------------------------------------------------------------------------------------------------
_FINE_BACKWARD = False    # consulted by SuperGlueMatch._check_forward_only (train() branch) and losses._no_grad_inputs


def fine_backward_enabled() -> bool:
    return _FINE_BACKWARD


def enable_fine_backward(on: bool = True) -> bool:
    """Sets the switch; returns what it was.  Off (the default): SuperGlueMatch in train() mode, MatchingLoss and MSELoss refuse
    inputs that would record a graph.  On: they are differentiable (csrc/match_train.hip's backward kernels).  eval() mode with
    autograd stays refused either way."""
    global _FINE_BACKWARD
    was, _FINE_BACKWARD = _FINE_BACKWARD, bool(on)
    return was


@contextlib.contextmanager
def fine_backward(on: bool = True):
    """`with training.fine_backward(): ...` - the switch of enable_fine_backward for the body, restored afterwards (also when the
    body raises)."""
    was = enable_fine_backward(on)
    try:
        yield
    finally:
        enable_fine_backward(was)


FINE_TRAIN_KEYS = ("loss", "loss_offsets") + FINE_VAL_KEYS


def train_fine_epoch(model, dataloader: Iterable[dict], optimizer, max_batches: Optional[int] = None, scene=None,
                     step_losses: Optional[list] = None) -> dict:
    """training/fine.py:36-116 (`train_epoch`): one pass over `dataloader` (batches as Kitti360FineDataset.collate_fn builds them:
    objects, hint_descriptions, object_points, matches, all_matches, offsets, poses) in train() mode, loss = MatchingLoss(P,
    all_matches) + 5 MSELoss(offsets, target offsets), and the reference's seven statistics as means over the batches: loss,
    loss_offsets, recall, precision, pose_mid, pose_mean, pose_offsets (fine_batch_stats).  Enters fine_backward() itself.
    A step whose loss is not finite (an untrained matcher's listed couplings can lie below fp32's range: -log 0) is skipped - no
    backward, no optimizer.step() - and counted in stats["skipped_steps"]; the reference gets there through detect_anomaly and its
    try / except around loss.backward().  Its loss still enters the mean, as in the reference.
    A batch with `scene_batch` (SceneFineFeed on a resident scene; `scene` defaults to dataloader.scene) takes the device path:
    forward_scene_batch packs it with one launch, the matching loss reads the batch's prebuilt device CSR (its ranges were checked
    when the feed was built: no host lists, no isnan read), the offset loss the gathered targets, ops.fine_step_stats computes the
    five figures where the outputs are, and ONE 56-byte copy per step brings back the finite-loss decision and all seven
    statistics.  step_losses: a list that receives every step's loss."""
    from .losses import _MatchingLossFn
    model.train()
    criterion_matching, criterion_offsets = MatchingLoss(), MSELoss()
    stats = {k: [] for k in FINE_TRAIN_KEYS}
    skipped = 0
    dev = model.device
    with fine_backward():
        for i_batch, batch in enumerate(dataloader):
            if max_batches is not None and i_batch >= max_batches:
                break
            optimizer.zero_grad()
            if "scene_batch" in batch:
                targets = batch["fine_targets"]
                output = model.forward_scene_batch(_feed_scene(dataloader, scene, "train_fine_epoch"), batch["scene_batch"],
                                                   batch["hint_descriptions"])
                loss_matching, _ = _MatchingLossFn.apply(output.P, targets["idx"], targets["entry_ptr"])
                loss_offsets = criterion_offsets(output.offsets, targets["target_offsets"])
                loss = loss_matching + 5 * loss_offsets
                row = _device_step_stats(output, targets, loss.detach(), loss_offsets.detach())
                if np.isfinite(row[0]):
                    loss.backward()
                    optimizer.step()
                else:
                    skipped += 1
                for i, k in enumerate(FINE_TRAIN_KEYS):
                    stats[k].append(float(row[i]))
                if step_losses is not None:
                    step_losses.append(float(row[0]))
                continue
            output = model(batch["objects"], batch["hint_descriptions"], batch["object_points"])
            loss_matching = criterion_matching(output.P, batch["all_matches"])
            target = torch.from_numpy(np.ascontiguousarray(np.asarray(batch["offsets"], dtype=np.float32))).to(dev)
            loss_offsets = criterion_offsets(output.offsets, target)
            loss = loss_matching + 5 * loss_offsets
            value = loss.item()
            if np.isfinite(value):
                loss.backward()
                optimizer.step()
            else:
                skipped += 1
            stats["loss"].append(value)
            if step_losses is not None:
                step_losses.append(value)
            stats["loss_offsets"].append(loss_offsets.item())
            for k, v in fine_batch_stats(batch, output).items():
                stats[k].append(v)
    out = {k: float(np.mean(v)) if v else float("nan") for k, v in stats.items()}
    out["skipped_steps"] = skipped
    return out
