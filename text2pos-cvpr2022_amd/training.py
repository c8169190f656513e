"""Host loops of the reference's PointNet++ pre-training (training/pointcloud/pointnet2.py:24-67, `train_epoch` / `val_epoch`:
train_pointnet_epoch, val_pointnet_epoch below) and of the reference's coarse training (training/coarse.py:31-62, `train_epoch`) on the HIP path: same batch
dictionary (`texts`, `objects`, `object_points` as the reference's Kitti360CoarseDataset.collate_fn yields them), same
order of calls; the arithmetic is docs/notebook.md 4.8.  val_fine_epoch is the validation pass of the fine stage
(training/fine.py:119-170, `eval_epoch`), which the reference runs in train() mode; train_fine_epoch is its training pass
(training/fine.py:36-116, `train_epoch`), inside the opt-in fine_backward().  The data side (datasets, augmentation, plotting) stays with the caller."""
import contextlib
from typing import Iterable, Optional

import numpy as np
import torch

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
    for i_batch, batch in enumerate(dataloader):
        if max_batches is not None and i_batch >= max_batches:
            break
        optimizer.zero_grad()
        if side is not None:
            main = torch.cuda.current_stream(dev)
            side.wait_stream(main)                       # zero_grad / the previous optimizer step
            with torch.cuda.stream(side):
                anchor = model.encode_text(batch["texts"])
            positive = model.encode_objects(batch["objects"], batch["object_points"])
            main.wait_stream(side)
            anchor.record_stream(main)                   # allocated on the side stream's pool, consumed by the loss on the main one
        else:
            anchor = model.encode_text(batch["texts"])
            positive = model.encode_objects(batch["objects"], batch["object_points"])
        loss = criterion(anchor, positive)
        loss.backward()
        optimizer.step()
        epoch_losses.append(loss.item())
        batches.append(batch)
    return float(np.mean(epoch_losses)) if epoch_losses else float("nan"), batches


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


@torch.no_grad()
def val_fine_epoch(model, dataloader: Iterable[dict]) -> dict:
    """training/fine.py:119-170 (`eval_epoch`): one pass over `dataloader` (batches as Kitti360FineDataset.collate_fn builds them:
    objects, hint_descriptions, object_points, matches, poses) WITHOUT touching the model's mode - the reference leaves its
    `model.eval()` commented out, so after a training epoch the validation runs in train() mode, with batch statistics in every
    BatchNorm and moving running estimates; the figures in the released checkpoint names come from that mode.  Returns the means
    over the batches of recall, precision, pose_mid, pose_mean, pose_offsets."""
    stats = {k: [] for k in FINE_VAL_KEYS}
    for batch in dataloader:
        output = model(batch["objects"], batch["hint_descriptions"], batch["object_points"])
        for k, v in fine_batch_stats(batch, output).items():
            stats[k].append(v)
    return {k: float(np.mean(v)) if v else float("nan") for k, v in stats.items()}


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


def train_fine_epoch(model, dataloader: Iterable[dict], optimizer, max_batches: Optional[int] = None) -> dict:
    """training/fine.py:36-116 (`train_epoch`): one pass over `dataloader` (batches as Kitti360FineDataset.collate_fn builds them:
    objects, hint_descriptions, object_points, matches, all_matches, offsets, poses) in train() mode, loss = MatchingLoss(P,
    all_matches) + 5 MSELoss(offsets, target offsets), and the reference's seven statistics as means over the batches: loss,
    loss_offsets, recall, precision, pose_mid, pose_mean, pose_offsets (fine_batch_stats).  Enters fine_backward() itself.
    A step whose loss is not finite (an untrained matcher's listed couplings can lie below fp32's range: -log 0) is skipped - no
    backward, no optimizer.step() - and counted in stats["skipped_steps"]; the reference gets there through detect_anomaly and its
    try / except around loss.backward().  Its loss still enters the mean, as in the reference."""
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
            stats["loss_offsets"].append(loss_offsets.item())
            for k, v in fine_batch_stats(batch, output).items():
                stats[k].append(v)
    out = {k: float(np.mean(v)) if v else float("nan") for k, v in stats.items()}
    out["skipped_steps"] = skipped
    return out
