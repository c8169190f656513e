"""Retrieval training loss of the reference on the HIP path: `PairwiseRankingLoss`
(training/losses.py:126-164; `--margin 0.35`, training/args.py:46; constructed at training/coarse.py:279-282).
Same call `criterion(anchor, positive)`; the reference's hard-coded `.cuda()` is gone (tensors stay on their device).
The hinge terms, their sum and the gradient with respect to the score matrix come from t2p_pairwise_ranking
(csrc/small_kernels.hip); the score matrix and its two gradient products run on the library's own fp32-MFMA GEMM (ops.matmul).
`HardestRankingLoss` (training/losses.py:167-201, --ranking_loss hardest) shares the wrapper on t2p_hardest_ranking.
`CrossEntropyLoss` is the criterion of the PointNet++ pre-training stage (training/pointcloud/pointnet2.py:37, :134:
`nn.CrossEntropyLoss()(output.class_pred, batch.y)`) on t2p_softmax_xent (csrc/classify.hip).
The fine stage (training/fine.py:35-36, :56-62): `MatchingLoss` (training/losses.py:13-30) on t2p_matching_loss and `MSELoss`
(`nn.MSELoss()`) on t2p_mse_loss (csrc/match_train.hip), differentiable with respect to P / the input inside
training.fine_backward() (t2p_matching_loss_backward, t2p_mse_loss_backward; opt-in, refused outside it) - and the two
host-side validation figures `calc_recall_precision` / `calc_pose_error` (training/losses.py:33-62, :81-123) in NumPy."""
import numpy as np
import torch
import torch.nn as nn

from . import ops


class _PairwiseRankingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im, s, margin, hardest=False):
        n_im = torch.norm(im.detach(), dim=1, keepdim=True)
        n_s = torch.norm(s.detach(), dim=1, keepdim=True)
        im_n, s_n = (im.detach() / n_im).contiguous(), (s.detach() / n_s).contiguous()
        scores = ops.matmul(im_n, s_n.t().contiguous())
        terms, d_scores = (ops.hardest_ranking if hardest else ops.pairwise_ranking)(scores, margin)
        ctx.save_for_backward(im_n, s_n, n_im, n_s, d_scores)
        return terms.sum() / im.shape[0]

    @staticmethod
    def backward(ctx, g):
        im_n, s_n, n_im, n_s, d_scores = ctx.saved_tensors
        d_imn, d_sn = ops.matmul(d_scores, s_n), ops.gemm_tn(d_scores, im_n)
        # x / |x|: d x = (d x_n - x_n <x_n, d x_n>) / |x|
        d_im = (d_imn - im_n * (im_n * d_imn).sum(1, keepdim=True)) / n_im
        d_s = (d_sn - s_n * (s_n * d_sn).sum(1, keepdim=True)) / n_s
        return g * d_im, g * d_s, None, None


class PairwiseRankingLoss(nn.Module):
    def __init__(self, margin: float = 1.0):
        super().__init__()
        self.margin = margin

    def forward(self, im, s):
        if im.shape != s.shape or im.dim() != 2:
            raise RuntimeError("PairwiseRankingLoss: anchor and positive must both be [B, D]")
        return _PairwiseRankingFn.apply(im, s, float(self.margin))


class HardestRankingLoss(nn.Module):
    """training/losses.py:167-201 (--ranking_loss hardest): only the hardest negative of every anchor / positive counts."""

    def __init__(self, margin: float = 1.0):
        super().__init__()
        self.margin = margin

    def forward(self, images, captions):
        if images.shape != captions.shape or images.dim() != 2:
            raise RuntimeError("HardestRankingLoss: images and captions must both be [B, D]")
        return _PairwiseRankingFn.apply(images, captions, float(self.margin), True)


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        x = logits.detach()
        if x.dtype != torch.float32:
            x = x.float()
        row_loss, d_logits, correct = ops.softmax_xent(x, target.to(device=x.device, dtype=torch.int32).contiguous())
        ctx.save_for_backward(d_logits)
        ctx.mark_non_differentiable(correct)
        return row_loss.sum() / logits.shape[0], correct      # the mean as a fixed-order sum: no float atomics

    @staticmethod
    def backward(ctx, g, _g_correct):
        (d_logits,) = ctx.saved_tensors
        return g * d_logits, None


class CrossEntropyLoss(nn.Module):
    """`nn.CrossEntropyLoss()` as the pre-training loop uses it: criterion(logits [n, C], target [n] of class indices), mean
    reduction.  Loss, gradient and the per-row hit (argmax == target, the accuracy line training/pointcloud/pointnet2.py:42)
    come from ONE kernel launch; `last_correct` (int32 [n], on the device) holds the hits of the latest call.
    A target outside [0, C) raises (the kernel marks the row with NaN instead of reading through the label; reading the loss
    back here costs the host synchronisation the loop's `loss.item()` pays anyway)."""

    def __init__(self):
        super().__init__()
        self.last_correct = None

    def forward(self, logits, target):
        if logits.dim() != 2 or target.dim() != 1 or target.shape[0] != logits.shape[0]:
            raise RuntimeError("CrossEntropyLoss: logits must be [n, C] and target [n] (class indices)")
        if target.is_floating_point():
            raise RuntimeError("CrossEntropyLoss: target must hold class indices (class probabilities are not built)")
        if logits.shape[0] == 0:
            raise RuntimeError("CrossEntropyLoss: empty batch")
        loss, correct = _CrossEntropyFn.apply(logits, target)
        self.last_correct = correct
        if bool(torch.isnan(loss.detach())):
            t = target.detach()
            bad = ((t < 0) | (t >= logits.shape[1])).nonzero()
            if bad.numel():
                raise IndexError(f"CrossEntropyLoss: target {int(t[bad[0, 0]])} of row {int(bad[0, 0])} is outside [0, {logits.shape[1]})")
            raise FloatingPointError("CrossEntropyLoss: the loss is NaN (NaN among the logits)")
        return loss


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _no_grad_inputs(what, *tensors):
    """Refuses inputs that would record a graph unless training.fine_backward() is on; returns whether a graph is wanted."""
    if not _wants_grad(*tensors):
        return False
    from . import training
    if not training.fine_backward_enabled():
        raise NotImplementedError(f"{what}: the backward is not built; detach the inputs or call it under torch.no_grad()")
    return True


class _MatchingLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, idx, entry_ptr):
        x = P.detach()
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        loss, sample = ops.matching_loss(x, idx, entry_ptr)
        ctx.save_for_backward(x, idx, entry_ptr)
        ctx.dtype = P.dtype
        ctx.mark_non_differentiable(sample)
        return loss[0], sample

    @staticmethod
    def backward(ctx, g, _g_sample):
        x, idx, entry_ptr = ctx.saved_tensors
        d_p = ops.matching_loss_backward(x, idx, entry_ptr, g.detach().float().reshape(1).contiguous())   # g stays on the device
        return d_p.to(ctx.dtype), None, None


class _MseLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, target):
        a, b = input.detach().float().contiguous(), target.detach().float().contiguous()
        ctx.save_for_backward(a, b)
        ctx.dtype = input.dtype
        return ops.mse_loss(a, b)[0]

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return ops.mse_loss_backward(a, b, g.detach().float().reshape(1).contiguous()).to(ctx.dtype), None


class MatchingLoss(nn.Module):
    """training/losses.py:13-30: criterion(P, all_matches) with P [B, n_obj + 1, n_hints + 1] (SuperGlueMatch's couplings) and
    all_matches a list of B integer [M_i, 2] tensors / arrays of (object, hint) pairs, dustbin indices n_obj / n_hints included:
    mean over the samples of the mean over a sample's pairs of -log P[b, i, j], in ONE kernel launch (fixed summation order, float64
    accumulation: bit-identical from call to call).  As in the reference, a listed coupling that is 0 in fp32 gives inf.
    `last_sample_losses` [B] holds the per-sample means of the latest call.  Differentiable with respect to P inside
    training.fine_backward(): dP = -g / (B M_b P) per listed entry (a pair listed twice counts twice), 0 elsewhere.
    A pair outside [0, n_obj] x [0, n_hints] raises IndexError (the kernel marks the sample with NaN instead of reading through it;
    reading the loss back here costs the host synchronisation the loop's `loss.item()` pays anyway)."""

    def __init__(self):
        super().__init__()
        self.eps = 1e-3          # (kept: the reference's attribute, unused there as well)
        self.last_sample_losses = None

    def forward(self, P, all_matches):
        if not isinstance(P, torch.Tensor) or P.dim() != 3:
            raise RuntimeError("MatchingLoss: P must be a [B, n_obj + 1, n_hints + 1] tensor")
        if not P.is_cuda:
            raise RuntimeError(f"MatchingLoss: P must live on the GPU (got device {P.device}); there is no CPU path")
        grad = _no_grad_inputs("MatchingLoss", P)
        if len(all_matches) != P.shape[0]:
            raise RuntimeError(f"MatchingLoss: {P.shape[0]} samples in P but {len(all_matches)} match lists")
        lists = []
        for i, mt in enumerate(all_matches):
            a = mt.detach().cpu().numpy() if isinstance(mt, torch.Tensor) else np.asarray(mt)
            if a.ndim != 2 or a.shape[1] != 2:
                raise RuntimeError(f"MatchingLoss: all_matches[{i}] must be [M, 2] (got shape {a.shape})")
            if a.shape[0] == 0:
                raise RuntimeError(f"MatchingLoss: sample {i} has no match entries (its mean is undefined)")
            if not np.issubdtype(a.dtype, np.integer):
                raise RuntimeError(f"MatchingLoss: all_matches[{i}] must hold integer indices (got {a.dtype})")
            lists.append(a.astype(np.int64))
        ptr = np.zeros(len(lists) + 1, dtype=np.int64)
        np.cumsum([a.shape[0] for a in lists], out=ptr[1:])
        flat = np.concatenate(lists, axis=0)
        # (indices past int32 are out of range anyway: clip them to a value that stays out of range)
        both = np.concatenate([np.clip(flat, -1, np.iinfo(np.int32).max).reshape(-1), ptr]).astype(np.int32)
        dev_both = torch.from_numpy(both).to(P.device)       # one upload
        idx, entry_ptr = dev_both[: 2 * flat.shape[0]].view(-1, 2), dev_both[2 * flat.shape[0]:]
        if grad:
            loss, sample = _MatchingLossFn.apply(P, idx.contiguous(), entry_ptr.contiguous())
        else:
            x = P.detach()
            if x.dtype != torch.float32:
                x = x.float()
            loss, sample = ops.matching_loss(x.contiguous(), idx, entry_ptr)
            loss = loss[0]
        self.last_sample_losses = sample
        if bool(torch.isnan(loss.detach())):
            m1, n1 = P.shape[1], P.shape[2]
            for b, a in enumerate(lists):
                bad = np.nonzero((a[:, 0] < 0) | (a[:, 0] >= m1) | (a[:, 1] < 0) | (a[:, 1] >= n1))[0]
                if bad.size:
                    e = int(bad[0])
                    raise IndexError(f"MatchingLoss: entry {e} of sample {b}, ({int(a[e, 0])}, {int(a[e, 1])}), is outside "
                                     f"[0, {m1 - 1}] x [0, {n1 - 1}]")
            raise FloatingPointError("MatchingLoss: the loss is NaN (NaN among the listed couplings)")
        return loss


class MSELoss(nn.Module):
    """`nn.MSELoss()` as training/fine.py:36, :57-59 uses it: criterion(output.offsets, target offsets), mean reduction, one kernel
    launch with a fixed summation order.  Differentiable with respect to the input inside training.fine_backward()
    (2 g (input - target) / n); a target that requires grad is refused."""

    def forward(self, input, target):
        if not isinstance(input, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise RuntimeError("MSELoss: input and target must be tensors")
        if input.shape != target.shape:
            raise RuntimeError(f"MSELoss: input {tuple(input.shape)} and target {tuple(target.shape)} must have the same shape")
        if not input.is_cuda or not target.is_cuda:
            raise RuntimeError(f"MSELoss: input and target must live on the GPU (got {input.device}, {target.device}); "
                               "there is no CPU path")
        if input.numel() == 0:
            raise RuntimeError("MSELoss: empty input")
        if _wants_grad(target):
            from . import training
            if training.fine_backward_enabled():
                raise NotImplementedError("MSELoss: the backward with respect to the target is not built; detach the target")
        if _no_grad_inputs("MSELoss", input, target):
            return _MseLossFn.apply(input, target)
        return ops.mse_loss(input.detach().float().contiguous(), target.detach().float().contiguous())[0]


def calc_recall_precision(batch_gt_matches, batch_matches0, batch_matches1):
    """training/losses.py:33-62.  Per sample: recall = share of the ground-truth (object, hint) pairs that matches0 or matches1
    report; precision = share of the objects matches0 assigns (>= 0) whose (object, hint) pair is a ground-truth pair; 0.0 where a
    sample has no ground-truth pair / no assigned object.  Returns the two means over the samples."""
    if not len(batch_gt_matches) == len(batch_matches0) == len(batch_matches1):
        raise RuntimeError("calc_recall_precision: the three batch lists differ in length")
    recalls, precisions = [], []
    for gt, m0, m1 in zip(batch_gt_matches, batch_matches0, batch_matches1):
        pairs = {(int(i), int(j)) for i, j in np.asarray(gt).reshape(-1, 2)}
        found = [int(m0[i]) == j or int(m1[j]) == i for i, j in sorted(pairs)]
        right = [(i, int(j)) in pairs for i, j in enumerate(m0) if j >= 0]
        recalls.append(float(np.mean(found)) if found else 0.0)
        precisions.append(float(np.mean(right)) if right else 0.0)
    return float(np.mean(recalls)), float(np.mean(precisions))


def calc_pose_error(objects, matches0, poses, offsets=None, use_mid_pred=False, return_samples=False):
    """training/losses.py:81-123: mean distance in the x-y plane between the ground-truth pose (in cell coordinates) and the
    estimate get_pos_in_cell makes from the matched objects' centres plus the offsets of their hints.  offsets None: zero offsets
    (the mean of the matched centres); use_mid_pred: the cell's middle (0.5, 0.5) whatever was matched.
    objects: List[List[Object3d]]; matches0 [B, n_obj]; poses: B of data.Pose (or anything with .pose); offsets [B, n_hints, 2]."""
    from .superglue_matcher import get_pos_in_cell
    matches0 = np.asarray(matches0)
    if not len(objects) == len(matches0) == len(poses):
        raise RuntimeError("calc_pose_error: objects, matches0 and poses differ in length")
    truth = np.array([np.asarray(getattr(p, "pose", p), dtype=np.float64)[0:2] for p in poses])
    if offsets is None:
        offsets = np.zeros((matches0.shape[0], int(matches0.max(initial=-1)) + 1, 2))
    elif len(offsets) != len(objects):
        raise RuntimeError("calc_pose_error: objects and offsets differ in length")
    errors = []
    for i in range(len(objects)):
        pred = np.array((0.5, 0.5)) if use_mid_pred else get_pos_in_cell(objects[i], matches0[i], offsets[i])
        errors.append(float(np.linalg.norm(truth[i] - pred)))
    return errors if return_samples else float(np.mean(errors))
