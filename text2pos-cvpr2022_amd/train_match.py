"""Training-mode forward of the fine matcher: what `output = model(objects, hints, object_points)` computes under `model.train()`
in training/fine.py:54 and - because its validation never calls `model.eval()` - in eval_epoch / eval_conf (:119-208).

Same graph as t2p_match (csrc/match.hip), but the BatchNorm inside every AttentionalPropagation (models/superglue.py:119-129)
normalises with the statistics of the rows it is called on, so nothing is folded.  The reference calls a layer twice, first on
the object tokens of the whole batch, then on the hint tokens (models/superglue.py:139-146): two BatchNorm calls per layer, over
B * n_obj and B * n_hints rows.  The token rows are therefore kept SET-major - all object tokens (sample-major), then all hint
tokens - and one train_ops.bn_relu_train over the two row segments does both calls, running estimates included, in that order.
Per layer:
    QKV = X [Wq | Wk | Wv]                    train_ops linear (every Conv1d(k=1) is a per-token Linear)
    MSG = multi-head attention per sample     ops.match_attention (t2p_match_attention, csrc/match_train.hip)
    H   = relu(BN([X | MSG Wm] W1))           linear, linear, bn_relu_train (batch statistics, two segments)
    X  += H W2                                linear
then final_proj, the optimal-transport head (ops.match_head, t2p_match_head) and mlp_offsets on the hint encodings
(models/superglue_matcher.py:116).  Exact fp32 GEMMs whatever model.precision says, as in the coarse training path.

With autograd on (SuperGlueMatch admits it inside training.fine_backward() only) the two kernels of csrc/match_train.hip run as
_MatchAttentionFn / _MatchHeadFn, whose backward kernels recompute what they need from the forward's inputs; every other layer has
its backward in train_ops.py.  The running estimates of the BatchNorms move in the forward alone, once, as under no_grad."""
import numpy as np
import torch

from . import ops
from . import train_ops as TO
from .train_cell import _host_plan, object_rows_train


def _conv(x, conv):
    """Conv1d(kernel_size=1) on token rows (or a Linear): x [rows, in] -> [rows, out]."""
    w = conv.weight
    # bias gradient from the float64 column sum: attn.proj.1 / .2, attn.merge and mlp.0 stand in front of a softmax or a BatchNorm,
    # their bias gradient is exactly zero and what the step sees of it is rounding alone
    return TO._LinearFn.apply(x, w.squeeze(-1) if w.dim() == 3 else w, conv.bias, True)


class _MatchAttentionFn(torch.autograd.Function):
    """ops.match_attention with t2p_match_attention_backward: the backward recomputes the scores and the softmax from qkv."""

    @staticmethod
    def forward(ctx, qkv, b, m, n, cross):
        qkv = qkv.detach().contiguous()
        ctx.save_for_backward(qkv)
        ctx.sizes = (b, m, n, bool(cross))
        return ops.match_attention(qkv, b, m, n, cross=cross)

    @staticmethod
    def backward(ctx, d_msg):
        (qkv,) = ctx.saved_tensors
        b, m, n, cross = ctx.sizes
        return ops.match_attention_backward(qkv, d_msg.contiguous(), b, m, n, cross), None, None, None, None


class _MatchHeadFn(torch.autograd.Function):
    """ops.match_head with t2p_match_head_backward.  bin_score is a tensor (the parameter); P is differentiable, the matches and the
    matching scores are not.  The backward re-runs the iterations in float64 from mdesc; the gradient of bin_score is the sum of the
    per-sample values d_bin (torch's sum of a [B] tensor: one reduction tree per B, no atomics)."""

    @staticmethod
    def forward(ctx, mdesc, bin_score, b, m, n, iters, threshold):
        mdesc = mdesc.detach().contiguous()
        alpha = float(bin_score.detach())
        out = ops.match_head(mdesc, b, m, n, alpha, iters, threshold)
        ctx.save_for_backward(mdesc)
        ctx.sizes = (b, m, n, alpha, int(iters), bin_score.dtype)
        rest = (out["matches0"], out["matches1"], out["matching_scores0"], out["matching_scores1"])
        ctx.mark_non_differentiable(*rest)
        return (out["P"],) + rest

    @staticmethod
    def backward(ctx, d_p, *_):
        (mdesc,) = ctx.saved_tensors
        b, m, n, alpha, iters, dtype = ctx.sizes
        d_mdesc, d_bin = ops.match_head_backward(mdesc, d_p.contiguous(), b, m, n, alpha, iters)
        return d_mdesc, d_bin.sum().to(dtype), None, None, None, None, None


def check_token_sets(batch: int, n_obj: int, n_hints: int, channels: int):
    """nn.BatchNorm1d refuses a single value per channel in training mode; so does the BatchNorm of the GNN for a token set that
    has a single row in the whole batch (B = 1 with one object or one hint).  Raised before anything is launched."""
    rows_min = min(batch * n_obj, batch * n_hints)
    if rows_min <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got a segment of {rows_min} row(s) "
                         f"x {channels} channels")     # the wording of train_ops.bn_relu_train / torch's _verify_batch_size


def match_train_forward(model, obj_enc: torch.Tensor, hint_enc: torch.Tensor) -> dict:
    """model: SuperGlueMatch in train(); obj_enc [B, n_obj, D], hint_enc [B, n_hints, D] fp32 unit descriptors on the GPU.
    Returns dict(P, matches0, matches1, matching_scores0, matching_scores1, offsets) as ops.match does; the running estimates of
    every GNN BatchNorm move twice (objects, then hints) and num_batches_tracked by 2.  With autograd on, P and offsets carry
    the graph back to the descriptors and to every parameter of superglue and mlp_offsets."""
    ops._need(obj_enc, "obj_enc", torch.float32, 3)
    dev = obj_enc.device
    ops._need(hint_enc, "hint_enc", torch.float32, 3, dev)
    b, m, d = obj_enc.shape
    n = hint_enc.shape[1]
    if hint_enc.shape[0] != b or hint_enc.shape[2] != d or d != model.embed_dim:
        raise RuntimeError(f"match_train_forward: obj_enc {tuple(obj_enc.shape)} / hint_enc {tuple(hint_enc.shape)} disagree "
                           f"(embed_dim {model.embed_dim})")
    check_token_sets(b, m, n, 2 * d)
    grad = torch.is_grad_enabled()        # (under no_grad the two kernels are called directly, as before their backward existed)
    sg = model.superglue
    seg = torch.from_numpy(np.array([0, b * m, b * (m + n)], dtype=np.int32)).to(dev, non_blocking=True)
    rows_min = min(b * m, b * n)
    hint_rows = hint_enc.reshape(b * n, d)
    x = torch.cat([obj_enc.reshape(b * m, d), hint_rows], dim=0)          # set-major token rows [B (m + n), D]
    for layer, name in zip(sg.gnn.layers, sg.gnn.names):
        w_qkv = torch.cat([p.weight.squeeze(-1) for p in layer.attn.proj], dim=0)      # [3D, D]: q | k | v side by side
        b_qkv = torch.cat([p.bias for p in layer.attn.proj], dim=0)
        qkv = TO._LinearFn.apply(x, w_qkv, b_qkv, True)
        if grad:
            msg = _MatchAttentionFn.apply(qkv, b, m, n, name == "cross")
        else:
            msg = ops.match_attention(qkv, b, m, n, cross=name == "cross")
        h = _conv(torch.cat([x, _conv(msg, layer.attn.merge)], dim=1), layer.mlp[0])
        h = TO.bn_relu_train(h, seg, layer.mlp[1], relu=True, rows_min=rows_min)
        x = x + _conv(h, layer.mlp[3])
    if grad:
        keys = ("P", "matches0", "matches1", "matching_scores0", "matching_scores1")
        out = dict(zip(keys, _MatchHeadFn.apply(_conv(x, sg.final_proj), sg.bin_score, b, m, n, model.sinkhorn_iters,
                                                sg.config["match_threshold"])))
    else:
        out = ops.match_head(_conv(x, sg.final_proj).contiguous(), b, m, n, float(sg.bin_score.detach()), model.sinkhorn_iters,
                             sg.config["match_threshold"])
    off = _conv(torch.relu(_conv(hint_rows.contiguous(), model.mlp_offsets[0])), model.mlp_offsets[2])
    out["offsets"] = off.reshape(b, n, 2)
    return out


def encode_objects_fine_train(model, xyz, rgb, center, mean_rgb, cell_ptr: np.ndarray, class_idx=None, color_idx=None):
    """The object side of SuperGlueMatch.forward in train() mode (models/superglue_matcher.py:99-103): ObjectEncoder.forward with
    the PointNet++ once per sample (train_cell.object_rows_train, shared with the coarse training path) and F.normalize.
    Returns [n_objects_total, D] unit rows."""
    cp = np.ascontiguousarray(np.asarray(cell_ptr), dtype=np.int64)
    plan = _host_plan(cp, 0, xyz.device)      # (k = 0: the fine model has no kNN graph)
    emb = object_rows_train(model, xyz, rgb, center, mean_rgb, plan, class_idx, color_idx)
    return TO.normalize(emb)
