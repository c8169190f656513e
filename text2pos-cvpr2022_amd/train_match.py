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

Forward only: the layers above except the two kernels of csrc/match_train.hip have a backward (train_ops.py); until those two
have one, a call with autograd enabled is refused by SuperGlueMatch."""
import numpy as np
import torch

from . import ops
from . import train_ops as TO
from .train_cell import _host_plan, object_rows_train


def _conv(x, conv):
    """Conv1d(kernel_size=1) on token rows (or a Linear): x [rows, in] -> [rows, out]."""
    w = conv.weight
    return TO._LinearFn.apply(x, w.squeeze(-1) if w.dim() == 3 else w, conv.bias)


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
    every GNN BatchNorm move twice (objects, then hints) and num_batches_tracked by 2."""
    ops._need(obj_enc, "obj_enc", torch.float32, 3)
    dev = obj_enc.device
    ops._need(hint_enc, "hint_enc", torch.float32, 3, dev)
    b, m, d = obj_enc.shape
    n = hint_enc.shape[1]
    if hint_enc.shape[0] != b or hint_enc.shape[2] != d or d != model.embed_dim:
        raise RuntimeError(f"match_train_forward: obj_enc {tuple(obj_enc.shape)} / hint_enc {tuple(hint_enc.shape)} disagree "
                           f"(embed_dim {model.embed_dim})")
    check_token_sets(b, m, n, 2 * d)
    sg = model.superglue
    seg = torch.from_numpy(np.array([0, b * m, b * (m + n)], dtype=np.int32)).to(dev, non_blocking=True)
    rows_min = min(b * m, b * n)
    hint_rows = hint_enc.reshape(b * n, d)
    x = torch.cat([obj_enc.reshape(b * m, d), hint_rows], dim=0)          # set-major token rows [B (m + n), D]
    for layer, name in zip(sg.gnn.layers, sg.gnn.names):
        w_qkv = torch.cat([p.weight.squeeze(-1) for p in layer.attn.proj], dim=0)      # [3D, D]: q | k | v side by side
        b_qkv = torch.cat([p.bias for p in layer.attn.proj], dim=0)
        qkv = TO._LinearFn.apply(x, w_qkv, b_qkv)
        msg = ops.match_attention(qkv, b, m, n, cross=name == "cross")
        h = _conv(torch.cat([x, _conv(msg, layer.attn.merge)], dim=1), layer.mlp[0])
        h = TO.bn_relu_train(h, seg, layer.mlp[1], relu=True, rows_min=rows_min)
        x = x + _conv(h, layer.mlp[3])
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
