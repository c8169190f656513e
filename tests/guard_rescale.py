"""Exact, function-preserving rescalings of the coarse model (test infrastructure for the fp16-range guard of the f16x3 path).

Multiplying one stage's activations by a power of two s and dividing the weights that consume them by s leaves the network's
output unchanged (every operation involved commutes with a power-of-two scale: Linear, BatchNorm in eval mode, ReLU, max / mean
aggregation), while that one stage moves through fp16's range.  ROWS lists one such recipe per guarded stage:

  mul:  state_dict entries multiplied by s (they produce the stage's activations)
  div:  (entry, column slice) pairs divided by s (they consume them; None = the whole tensor)
  bit:  the guard bit that must fire when the stage's largest activation passes fp16's largest value (None: safety only)

The key prefix P is the PointNet++ of the object encoder.  ROW "input colours" scales the `rgb` point argument itself (not
`mean_rgb`): apply() returns the rescaled colours along with the state dict.
"""
import copy
from types import SimpleNamespace

import torch

P = "object_encoder.pointnet."
SA_C = (64, 128, 256)     # output channels of SA levels 1..3: the feature columns of the consumer's first Linear


def _hidden(nn_):
    """Hidden layer of a mlp([a, b, c]) with BatchNorm (Linear, BN, ReLU) x 2: BN 1 and Linear 2's bias grow by s, BN 2 takes
    the factor back (its running mean grows with its input, its weight shrinks)."""
    return dict(mul=[nn_ + "0.1.weight", nn_ + "0.1.bias", nn_ + "1.0.bias", nn_ + "1.1.running_mean"],
                div=[(nn_ + "1.1.weight", None)])


def _rows():
    rows = {}
    for l in (1, 2, 3):
        nn_ = f"{P}sa{l}.point_conv.local_nn."
        rows[f"sa{l} hidden"] = dict(_hidden(nn_), bit=1 << (l - 1), site=("local_nn", l, 0))
        consumer = f"{P}sa{l + 1}.point_conv.local_nn.0.0.weight" if l < 3 else f"{P}ga.mlp.0.0.weight"
        rows[f"sa{l} output"] = dict(mul=[nn_ + "1.1.weight", nn_ + "1.1.bias"], div=[(consumer, slice(0, SA_C[l - 1]))],
                                    bit=0x8, site=("local_nn", l, 1))
    rows["ga hidden"] = dict(_hidden(P + "ga.mlp."), bit=0x10, site=("ga", 0))
    rows["f0"] = dict(mul=[P + "ga.mlp.1.1.weight", P + "ga.mlp.1.1.bias"], div=[(P + "lin1.weight", None)], bit=0x20,
                      site=("features", 0))
    rows["f1"] = dict(mul=[P + "lin1.weight", P + "lin1.bias"], div=[(P + "lin2.weight", None)], bit=0x20, site=("features", 1))
    rows["f2"] = dict(mul=[P + "lin2.weight", P + "lin2.bias"], div=[("object_encoder.mlp_pointnet.0.0.weight", None)], bit=0x20,
                      site=("features", 2))
    rows["edge hidden"] = dict(_hidden("graph1.nn."), bit=0x20, site=("edge", 0))
    rows["input colours"] = dict(mul=[], div=[(f"{P}sa1.point_conv.local_nn.0.0.weight", slice(0, 3))], bit=None,
                                 site=("rgb",))
    return {k: SimpleNamespace(name=k, **v) for k, v in rows.items()}


ROWS = _rows()


def apply(sd, rgb, row, s):
    """(state_dict, rgb) with `row` rescaled by s: fresh tensors, the inputs are left as they are.  s should be a power of two
    (then the rescaling is exact in any binary floating-point type)."""
    r = ROWS[row] if isinstance(row, str) else row
    out = copy.deepcopy(sd)
    for k in r.mul:
        out[k] = out[k] * s
    for k, cols in r.div:
        if cols is None:
            out[k] = out[k] / s
        else:
            w = out[k].clone()
            w[:, cols] = w[:, cols] / s
            out[k] = w
    if r.site == ("rgb",):
        rgb = rgb * s
    return out, rgb


def activation_maxima(om, xyz, rgb, center, mean_rgb, cell_ptr):
    """(output of om.encode_objects_packed, {row: largest |activation| of the stage the row scales}).  Forward hooks record the
    maximum over all per-cell calls of local_nn[0] / local_nn[1] of each SA level, ga.mlp[0] and graph1.nn[0]; features0/1/2
    come from the oracle's trace."""
    seen = {}
    handles = []

    def hook(key):
        def f(mod, inp, out):
            seen[key] = max(seen.get(key, 0.0), float(out.detach().abs().max()))
        return f
    pn = om.object_encoder.pointnet
    for l in (1, 2, 3):
        nn_ = getattr(pn, f"sa{l}").point_conv.local_nn
        for i in (0, 1):
            handles.append(nn_[i].register_forward_hook(hook(("local_nn", l, i))))
    handles.append(pn.ga.mlp[0].register_forward_hook(hook(("ga", 0))))
    handles.append(om.graph1.nn[0].register_forward_hook(hook(("edge", 0))))
    tr = []
    try:
        out = om.encode_objects_packed(xyz, rgb, center, mean_rgb, cell_ptr, trace=tr)
    finally:
        for h in handles:
            h.remove()
    for i in (0, 1, 2):
        seen[("features", i)] = max(float(t[f"features{i}"].abs().max()) for t in tr if f"features{i}" in t)
    seen[("rgb",)] = float(torch.as_tensor(rgb).abs().max())
    return out, {name: seen[r.site] for name, r in ROWS.items()}
