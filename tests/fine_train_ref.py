"""Shared by tests/test_gpu_fine_train_forward.py and tests/test_fine_train_host.py: the shapes of the train-mode fine forward, the
float64 / fp32 oracle references (computed once per shape and handed out unchanged) and the log-domain decision margins.

Reference: oracle/fine.py's OracleSuperGlueMatch in .train() - its forward_packed is no_grad and follows the reference's call order
(PointNet++ once per sample, the other object MLPs once per batch, each GNN layer first on the object tokens, then on the hint
tokens).  Weights: tests/golden/weights.py seed 14, copied as conftest.make_fine_pair copies them.  The float64 evaluation uses the
`.double()` + `torch.Tensor.float` patch of test_gpu_parity.py::test_training_step_at_the_reference_batch_size."""
import copy
import functools

import numpy as np
import torch

SINKHORN_ITERS = 50
WEIGHT_SEED = 14
MARGIN = 1e-3          # log domain
LOG_THRESHOLD = float(np.log(0.2))

# B samples, M objects, N hints, D channels, GNN layer pairs, points per object; cells = S.make_cells(cell_seed, B, fixed_n=M,
# n_pts=P), hints = S.make_texts(text_seed, 0, B * N, n_hints=1) cut into B lists of N; cap = largest share of matches0 (and of
# matches1) entries whose decision margin may lie below MARGIN.
SHAPES = {
    "a": dict(B=4, M=16, N=6, D=128, layers=2, P=64, cell_seed=707, text_seed=808, cap=0.0),
    "b": dict(B=1, M=16, N=6, D=128, layers=1, P=64, cell_seed=707, text_seed=808, cap=0.0),    # one sample: statistics over 16 and 6 rows
    "c": dict(B=3, M=5, N=7, D=64, layers=1, P=32, cell_seed=707, text_seed=808, cap=0.0),      # more hints than objects, odd counts
    "d": dict(B=2, M=4, N=2, D=128, layers=1, P=8, cell_seed=707, text_seed=808, cap=0.0),      # the smallest
    # (e) with text seed 808 leaves 2 of its 12 matches1 entries (16.7 %) below the margin in the float64 oracle: text seed 809
    "e": dict(B=2, M=16, N=6, D=256, layers=2, P=64, cell_seed=707, text_seed=809, cap=0.15),
    "f": dict(B=5, M=16, N=6, D=128, layers=2, P=256, cell_seed=707, text_seed=808, cap=0.15),  # the reference's sample shape
}


def vocab():
    from text2pos_amd import synthetic as S
    return dict(classes=S.LABELS + ["pad"], colors=S.COLOR_NAMES, words=S.known_words())


def fine_args(d, layers):
    from oracle import model as OM
    return OM.default_args(embed_dim=d, num_layers=layers, sinkhorn_iters=SINKHORN_ITERS)


def shape_inputs(name):
    """(xyz, rgb, center, mean_rgb, cell_ptr, hints) of a shape."""
    from text2pos_amd import synthetic as S
    s = SHAPES[name]
    cells = S.make_cells(s["cell_seed"], s["B"], fixed_n=s["M"], n_pts=s["P"])
    flat = S.make_texts(s["text_seed"], 0, s["B"] * s["N"], n_hints=1)
    hints = [flat[i * s["N"]: (i + 1) * s["N"]] for i in range(s["B"])]
    return cells + (hints,)


def make_product(d, layers, device=None):
    """SuperGlueMatch with the golden weights (seed 14), in eval() as constructed by conftest.make_fine_pair."""
    import weights as W
    import text2pos_amd as t2p
    v = vocab()
    prod = t2p.SuperGlueMatch(v["classes"], v["colors"], v["words"], fine_args(d, layers)).eval()
    W.fill_state_dict(prod, WEIGHT_SEED)
    return prod.to(device) if device is not None else prod


def oracle_from(state_dict, d, layers):
    """CPU oracle (fp32, eval()) carrying a product state_dict - parameters AND BatchNorm buffers."""
    from oracle import fine as OF
    v = vocab()
    sd = {k: t.detach().cpu() for k, t in state_dict.items()}
    orc = OF.OracleSuperGlueMatch(v["classes"], v["colors"], v["words"], fine_args(d, layers)).eval()
    own = orc.state_dict()
    orc.load_state_dict({k: sd[k] for k in own if not k.startswith("superglue.")}, strict=False)
    orc.superglue.load_reference_state(sd)
    for i, layer in enumerate(orc.superglue.layers):
        layer.bn.num_batches_tracked.copy_(sd[f"superglue.gnn.layers.{i}.mlp.1.num_batches_tracked"])
    return orc


def run_oracle(orc, inputs, double):
    """forward_packed of a deep copy of `orc` in train() mode; float64: the whole module in double, the oracle's own `.float()`
    casts of its inputs turned into `.double()`.  Returns (outputs, the copy - its BatchNorm buffers have moved)."""
    m = copy.deepcopy(orc).train()
    if not double:
        return m.forward_packed(*inputs), m
    m = m.double()
    orig_float = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        out = m.forward_packed(*inputs)
    finally:
        torch.Tensor.float = orig_float
    return out, m


def oracle_buffer_name(name):
    """Product buffer name -> the oracle's (superglue.gnn.layers.{i}.mlp.1.* -> superglue.layers.{i}.bn.*)."""
    if name.startswith("superglue.gnn.layers."):
        i, rest = name[len("superglue.gnn.layers."):].split(".", 1)
        assert rest.startswith("mlp.1."), name
        return f"superglue.layers.{i}.bn.{rest[len('mlp.1.'):]}"
    return name


def _top2_gap(x, axis):
    """Gap between the two largest entries along `axis` (inf when there is only one)."""
    if x.shape[axis] < 2:
        return np.full(np.delete(x.shape, axis), np.inf)
    s = np.sort(x, axis=axis)
    return np.take(s, -1, axis=axis) - np.take(s, -2, axis=axis)


def decision_margins(p64):
    """Log-domain margins of the matches0 / matches1 decisions of couplings p64 [B, M + 1, N + 1] (float64).
    matches0[b, o]: the smallest of (gap between the two largest entries of inner row o, gap between the two largest entries of the
    winning hint's inner column, distance of the winner from log 0.2), in log P with P clamped at 1e-300; matches1[b, h]: the same
    with rows and columns exchanged.  Returns (margin0 [B, M], margin1 [B, N])."""
    lp = np.log(np.maximum(np.asarray(p64, dtype=np.float64), 1e-300))[:, :-1, :-1]
    row_gap, col_gap = _top2_gap(lp, 2), _top2_gap(lp, 1)           # [B, M], [B, N]
    row_arg, col_arg = lp.argmax(2), lp.argmax(1)
    row_max, col_max = lp.max(2), lp.max(1)
    m0 = np.minimum(np.minimum(row_gap, np.take_along_axis(col_gap, row_arg, 1)), np.abs(row_max - LOG_THRESHOLD))
    m1 = np.minimum(np.minimum(col_gap, np.take_along_axis(row_gap, col_arg, 1)), np.abs(col_max - LOG_THRESHOLD))
    return m0, m1


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests compare a shape against, computed once: inputs, float64 outputs `out64` (tensors), the fp32 oracle's
    own distance `e32` of P from them, the decision margins and the float64 oracle's BatchNorm buffers after the forward."""
    s = SHAPES[name]
    inputs = shape_inputs(name)
    orc = oracle_from(make_product(s["D"], s["layers"]).state_dict(), s["D"], s["layers"])
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    try:
        out64, m64 = run_oracle(orc, inputs, double=True)
        out32, _ = run_oracle(orc, inputs, double=False)
    finally:
        torch.set_num_threads(threads)
    e32 = (out32["P"].double() - out64["P"]).abs().max().item()
    m0, m1 = decision_margins(out64["P"].numpy())
    return dict(shape=s, inputs=inputs, out64=out64, e32=e32, margin0=m0, margin1=m1,
                buffers64={k: v.clone() for k, v in m64.named_buffers()})
