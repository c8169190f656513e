# How far the fp32 oracle's training-mode gradients are from its own float64 evaluation (the conditioning behind the gradient bars of
# tests/test_gpu_parity.py::test_cell_branch_training_step_matches_autograd): python profiles/oracle_grad_conditioning.py <seed> [alt|nc|f1|sl] [cells]
import os, sys, torch, numpy as np, copy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import weights as W
from text2pos_amd import synthetic as S
from oracle import model as OM
classes, words = S.LABELS + ["pad"], S.known_words()
seed = int(sys.argv[1])
mode = sys.argv[2] if len(sys.argv) > 2 else ''
kw = {}
if mode in ('alt', 'nc'): kw['use_features'] = ['class', 'position']
if mode in ('alt', 'f1'): kw['pointnet_features'] = 1
sl = mode not in ('alt', 'sl')
NC = int(sys.argv[3]) if len(sys.argv) > 3 else 3
def run(dtype):
    om = OM.OracleCellRetrieval(classes, S.COLOR_NAMES, words, OM.default_args(**kw), sl); W.fill_state_dict(om, 23); om.train()
    om = om.to(dtype)
    for p in om.parameters(): p.requires_grad_(True)
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(seed, NC)
    coef = torch.randn(len(cell_ptr) - 1, 256, generator=torch.Generator().manual_seed(5)).to(dtype)
    # keep the geometry in fp32 so that FPS / ball query pick the same indices; only the arithmetic changes precision
    import oracle.model as M
    out = om.encode_objects_packed_grad(xyz, rgb, center, mean_rgb, cell_ptr) if dtype == torch.float32 else None
    return om, out, coef
om32, out32, coef = run(torch.float32); (out32 * coef).sum().backward()
# fp64: monkeypatch .float() calls by casting inputs; simplest: upcast module + feed float64 tensors
om64 = OM.OracleCellRetrieval(classes, S.COLOR_NAMES, words, OM.default_args(**kw), sl); W.fill_state_dict(om64, 23); om64.train(); om64 = om64.double()
for p in om64.parameters(): p.requires_grad_(True)
xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(seed, NC)
import torch.nn.functional as F
from oracle import pyg_restated as gnn
cp = [int(v) for v in cell_ptr]; P = xyz.shape[1]; X = torch.as_tensor(xyz).double(); R = torch.as_tensor(rgb).double()
batches, batch = [], []
for c in range(len(cp) - 1):
    lo, hi = cp[c], cp[c + 1]; n = hi - lo
    batches.append(gnn.Batch(x=R[lo:hi].reshape(n * P, 3).clone(), pos=X[lo:hi].reshape(n * P, 3).clone(), batch=torch.arange(n).repeat_interleave(P)))
    batch += [c] * n
batch = torch.tensor(batch)
oe = om64.object_encoder
orig_float = torch.Tensor.float
torch.Tensor.float = lambda self, *a, **k: self.double()   # the oracle casts some inputs with .float()
try:
    emb = oe(batches, torch.as_tensor(mean_rgb).double(), torch.as_tensor(center).double())
    emb = F.normalize(emb, dim=-1); x = om64.graph1(emb, batch); x = gnn.global_max_pool(x, batch); x = om64.lin(x); out64 = F.normalize(x)
finally:
    torch.Tensor.float = orig_float
(out64 * coef.double()).sum().backward()
print('out fp32 vs fp64', (out32.double() - out64).abs().max().item())
rows = []
for (n, a), (_, b) in zip(om32.named_parameters(), om64.named_parameters()):
    if a.grad is None or b.grad is None: continue
    rows.append(((a.grad.double() - b.grad).abs().max().item() / max(1e-30, b.grad.abs().max().item()), b.grad.abs().max().item(), n))
for r in [q for q in sorted(rows, reverse=True) if not q[2].endswith('.0.bias')][:8]:
    print('%.2e  gmax %.3e  %s' % r)
