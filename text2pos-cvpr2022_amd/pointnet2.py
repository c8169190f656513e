"""Mirror of models/pointcloud/pointnet2.py (PointNet2 with three set-abstraction layers, a global-abstraction layer and two
linear heads): the reference's constructor and state_dict layout, so that its checkpoints load unchanged, and its forward on the
HIP path.

PointNet2 is run in two places.  Inside CellRetrievalNetwork.encode_objects / SuperGlueMatch.forward it is part of the fused cell
encoder, batched over all objects of all cells.  On its own it is the object classifier the reference pre-trains first
(training/pointcloud/pointnet2.py) and every ObjectEncoder then loads (models/object_encoder.py:46): `PointNet2(...)(batch)`
returns features0 / 1 / 2, class_pred and color_pred as models/pointcloud/pointnet2.py:80-100 does - eval() on the folded inference
kernels of the cell encoder's trunk (t2p_pointnet2_forward) followed by the heads kernel, train() on the batch-statistics path of
train_cell.py with a backward pass.  The classifier sees a DataLoader batch as ONE PyG batch: PointConv's self-loop rewrite and
every BatchNorm span the whole batch (DESIGN.md section 2 says the same of a cell).
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import _lib, ops, packing
from .modules import Fp16RangeGuard, PicklableModule, get_mlp

MAX_BATCH_OBJECTS = _lib.DEFINES["T2P_MAX_CHUNK_OBJECTS"]   # the batch is one cell


class PointConv(nn.Module):
    """Holds `local_nn` under the key torch_geometric.nn.PointConv uses (`point_conv.local_nn.*`)."""

    def __init__(self, local_nn):
        super().__init__()
        self.local_nn = local_nn


class SetAbstractionLayer(nn.Module):
    def __init__(self, ratio, radius, mlp):
        super().__init__()
        self.ratio = ratio
        self.radius = radius
        self.point_conv = PointConv(local_nn=mlp)


class GlobalAbstractionLayer(nn.Module):
    def __init__(self, mlp):
        super().__init__()
        self.mlp = mlp


class PointNet2(Fp16RangeGuard, PicklableModule):
    _TRANSIENT = {"_pack": None, "_overflow": None}

    def __init__(self, num_classes, num_colors, args, add_self_loops: bool = True, precision: str = "f16x3",
                 on_overflow: str = "raise"):
        """add_self_loops, precision, on_overflow: as on CellRetrievalNetwork (they govern this module's OWN forward; inside a
        cell encoder the owning model's settings apply)."""
        super().__init__()
        assert args.pointnet_layers == 3 and args.pointnet_variation == 0  # models/pointcloud/pointnet2.py:55
        self.args = args
        self.add_self_loops = add_self_loops
        if precision not in ("f16x3", "fp32"):
            raise ValueError("precision must be 'f16x3' or 'fp32'")
        if on_overflow not in ("raise", "fp32"):
            raise ValueError("on_overflow must be 'raise' or 'fp32'")
        self.precision, self.on_overflow = precision, on_overflow
        self.tuning = 0
        self._pack, self._overflow = None, None
        self.sa1 = SetAbstractionLayer(0.5, 0.2, get_mlp([3 + 3, 32, 64]))
        self.sa2 = SetAbstractionLayer(0.5, 0.3, get_mlp([64 + 3, 128, 128]))
        self.sa3 = SetAbstractionLayer(0.5, 0.4, get_mlp([128 + 3, 256, 256]))
        self.ga = GlobalAbstractionLayer(get_mlp([256 + 3, 512, 1024]))
        self.lin1 = nn.Linear(1024, 512)
        self.lin2 = nn.Linear(512, 256)
        # unused on the retrieval path; the pre-training stage trains the trunk through class_classifier
        self.class_classifier = nn.Linear(256, num_classes)
        self.color_classifier = nn.Linear(256, num_colors)
        self.dim0, self.dim1, self.dim2 = 1024, 512, 256

    @property
    def radii(self):
        return (self.sa1.radius, self.sa2.radius, self.sa3.radius)

    @property
    def device(self):
        return next(self.lin1.parameters()).device

    # ---- the stand-alone classifier ------------------------------------------------------------------------------
    def forward(self, data):
        """data: data.Batch, or anything with .x (rgb), .pos and .batch: ONE PyG batch of n objects with
        args.pointnet_numpoints points each (models/pointcloud/pointnet2.py:80-100)."""
        from .data import _check_batch_vectors
        n_pts = int(getattr(self.args, "pointnet_numpoints", 256))
        pos, x, batch = data.pos, data.x, getattr(data, "batch", None)
        if batch is None:
            raise RuntimeError("PointNet2.forward: the batch has no batch vector")
        if pos.dim() != 2 or pos.shape[1] != 3 or tuple(x.shape) != tuple(pos.shape) or pos.shape[0] % n_pts != 0:
            raise RuntimeError(f"PointNet2.forward: x {tuple(x.shape)} / pos {tuple(pos.shape)} are not n objects of {n_pts} points x 3")
        n = pos.shape[0] // n_pts
        try:
            _check_batch_vectors([data], [n], n_pts)
        except RuntimeError:
            raise RuntimeError(f"PointNet2.forward: the batch vector is not {n} contiguous groups of {n_pts}") from None
        dev = self.device
        to = lambda t: t.detach().to(dev, torch.float32).reshape(n, n_pts, 3).contiguous()
        return self.forward_packed(to(pos), to(x))

    def _trunk_pack(self):
        x3 = self.precision == "f16x3"
        ver = (packing.params_version(self), str(self.device))
        if self._pack is None or self._pack[0] != ver or (x3 and not self._pack[3]):
            tensors = packing.pack_pointnet_weights(self, self.device, x3=x3)
            self._pack = (ver, tensors, ops.make_cell_weights(tensors), x3)
        return self._pack

    def forward_packed(self, xyz, rgb):
        """Device-resident inputs xyz / rgb [n, P, 3] (fp32), P from 8 to 256.  eval(): the folded inference kernels (under
        torch.no_grad(), as the cell encoder's); train(): the batch-statistics path, results carry a grad_fn and the BatchNorm
        running estimates move as nn.BatchNorm1d's do."""
        if xyz.dim() != 3 or tuple(rgb.shape) != tuple(xyz.shape) or xyz.shape[2] != 3:
            raise RuntimeError(f"PointNet2: xyz {tuple(xyz.shape)} / rgb {tuple(rgb.shape)} must both be [n_obj, n_pts, 3]")
        n = xyz.shape[0]
        if n > MAX_BATCH_OBJECTS:
            raise RuntimeError(f"PointNet2: {n} objects in one forward; the batch is one cell of at most {MAX_BATCH_OBJECTS} objects")
        if self.training:
            return self._forward_train(xyz, rgb)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("the inference kernels are forward-only (BatchNorm folded): call them under "
                                      "torch.no_grad(), or put the model in train() for the training-mode path")
        n_classes, n_colors = self.class_classifier.out_features, self.color_classifier.out_features

        def run():
            _, tensors, weights, _ = self._trunk_pack()
            cfg = ops.make_cell_config(n_pts=xyz.shape[1], self_loops=self.add_self_loops, radius=self.radii,
                                       precision=self.precision, tuning=self.tuning,
                                       overflow_flag=self._overflow_word() if self.precision == "f16x3" else None)
            return ops.pointnet2_forward(xyz, rgb, weights, cfg, tensors["head_w"], tensors["head_b"], n_classes, n_colors)
        return SimpleNamespace(**(self._with_guard(run) if n > 0 else run()))

    def _forward_train(self, xyz, rgb):
        from .train_cell import pointnet_trunk_train
        dev = xyz.device
        n = xyz.shape[0]
        # the batch is one cell: cell_ptr = [0, n], every object's cell starts at object 0 (two device-side fills: no host copy
        # queued behind the previous step's kernels)
        cell_ptr_dev = torch.zeros(2, dtype=torch.int32, device=dev)
        cell_ptr_dev[1:].fill_(n)
        first_obj = torch.zeros(n, dtype=torch.int32, device=dev)
        f0, f1, f2 = pointnet_trunk_train(self, xyz, rgb, first_obj, cell_ptr_dev, self.add_self_loops)
        return SimpleNamespace(features0=f0, features1=f1, features2=f2, class_pred=_head_train(f2, self.class_classifier),
                               color_pred=_head_train(f2, self.color_classifier))


def _head_train(x, lin: nn.Linear):
    """A classifier head in train() mode on train_ops.linear (tiled GEMM forward, dX and dW kernels): the GEMM's column
    granule is 8, so the weight rows are zero-padded to it (22 classes -> 24) and the pad columns cut off again."""
    from . import train_ops as TO
    n = lin.out_features
    pad = (-n) % 8
    if not pad:
        return TO.linear(x, lin)
    w = torch.nn.functional.pad(lin.weight, (0, 0, 0, pad))
    b = torch.nn.functional.pad(lin.bias, (0, pad)) if lin.bias is not None else None
    return TO._LinearFn.apply(x, w, b)[:, :n]
