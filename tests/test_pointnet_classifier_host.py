"""CPU tests of the PointNet++ pre-training surface (stage one of the reference, training/pointcloud/pointnet2.py): what
imports and validates without a GPU.  The arithmetic is tested in tests/test_gpu_pointnet_classifier.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import text2pos_amd as t2p
from text2pos_amd import _lib, data as D, ops, packing, synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("t2p_pointnet2_workspace_bytes", "t2p_pointnet2_forward", "t2p_classifier_heads", "t2p_softmax_xent")


def test_loss_and_epoch_functions_import_without_the_library(monkeypatch):
    """losses.CrossEntropyLoss and the two epoch functions are plain Python around the C ABI: importing and constructing them
    loads nothing; using them without the library fails loudly (no fall-back to torch's cross entropy)."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libt2p_hip.so")
    from text2pos_amd import losses, training
    assert t2p.CrossEntropyLoss is losses.CrossEntropyLoss
    crit = losses.CrossEntropyLoss()
    assert callable(training.train_pointnet_epoch) and callable(training.val_pointnet_epoch)
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(torch.zeros(4, 22), torch.zeros(4, dtype=torch.long))
    assert np.isnan(training.val_pointnet_epoch(t2p.PointNet2(22, 8, S.default_args()), []))   # an empty loader: np.mean([])


def test_cross_entropy_rejects_malformed_calls():
    crit = t2p.CrossEntropyLoss()
    with pytest.raises(RuntimeError, match=r"\[n, C\]"):
        crit(torch.zeros(4), torch.zeros(4, dtype=torch.long))
    with pytest.raises(RuntimeError, match=r"\[n, C\]"):
        crit(torch.zeros(4, 3), torch.zeros(5, dtype=torch.long))
    with pytest.raises(RuntimeError, match="class indices"):
        crit(torch.zeros(4, 3), torch.zeros(4))
    with pytest.raises(RuntimeError, match="empty batch"):
        crit(torch.zeros(0, 3), torch.zeros(0, dtype=torch.long))


def test_state_dict_keys_equal_the_oracles():
    from oracle import model as OM
    om = OM.OraclePointNet2(22, 8)
    hm = t2p.PointNet2(22, 8, S.default_args())
    assert list(hm.state_dict().keys()) == list(om.state_dict().keys())
    assert all(hm.state_dict()[k].shape == v.shape for k, v in om.state_dict().items())
    hm.load_state_dict(om.state_dict(), strict=True)
    assert hm.add_self_loops is True and hm.precision == "f16x3"
    assert t2p.PointNet2(22, 8, S.default_args(), add_self_loops=False).add_self_loops is False
    # the trunk inside an ObjectEncoder is the same class with the same keys (models/object_encoder.py:44-46)
    oe = t2p.ObjectEncoder(256, S.LABELS + ["pad"], S.COLOR_NAMES, S.default_args())
    assert isinstance(oe.pointnet, t2p.PointNet2)
    assert list(oe.pointnet.state_dict().keys()) == list(OM.OraclePointNet2(len(S.LABELS) + 1, len(S.COLOR_NAMES)).state_dict().keys())


def _batch(n, n_pts, seed=3):
    xyz, rgb, _, _ = S.make_objects(seed, 0, n, n_pts)
    return D.Batch(x=torch.from_numpy(rgb.reshape(-1, 3)), pos=torch.from_numpy(xyz.reshape(-1, 3)),
                   batch=torch.arange(n).repeat_interleave(n_pts))


def test_batch_vector_validation_rejects_a_permuted_vector():
    """PointNet2.forward checks the batch vector the way data._check_batch_vectors does for the cell encoder: n contiguous
    groups of pointnet_numpoints.  The check runs before anything touches the device."""
    m = t2p.PointNet2(22, 8, S.default_args(pointnet_numpoints=64))
    b = _batch(5, 64)
    perm = torch.randperm(b.batch.shape[0], generator=torch.Generator().manual_seed(1))
    b.batch = b.batch[perm]
    with pytest.raises(RuntimeError, match="5 contiguous groups of 64"):
        m(b)
    b = _batch(5, 64)
    b.batch = b.batch.flip(0).contiguous()                      # contiguous groups, wrong order
    with pytest.raises(RuntimeError, match="contiguous groups"):
        m(b)
    b = _batch(5, 64)
    b.batch = None
    with pytest.raises(RuntimeError, match="no batch vector"):
        m(b)
    b = _batch(5, 64)
    b.pos, b.x = b.pos[:-1], b.x[:-1]                           # not a whole number of objects
    with pytest.raises(RuntimeError, match="64 points"):
        m(b)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):  # a well-formed batch gets as far as the device check
        with torch.no_grad():
            m.eval()(_batch(5, 64))


def test_batches_larger_than_a_chunk_are_refused():
    m = t2p.PointNet2(22, 8, S.default_args()).eval()
    z = torch.zeros(65536, 8, 3)
    with pytest.raises(RuntimeError, match="65535"):
        m.forward_packed(z, z)


def test_forward_wording_is_no_longer_shared_with_the_object_encoder():
    oe = t2p.ObjectEncoder(256, S.LABELS + ["pad"], S.COLOR_NAMES, S.default_args())
    with pytest.raises(NotImplementedError, match="ObjectEncoder runs fused"):
        oe(None, None)
    src = open(os.path.join(ROOT, "text2pos-cvpr2022_amd", "pointnet2.py")).read()
    assert "no stand-alone forward" not in src


def test_new_symbols_are_declared_bound_and_exported():
    handle = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, f"{name} missing from include/t2p.h"
        assert hasattr(handle, name), f"{name} not exported by libt2p_hip.so"
    assert _lib.ABI_VERSION == handle.t2p_abi_version()


def test_pointnet2_workspace_query_and_argument_checks_need_no_gpu():
    L = _lib.lib()
    cfg = ops.make_cell_config()
    a, b = L.t2p_pointnet2_workspace_bytes(32, cfg), L.t2p_pointnet2_workspace_bytes(512, cfg)
    assert 0 < a < b < 1 << 30
    # the trunk alone needs no more than the whole cell encoder on one cell of the same objects
    assert b <= L.t2p_encode_cells_workspace_bytes(512, 1, cfg)
    w = _lib.CellWeights()
    one = torch.zeros(256)
    ptr = lambda t: t.data_ptr()
    # more classes than the heads kernel is built for: T2P_E_UNSUPPORTED before anything is launched
    rc = L.t2p_classifier_heads(ptr(one), ptr(one), ptr(one), 1, 65, 8, ptr(one), ptr(one), None)
    assert rc == -3 and b"outside [1, 64]" in L.t2p_last_error()
    rc = L.t2p_pointnet2_forward(ptr(one), ptr(one), 1, w, cfg, ptr(one), ptr(one), 22, 100, None, None, None, ptr(one), ptr(one),
                                 ptr(one), 1 << 20, None)
    assert rc == -3
    rc = L.t2p_pointnet2_forward(ptr(one), ptr(one), 70000, w, cfg, None, None, 0, 0, None, None, None, None, None, ptr(one), 1 << 20,
                                 None)
    assert rc == -1 and b"limited to 65535" in L.t2p_last_error()
    rc = L.t2p_softmax_xent(ptr(one), 4, ptr(one), 2, 8, ptr(one), ptr(one), 8, ptr(one), None)
    assert rc == -1 and b"row pitch" in L.t2p_last_error()


def test_trunk_pack_is_the_cell_encoders_pack():
    """packing.pack_pointnet_weights is the trunk's part of pack_cell_weights, factored out: for the same PointNet2 weights the
    two give the same tensors bit for bit (fp32 matrices, f16x3 images, scales, guard norms)."""
    import weights as W
    torch.manual_seed(0)
    cm = t2p.CellRetrievalNetwork(S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words(), S.default_args())
    W.fill_state_dict(cm, 11)
    cell = packing.pack_cell_weights(cm, "cpu", x3=True)
    pn = cm.object_encoder.pointnet
    trunk = packing.pack_pointnet_weights(pn, "cpu", x3=True)
    same = lambda a, b: torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
    for key, val in trunk.items():
        if key in ("head_w", "head_b"):
            continue
        other = cell[key]
        if isinstance(val, list):
            assert len(val) == len(other) and all((a is None and b is None) or same(a, b) for a, b in zip(val, other)), key
        else:
            assert same(val, other), key
    assert {"sa_w2_x3", "ga_w2_x3", "lin1_x3", "lin2_x3", "ga_w1_l1", "sa_wp_l1"} <= set(trunk)
    assert not {"pn_w", "merge_w", "g_wp"} & set(trunk)
    n1, n2 = pn.class_classifier.out_features, pn.color_classifier.out_features
    assert tuple(trunk["head_w"].shape) == (256, n1 + n2)
    assert torch.equal(trunk["head_w"][:, :n1], pn.class_classifier.weight.detach().t())
    assert torch.equal(trunk["head_w"][:, n1:], pn.color_classifier.weight.detach().t())
    assert torch.equal(trunk["head_b"], torch.cat([pn.class_classifier.bias, pn.color_classifier.bias]).detach())


def test_pretrain_script_help_runs_and_batches_carry_labels():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pretrain_pointnet.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--out" in r.stdout and "--lr-idx" in r.stdout
    import pretrain_pointnet as PP
    b = PP.object_batch(7, 10, 14, 32)
    shape, _, _ = S.object_attributes(7, 10, 14)
    assert b.y.tolist() == shape.tolist() and b.pos.shape == (4 * 32, 3) and b.batch.view(4, 32)[:, 0].tolist() == [0, 1, 2, 3]
    assert abs(float(np.logspace(-2, -4.0, 5)[PP.DEFAULTS["lr_idx"]]) - 10 ** -2.5) < 1e-12 and PP.DEFAULTS["batch"] == 32


def test_model_pickles_without_its_device_caches():
    import pickle
    m = t2p.PointNet2(22, 8, S.default_args())
    m._pack, m._overflow = ("stale", lambda: None), torch.zeros(1)          # (what a pickle cannot carry)
    clone = pickle.loads(pickle.dumps(m))
    assert clone._pack is None and clone._overflow is None
    assert list(clone.state_dict().keys()) == list(m.state_dict().keys())
