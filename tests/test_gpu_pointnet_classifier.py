"""GPU tests (-m gpu) of stage one of the reference's training on the HIP path: PointNet++ as a classifier of its own
(models/pointcloud/pointnet2.py:80-100), its loss and its loop (training/pointcloud/pointnet2.py:24-67, :125-159), against the CPU
oracle (oracle.model.OraclePointNet2; class_pred = om.class_classifier(om(batch).features2)) and float64 torch.

Bars: features within the project's 1e-4; the logits within 1e-4 * max(1, r), r the largest row sum of |W| of the head (what the
1e-4 feature bar implies for a linear map of features2); the two new kernels alone within 1e-5 / the bars of
test_pairwise_ranking_loss_matches_reference_formula; the training step on the two-sided bar of
test_training_step_at_the_reference_batch_size."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _dev():
    return torch.device("cuda:0")


def _to_dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) for a in arrs]


def _batch(xyz, rgb, dtype=torch.float32):
    """n objects as ONE PyG-style batch, the way the reference's DataLoader hands them to PointNet2.forward."""
    from text2pos_amd import data as D
    n, p = xyz.shape[0], xyz.shape[1]
    return D.Batch(x=torch.from_numpy(rgb.reshape(n * p, 3)).to(dtype), pos=torch.from_numpy(xyz.reshape(n * p, 3)).to(dtype),
                   batch=torch.arange(n).repeat_interleave(p))


def _args(**kw):
    from text2pos_amd import synthetic as S
    return S.default_args(**kw)


@pytest.fixture
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))   # the oracle's eager graph: 8-16 intra-op threads are fastest
    yield
    torch.set_num_threads(n)


# ---------------------------------------------------------------------------------------------------------------
# 1. eval parity
# ---------------------------------------------------------------------------------------------------------------
_ORACLE_EVAL = {}


def _oracle_eval(n, n_pts, self_loops):
    """(oracle model, objects, its outputs on the single batch) for the golden weights; shared by the two precisions."""
    import weights as W
    from oracle import model as OM
    from text2pos_amd import synthetic as S
    key = (n, n_pts, self_loops)
    if key not in _ORACLE_EVAL:
        om = OM.OraclePointNet2(22, 8, self_loops).eval()
        W.fill_state_dict(om, 11)
        xyz, rgb, _, _ = S.make_objects(41, 0, n, n_pts)
        with torch.no_grad():
            o = om(_batch(xyz, rgb))
            want = dict(features0=o.features0, features1=o.features1, features2=o.features2,
                        class_pred=om.class_classifier(o.features2), color_pred=om.color_classifier(o.features2))
        _ORACLE_EVAL[key] = (om, xyz, rgb, want)
    return _ORACLE_EVAL[key]


@pytest.mark.parametrize("self_loops", [True, False])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("n_pts", [256, 100])
@pytest.mark.parametrize("n", [1, 32, 300])
def test_eval_forward_matches_the_oracle_on_one_batch(n, n_pts, precision, self_loops, _oracle_threads):
    """PointNet2(...)(batch) in eval(): features0 / 1 / 2, class_pred, color_pred against the oracle run on the SAME single PyG
    batch - PointConv's self-loop rewrite aliases dense row i of the BATCH onto centroid row i of the batch (300 objects: twice
    the largest cell the cell-encoder tests fuzz).  The eval kernels are the cell encoder's trunk with cell_ptr = [0, n]."""
    import text2pos_amd as t2p
    om, xyz, rgb, want = _oracle_eval(n, n_pts, self_loops)
    hm = t2p.PointNet2(22, 8, _args(pointnet_numpoints=n_pts), add_self_loops=self_loops, precision=precision)
    hm.load_state_dict(om.state_dict(), strict=True)
    hm = hm.to(_dev()).eval()
    with torch.no_grad():
        got = hm(_batch(xyz, rgb))
        again = hm.forward_packed(*_to_dev(xyz, rgb))
    assert hm.overflow_detected() == 0
    for name, dim in (("features0", 1024), ("features1", 512), ("features2", 256), ("class_pred", 22), ("color_pred", 8)):
        g = getattr(got, name)
        assert tuple(g.shape) == (n, dim) and g.dtype == torch.float32 and g.is_cuda, name
        assert torch.equal(g, getattr(again, name)), name           # forward(data) is forward_packed on the same arrays
    errs = {k: (getattr(got, k).cpu() - want[k]).abs().max().item() for k in want}
    print(f"n={n} P={n_pts} {precision} self_loops={self_loops}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["features0"] < TOL and errs["features2"] < TOL and errs["features1"] < TOL, errs
    for head, lin in (("class_pred", om.class_classifier), ("color_pred", om.color_classifier)):
        r = float(lin.weight.detach().abs().sum(1).max())           # |W f - W f'| <= max row sum of |W| * max |f - f'|
        assert errs[head] < TOL * max(1.0, r), (head, errs[head], r)


def test_eval_forward_refuses_gradients_and_reports_the_guard(_oracle_threads):
    """As on CellRetrievalNetwork: the folded kernels are forward-only, and the guard word / on_overflow act on this model's own
    f16x3 calls (a checkpoint scaled out of fp16's range raises, or is recomputed on fp32 with a warning)."""
    import text2pos_amd as t2p
    om, xyz, rgb, want = _oracle_eval(32, 256, True)
    hm = t2p.PointNet2(22, 8, _args())
    hm.load_state_dict(om.state_dict(), strict=True)
    hm = hm.to(_dev()).eval()
    with pytest.raises(NotImplementedError, match="forward-only"):
        hm.forward_packed(*_to_dev(xyz, rgb))
    sd = {k: v.clone() for k, v in om.state_dict().items()}
    key = "sa3.point_conv.local_nn.0.1."                  # the BatchNorm behind SA3's first Linear: activations past 65504
    sd[key + "weight"], sd[key + "bias"] = sd[key + "weight"] * 3.0e5, sd[key + "bias"] * 3.0e5
    hot = t2p.PointNet2(22, 8, _args())
    hot.load_state_dict(sd, strict=True)
    hot = hot.to(_dev()).eval()
    with torch.no_grad():
        with pytest.raises(FloatingPointError, match="0x"):
            hot.forward_packed(*_to_dev(xyz, rgb))
        assert hot.overflow_detected() == 0
        hot.on_overflow = "fp32"
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            redone = hot.forward_packed(*_to_dev(xyz, rgb))
        assert any("fp32" in str(w.message) for w in caught)
        hot.precision = "fp32"
        exact = hot.forward_packed(*_to_dev(xyz, rgb))
    assert torch.equal(redone.class_pred, exact.class_pred) and torch.equal(redone.features0, exact.features0)


# ---------------------------------------------------------------------------------------------------------------
# 2. the heads kernel alone
# ---------------------------------------------------------------------------------------------------------------
def test_heads_kernel_matches_float64_on_the_gpus_own_features(_oracle_threads):
    import text2pos_amd as t2p
    from text2pos_amd import ops
    om, xyz, rgb, _ = _oracle_eval(300, 256, True)
    hm = t2p.PointNet2(22, 8, _args())
    hm.load_state_dict(om.state_dict(), strict=True)
    hm = hm.to(_dev()).eval()
    with torch.no_grad():
        out = hm.forward_packed(*_to_dev(xyz, rgb))
    f2 = out.features2
    pack = hm._trunk_pack()[1]
    cls, col = ops.classifier_heads(f2, pack["head_w"], pack["head_b"], 22, 8)
    assert torch.equal(cls, out.class_pred) and torch.equal(col, out.color_pred)      # the forward IS this kernel on features2
    f64 = f2.cpu().double()
    for got, lin in ((cls, hm.class_classifier), (col, hm.color_classifier)):
        want = f64 @ lin.weight.detach().cpu().double().t() + lin.bias.detach().cpu().double()
        err = (got.cpu().double() - want).abs().max().item()
        print(f"heads on the GPU's features2: {lin.out_features} logits, max error {err:.2e}")
        assert err < 1e-5
        top2 = want.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-5
        assert int(clear.sum()) > 0
        assert torch.equal(got.cpu().argmax(1)[clear], want.argmax(1)[clear])


@pytest.mark.parametrize("n,c1,c2", [(1, 22, 8), (7, 1, 1), (1000, 64, 64), (33, 5, 64), (4097, 22, 8)])
def test_heads_kernel_shapes(n, c1, c2):
    """Both heads in one launch for every supported width (1 .. 64 each), row counts that do not fill a pass, grid-stride passes."""
    from text2pos_amd import ops
    g = torch.Generator().manual_seed(n + c1)
    f2 = torch.relu(torch.randn(n, 256, generator=g))
    w = torch.randn(256, c1 + c2, generator=g) / 16.0
    b = torch.randn(c1 + c2, generator=g)
    cls, col = ops.classifier_heads(f2.to(_dev()), w.to(_dev()), b.to(_dev()), c1, c2)
    want = f2.double() @ w.double() + b.double()
    assert tuple(cls.shape) == (n, c1) and tuple(col.shape) == (n, c2)
    assert (torch.cat([cls, col], 1).cpu().double() - want).abs().max().item() < 1e-5
    with pytest.raises(Exception, match=r"outside \[1, 64\]"):
        ops.classifier_heads(f2.to(_dev()), torch.zeros(256, 65 + c2, device=_dev()), torch.zeros(65 + c2, device=_dev()), 65, c2)


# ---------------------------------------------------------------------------------------------------------------
# 3. the cross-entropy kernel alone
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 8, 22, 64])
@pytest.mark.parametrize("n", [1, 32, 257])
def test_cross_entropy_matches_float64(n, c):
    """losses.CrossEntropyLoss against float64 F.cross_entropy: loss within 1e-5 * max(1, |loss|), gradient within 1e-4 of its
    largest entry (the bars of test_pairwise_ranking_loss_matches_reference_formula), hit count equal to torch's, ties to the
    lower index; logits of +-80 stay finite (the row maximum is subtracted before exp)."""
    import text2pos_amd as t2p
    g = torch.Generator().manual_seed(100 * n + c)
    for scale in (3.0, 80.0):
        logits = torch.randn(n, c, generator=g) * scale
        if scale == 80.0:
            logits = logits.clamp(-80.0, 80.0)
            logits[0, 0], logits[0, c - 1] = 80.0, -80.0
        if n > 2:
            logits[1, :] = logits[1, 0]                         # a row of ties: argmax 0
            logits[2, c - 1] = logits[2].max()                  # a tie between the last column and an earlier one
        y = torch.randint(0, c, (n,), generator=g)
        if n > 2:
            y[1], y[2] = 0, int(logits[2].argmax())
        ref_in = logits.double().requires_grad_(True)
        ref = F.cross_entropy(ref_in, y)
        ref.backward()
        crit = t2p.CrossEntropyLoss()
        x = logits.to(_dev()).requires_grad_(True)
        loss = crit(x, y.to(_dev()))
        loss.backward()
        assert torch.isfinite(loss).item() and torch.isfinite(x.grad).all().item()
        e_loss = abs(loss.item() - ref.item())
        e_grad = (x.grad.cpu().double() - ref_in.grad).abs().max().item()
        print(f"n={n} C={c} scale={scale}: loss {loss.item():.6f} (error {e_loss:.2e}), gradient error {e_grad:.2e} of {ref_in.grad.abs().max().item():.2e}")
        assert e_loss < 1e-5 * max(1.0, abs(ref.item()))
        assert e_grad < 1e-4 * ref_in.grad.abs().max().item()
        want_hits = logits.double().argmax(1) == y
        assert crit.last_correct.dtype == torch.int32 and torch.equal(crit.last_correct.cpu().bool(), want_hits)
        # a second call is bit-identical (no atomics), and a scaled upstream gradient scales the result
        x2 = logits.to(_dev()).requires_grad_(True)
        (2.0 * crit(x2, y.to(_dev()))).backward()
        assert torch.equal(x2.grad, 2.0 * x.grad)


def test_cross_entropy_on_a_column_slice_and_out_of_range_labels():
    import text2pos_amd as t2p
    from text2pos_amd import ops
    g = torch.Generator().manual_seed(8)
    wide = torch.randn(40, 32, generator=g).to(_dev())
    y = torch.randint(0, 22, (40,), generator=g)
    row_loss, d, hits = ops.softmax_xent(wide[:, :22], y.to(_dev(), torch.int32))           # row pitch 32, 22 classes
    ref = F.cross_entropy(wide[:, :22].cpu().double(), y, reduction="none")
    assert (row_loss.cpu().double() - ref).abs().max().item() < 1e-5
    assert tuple(d.shape) == (40, 22) and int(hits.sum()) == int((wide[:, :22].cpu().argmax(1) == y).sum())
    crit = t2p.CrossEntropyLoss()
    for bad in (22, -1, 1 << 20):
        yb = y.clone()
        yb[17] = bad
        row_loss, d, hits = ops.softmax_xent(wide[:, :22], yb.to(_dev(), torch.int32))
        assert torch.isnan(row_loss[17]).item() and torch.isnan(d[17]).all().item() and int(hits[17]) == 0
        keep = torch.arange(40) != 17
        assert torch.isfinite(row_loss.cpu()[keep]).all().item() and torch.isfinite(d.cpu()[keep]).all().item()
        with pytest.raises(IndexError, match=rf"target {bad} of row 17 is outside \[0, 22\)"):
            crit(wide[:, :22].contiguous(), yb.to(_dev()))
    with pytest.raises(FloatingPointError, match="NaN among the logits"):
        crit(torch.full((4, 22), float("nan"), device=_dev()), torch.zeros(4, dtype=torch.long, device=_dev()))


# ---------------------------------------------------------------------------------------------------------------
# 4. one training step against float64 autograd
# ---------------------------------------------------------------------------------------------------------------
def test_training_step_matches_float64_autograd(_oracle_threads):
    """model.train(); output = model(batch); loss = criterion(output.class_pred, batch.y); loss.backward()
    (training/pointcloud/pointnet2.py:34-38) at the reference's batch size, 32 objects x 256 points, against torch.autograd
    through the oracle in FLOAT64 (same weights, same fp32 geometry).  The batch is ONE segment for every BatchNorm and one
    cell for the self-loop rewrite.  Bar: the two-sided one of test_training_step_at_the_reference_batch_size, unchanged - per
    parameter, error over max(1e-2 g_all, |g|max) below max(5e-3, 1.5 x the fp32 oracle's own deviation) and below 5e-2, at
    least 85 % of the parameters below 5e-3 outright, biases in front of a BatchNorm skipped; loss within 2e-6 relative;
    running estimates within 1e-4.  (On the CPU the fp32 oracle alone keeps all 30 compared parameters below 5e-3 for these
    inputs, worst 4.2e-3 in sa3.point_conv.local_nn.1.0.weight.)"""
    import weights as W
    import text2pos_amd as t2p
    from oracle import model as OM
    from text2pos_amd import synthetic as S
    xyz, rgb, _, _ = S.make_objects(91, 0, 32)
    shape, color, _ = S.object_attributes(91, 0, 32)
    y = torch.from_numpy((shape * 7 + color) % 22)

    def oracle(dtype):
        om = OM.OraclePointNet2(22, 8)
        W.fill_state_dict(om, 23)
        om.train()
        om = om.to(dtype)
        for p in om.parameters():
            p.requires_grad_(True)
        loss = F.cross_entropy(om.class_classifier(om(_batch(xyz, rgb, dtype)).features2), y)
        loss.backward()
        return om, loss

    sd0 = OM.OraclePointNet2(22, 8)
    W.fill_state_dict(sd0, 23)
    om32, l32 = oracle(torch.float32)
    om64, l64 = oracle(torch.float64)
    hm = t2p.PointNet2(22, 8, _args())
    hm.load_state_dict(sd0.state_dict(), strict=True)
    hm = hm.to(_dev()).train()
    out = hm(_batch(xyz, rgb))
    assert out.class_pred.requires_grad and out.features0.requires_grad and tuple(out.color_pred.shape) == (32, 8)
    lh = t2p.CrossEntropyLoss()(out.class_pred, y.to(_dev()))
    lh.backward()
    print(f"loss: HIP {lh.item():.8f}, float64 {l64.item():.8f}, fp32 oracle {l32.item():.8f}")
    assert abs(lh.item() - l64.item()) < 2e-6 * abs(l64.item()), (lh.item(), l64.item(), l32.item())
    r32, r64 = dict(om32.named_parameters()), dict(om64.named_parameters())
    g_all = max(float(q.grad.abs().max()) for q in r64.values() if q.grad is not None)
    bn = dict(om32.named_buffers())
    rows = []
    for name, p in hm.named_parameters():
        g = r64[name].grad
        if name.startswith("color_classifier."):          # not in the loss: no gradient on either side
            assert g is None and (p.grad is None or float(p.grad.abs().max()) == 0.0), name
            continue
        assert g is not None and p.grad is not None, name
        if name.endswith(".0.bias") and name[:-len(".0.bias")] + ".1.running_mean" in bn:
            continue                                      # bias in front of a BatchNorm: zero gradient, rounding noise on both sides
        scale = max(1e-2 * g_all, g.abs().max().item())
        e32 = (r32[name].grad.double() - g).abs().max().item() / scale
        eh = (p.grad.cpu().double() - g).abs().max().item() / scale
        rows.append((eh, e32, name))
    for eh, e32, name in sorted(rows, reverse=True):
        print(f"  {name}: HIP {eh:.2e}, fp32 oracle {e32:.2e}")
    for eh, e32, name in rows:
        assert eh < max(5e-3, 1.5 * e32) and eh < 5e-2, (name, eh, e32)
    assert len(rows) == 30 and sum(r[0] < 5e-3 for r in rows) >= 0.85 * len(rows), sorted(rows, reverse=True)[:6]
    rb, hb = dict(om64.named_buffers()), dict(hm.named_buffers())
    worst = 0.0
    for name, b in hb.items():
        if name.endswith("running_mean") or name.endswith("running_var"):
            err = (b.cpu().double() - rb[name]).abs().max().item()
            worst = max(worst, err)
            assert err < 1e-4, (name, err)
        elif name.endswith("num_batches_tracked"):
            assert int(b) == int(rb[name]) == 1, name
    print(f"running estimates: worst deviation {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------
# 5. learning
# ---------------------------------------------------------------------------------------------------------------
def _stream_batch(seed, lo, hi):
    from text2pos_amd import synthetic as S
    xyz, rgb, _, _ = S.make_objects(seed, lo, hi)
    b = _batch(xyz, rgb)
    b.y = torch.from_numpy(S.object_attributes(seed, lo, hi)[0])
    return b


def test_pretraining_loop_learns_as_the_oracle_does(_oracle_threads):
    """160 Adam steps (lr 10^-2.5, batch 32: objects 32 s .. 32 s + 31 of stream 77 at step s, label = the generator's shape class)
    of training.train_pointnet_epoch, then training.val_pointnet_epoch in eval() on objects 100,000 - 100,255 in four batches of 64
    - and the same loop on the CPU oracle from the same initial weights (torch's default init under manual_seed(5)).  Trajectories
    are chaotic (two runs of the oracle differ in the third digit of the loss by step 10), so the bar is coarse: the HIP accuracy
    reaches at least half of the oracle's gain over the majority-class rate m of the held-out labels; the oracle itself must
    reach 0.85, otherwise the comparison says nothing and the test fails as inconclusive.  Also: the mean training loss of the
    last 10 steps is below that of the first 10."""
    import text2pos_amd as t2p
    from oracle import model as OM
    from text2pos_amd import training as T
    steps, lr = 160, 10 ** -2.5
    train = [_stream_batch(77, 32 * s, 32 * s + 32) for s in range(steps)]
    val = [_stream_batch(77, 100000 + 64 * i, 100000 + 64 * i + 64) for i in range(4)]
    labels = torch.cat([b.y for b in val])
    m = float(torch.bincount(labels).max()) / labels.numel()

    torch.manual_seed(5)
    om = OM.OraclePointNet2(22, 8)
    hm = t2p.PointNet2(22, 8, _args(), on_overflow="fp32")      # (a guard verdict would be recomputed and warned about, not hidden)
    hm.load_state_dict(om.state_dict(), strict=True)
    hm = hm.to(_dev())

    opt = torch.optim.Adam(hm.parameters(), lr=lr)
    crit = t2p.CrossEntropyLoss()
    tens = [T.train_pointnet_epoch(hm, train[i: i + 10], opt, crit) for i in range(0, steps, 10)]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        a_hip = T.val_pointnet_epoch(hm, val)
    assert not hm.training
    print(f"HIP: loss first 10 steps {tens[0][0]:.4f}, last 10 {tens[-1][0]:.4f}; train accuracy {tens[0][1]:.3f} -> {tens[-1][1]:.3f}; "
          f"held-out accuracy {a_hip:.4f} (guard warnings: {len(caught)})")
    assert tens[-1][0] < tens[0][0]

    om.train()
    o_opt = torch.optim.Adam(om.parameters(), lr=lr)
    o_losses = []
    for b in train:                                             # training/pointcloud/pointnet2.py:30-41 on the oracle
        o_opt.zero_grad()
        loss = F.cross_entropy(om.class_classifier(om(b).features2), b.y)
        loss.backward()
        o_opt.step()
        o_losses.append(loss.item())
    om.eval()
    with torch.no_grad():
        a_oracle = float(np.mean([(om.class_classifier(om(b).features2).argmax(1) == b.y).float().mean().item() for b in val]))
    print(f"oracle: loss first 10 steps {np.mean(o_losses[:10]):.4f}, last 10 {np.mean(o_losses[-10:]):.4f}; held-out accuracy "
          f"{a_oracle:.4f}; majority-class rate {m:.4f}; bar {m + 0.5 * (a_oracle - m):.4f}")
    assert a_oracle >= 0.85, f"inconclusive: the oracle itself reached only {a_oracle:.3f}"
    assert a_hip >= m + 0.5 * (a_oracle - m), (a_hip, a_oracle, m)


# ---------------------------------------------------------------------------------------------------------------
# 6. round trip through args.pointnet_path, 7. pointnet_freeze
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pretrained_path(tmp_path_factory):
    """pretrain_pointnet.py at a few steps (2 epochs of 4 batches): the file args.pointnet_path names."""
    import pretrain_pointnet as PP
    path = str(tmp_path_factory.mktemp("pointnet") / "pointnet_pretrained.pth")
    records = PP.pretrain(PP.fresh_model(), path, epochs=2, train_objects=128, val_objects=64)
    assert len(records) == 2 and os.path.exists(path)
    return path


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_pretrained_file_round_trips_into_the_cell_encoder(pretrained_path, vocab, precision):
    """torch.save(model.state_dict(), path) -> CellRetrievalNetwork(..., args.pointnet_path = path): on a one-cell batch the
    cell encoder's features2 is bit-identical to PointNet2.forward_packed of the same objects (the same kernels on the same
    weights); the file also loads into the oracle with strict=True."""
    import text2pos_amd as t2p
    from oracle import model as OM
    from text2pos_amd import synthetic as S
    sd = torch.load(pretrained_path, map_location="cpu")
    OM.OraclePointNet2(22, 8).load_state_dict(sd, strict=True)
    assert int(sd["lin1.weight"].shape[0]) == 512 and int(sd["sa1.point_conv.local_nn.0.1.num_batches_tracked"]) == 8
    pn = t2p.PointNet2(22, 8, _args(), precision=precision)
    pn.load_state_dict(sd, strict=True)
    pn = pn.to(_dev()).eval()
    # (the coarse model's own heads have len(known_classes) = 22 and 8 outputs as well: the file fits strictly)
    cm = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], _args(pointnet_path=pretrained_path),
                                  precision=precision).to(_dev()).eval()
    for k, v in sd.items():
        assert torch.equal(cm.object_encoder.pointnet.state_dict()[k].cpu(), v), k
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(57, 1, fixed_n=20)
    with torch.no_grad():
        _, trace = cm.encode_objects_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, want_trace=("features0", "features1", "features2"))
        out = pn.forward_packed(*_to_dev(xyz, rgb))
    assert cm.overflow_detected() == 0 and pn.overflow_detected() == 0
    for name in ("features0", "features1", "features2"):
        assert torch.equal(trace[name], getattr(out, name)), name
    assert float(out.features2.abs().max()) > 0.0


def test_frozen_pretrained_trunk_in_a_coarse_training_step(pretrained_path, vocab):
    """args.pointnet_path + args.pointnet_freeze = True in one step of training/coarse.py:31-62, as the reference does it
    (models/object_encoder.py:46-49: load, then requires_grad_(False)): the trunk's parameters get no gradient, their BatchNorm
    running estimates still move (requires_grad_(False) does not stop them: one update per cell), everything else that takes
    part trains - with the same gradients as without the freeze."""
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    n_cells = 8
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(63, n_cells)
    texts = S.make_texts(63, 0, n_cells)

    def step(freeze):
        torch.manual_seed(7)
        m = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"],
                                     _args(pointnet_path=pretrained_path, pointnet_freeze=freeze)).to(_dev())
        m.train()
        before = {k: v.clone() for k, v in m.object_encoder.pointnet.state_dict().items()}
        loss = t2p.PairwiseRankingLoss(0.35)(m.encode_text(texts), m.encode_objects_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr))
        loss.backward()
        return m, before, loss

    frozen, before, l_frozen = step(True)
    free, _, l_free = step(False)
    assert abs(l_frozen.item() - l_free.item()) <= 1e-6 * abs(l_free.item())      # the same forward
    trunk = "object_encoder.pointnet."
    unused = ("object_encoder.class_embedding.", "object_encoder.color_embedding.")     # class_embed / color_embed are off
    g_free = {k: p.grad for k, p in free.named_parameters()}
    buffers = dict(frozen.named_buffers())
    before_bn = lambda name: name.endswith(".0.bias") and name[:-len(".0.bias")] + ".1.running_mean" in buffers
    trained = 0
    for name, p in frozen.named_parameters():
        if name.startswith(trunk):
            assert not p.requires_grad and p.grad is None, name
            if not name.startswith((trunk + "class_classifier", trunk + "color_classifier")) and not before_bn(name):
                assert g_free[name] is not None and float(g_free[name].abs().max()) > 0.0, name      # (it WOULD train)
            continue
        if name.startswith(unused):
            continue
        assert p.requires_grad and p.grad is not None and torch.isfinite(p.grad).all().item(), name
        if before_bn(name):
            continue                                           # zero gradient, rounding noise on both sides
        ref = g_free[name]
        assert float(ref.abs().max()) > 0.0, name
        assert (p.grad - ref).abs().max().item() <= 1e-4 * float(ref.abs().max()), name   # (float atomics in the scatter backward)
        trained += 1
    assert trained >= 25
    after = frozen.object_encoder.pointnet.state_dict()
    moved = 0
    for k, v in after.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + n_cells, k       # one PointNet++ call per cell
        elif k.endswith("running_mean") or k.endswith("running_var"):
            assert not torch.equal(v, before[k]), k
            other = free.object_encoder.pointnet.state_dict()[k]
            assert (v - other).abs().max().item() <= 1e-6 * max(1.0, float(other.abs().max())), k
            moved += 1
        else:
            assert torch.equal(v, before[k]), k                # weights untouched by the step
    assert moved == 16
    # an optimizer over the trainable parameters leaves the trunk alone
    opt = torch.optim.Adam([p for p in frozen.parameters() if p.requires_grad], lr=1e-3)
    opt.step()
    for k, v in frozen.object_encoder.pointnet.named_parameters():
        assert torch.equal(v, before[k].to(v.device)), k
