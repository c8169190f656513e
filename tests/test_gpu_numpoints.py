"""args.pointnet_numpoints other than 256 (8 to 256 points per object; training/args.py:53): every layer of the cell encoder at the
object sizes a model may be trained with, on both arithmetic paths, against the CPU oracle (which is generic in the point count).

At 256 points the specialised f16x3 SA kernels run; every other size takes the generic f16x3 SA kernel (the stream kernel of
csrc/ws_sa.hip) for the level shapes that are not the 256-point ones, and the GA max runs over groups of gp = next power of two >= the level-3 centroid
count (SA level 3 pads each object to gp rows with copies of its last centroid).
"""
import re

import numpy as np
import pytest
import torch

import knn_graph as KG

pytestmark = pytest.mark.gpu
TOL = 1e-4
LIGHT = ("obj_emb", "knn_idx")     # the trace check_cells needs
SIZES = [8, 16, 31, 64, 100, 128, 200, 255]


def _dev():
    return torch.device("cuda:0")


def _to_dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) for a in arrays]


def _levels(n_pts):
    """[(n_cent, C)] of the three SA levels for n_pts points per object."""
    out, nd = [], n_pts
    for c in (64, 128, 256):
        nc = (nd + 1) // 2
        out.append((nc, c))
        nd = nc
    return out


def _pair(vocab, n_pts, precision="f16x3", self_loops=True, **kw):
    """(oracle, product module on cuda:0) with the golden weights (seed 11) for n_pts points per object."""
    import weights as W
    import text2pos_amd as t2p
    from oracle import model as OM
    from text2pos_amd import synthetic as S
    om = OM.OracleCellRetrieval(vocab["classes"], vocab["colors"], vocab["words"], OM.default_args(pointnet_numpoints=n_pts, **kw),
                                add_self_loops=self_loops).eval()
    W.fill_state_dict(om, 11)
    hm = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(pointnet_numpoints=n_pts, **kw),
                                  precision=precision)
    hm.load_state_dict(om.state_dict(), strict=True)
    hm.add_self_loops = self_loops
    return om, hm.to(_dev()).eval()


def _check_cells(om, got, gtr, want, wtr, cell_ptr, tag):
    """Cell embeddings at the 1e-4 bar, every cell (tests/knn_graph.py): against the oracle where the kNN graphs agree, against the
    float64 oracle head on the kernel's graph where a proven near-tie picked another neighbour (at most one such cell); the
    kernel's lists a kNN graph of its own object embeddings.  gtr: the kernel's trace ("obj_emb", "knn_idx"), wtr: the oracle's."""
    got_knn = KG.global_knn(gtr["knn_idx"].cpu().numpy(), cell_ptr)
    viol = KG.knn_violation(got_knn, KG.normalized64(gtr["obj_emb"]), cell_ptr)
    assert viol <= 0, f"{tag}: a chosen neighbour is farther than an unchosen one by {viol:.2e} beyond fp32 rounding"
    emb = [d for d in wtr if "object_embeddings" in d][0]["object_embeddings"].numpy()
    flips, resolved, gap = KG.check_cells(np.asarray(got), got_knn, np.asarray(want), KG.oracle_knn(emb, cell_ptr), emb, cell_ptr,
                                          KG.float64_oracle(om), tag)
    assert len(flips) <= 1, f"{tag}: {len(flips)} cells with a kNN near-tie flip"
    print(f"[{tag}] {len(flips)} cells with a proven kNN near-tie flip (distance gap {gap:.1e}, resolved to {resolved:.2e}); "
          f"worst knn_violation {viol:.2e}")


def _stagewise(om, hm, cells, tag):
    xyz, rgb, center, mean_rgb, cell_ptr = cells
    n_pts = xyz.shape[1]
    tr = []
    want = om.encode_objects_packed(xyz, rgb, center, mean_rgb, cell_ptr, trace=tr).numpy()
    with torch.no_grad():
        got, gtr = hm.encode_objects_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, want_trace=True)
    n_obj = xyz.shape[0]
    pn = [d for d in tr if "sa" in d]
    for l, (nc, c) in enumerate(_levels(n_pts)):
        want_sa = torch.cat([d["sa"][l]["out"] for d in pn]).numpy()
        got_sa = gtr["sa_out"][l].cpu().numpy()[:, :c]
        assert got_sa.shape == want_sa.shape == (n_obj * nc, c), f"{tag} SA{l + 1} shape"
        err = np.abs(got_sa - want_sa).max()
        assert err < TOL, f"{tag} SA{l + 1} output {err:.2e}"
    for k in ("features0", "features2"):
        w = torch.cat([d[k] for d in pn]).numpy()
        err = np.abs(gtr[k].cpu().numpy() - w).max()
        assert err < TOL, f"{tag} {k} {err:.2e}"
    emb = [d for d in tr if "object_embeddings" in d][0]["object_embeddings"].numpy()
    err = np.abs(gtr["obj_emb"].cpu().numpy() - emb).max()
    assert err < TOL, f"{tag} object embeddings {err:.2e}"
    _check_cells(om, got.cpu().numpy(), gtr, want, tr, cell_ptr, tag)
    return got


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("n_pts", SIZES)
def test_stagewise_vs_oracle(vocab, n_pts, precision):
    from text2pos_amd import synthetic as S
    om, hm = _pair(vocab, n_pts, precision)
    _stagewise(om, hm, S.make_cells(300 + n_pts, 4, n_pts=n_pts), f"{n_pts} points {precision}")


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_self_loops_off(vocab, precision):
    from text2pos_amd import synthetic as S
    om, hm = _pair(vocab, 100, precision, self_loops=False)
    _stagewise(om, hm, S.make_cells(17, 4, n_pts=100), f"100 points, no self loops, {precision}")


@pytest.mark.parametrize("kw", [dict(variation=1), dict(pointnet_features=1, use_features=["class", "position"])],
                         ids=["variation1", "features1_class_position"])
def test_ablations_at_128(vocab, kw):
    from text2pos_amd import synthetic as S
    for precision in ("f16x3", "fp32"):
        om, hm = _pair(vocab, 128, precision, **kw)
        xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(23, 6, n_pts=128)
        wtr = []
        want = om.encode_objects_packed(xyz, rgb, center, mean_rgb, cell_ptr, trace=wtr).numpy()
        with torch.no_grad():
            got, gtr = hm.encode_objects_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, want_trace=LIGHT)
        _check_cells(om, got.cpu().numpy(), gtr, want, wtr, cell_ptr, f"{kw} {precision}")


def _odd_object(rng, kind, n):
    """The object shapes of tests/tools/fuzz_cells.py at n points."""
    def norm(p):
        p = p - p.mean(0, keepdims=True)
        return (p * (0.999999 / np.abs(p).max())).astype(np.float32)
    if kind == "few":            # 2 - 5 distinct points, repeated
        k = int(rng.choice([2, 3, 5]))
        base = rng.uniform(-1, 1, (k, 3))
        return norm(base[rng.integers(0, k, n)])
    if kind == "line":
        return norm(rng.uniform(-1, 1, (n, 1)) * rng.uniform(-1, 1, (1, 3)))
    if kind == "dense":          # every ball at its 32-neighbour cap
        p = rng.uniform(-0.05, 0.05, (n, 3))
        p[0] = (1.0, 1.0, 1.0)
        return norm(p)
    p = rng.uniform(-1, 1, (n, 3))   # "sparse": most balls hold their centre only
    return norm(np.sign(p) * np.abs(p) ** 0.2)


@pytest.mark.parametrize("n_pts", [64, 100])
def test_degenerate_objects(vocab, n_pts):
    from text2pos_amd import synthetic as S
    rng = np.random.default_rng(n_pts)
    xyz, rgb, center, mean_rgb, cell_ptr = (a.copy() for a in S.make_cells(41, 5, n_pts=n_pts))
    kinds = ["few", "line", "dense", "sparse"]
    for o in range(xyz.shape[0]):
        xyz[o] = _odd_object(rng, kinds[o % 4], n_pts)
    for precision in ("f16x3", "fp32"):
        om, hm = _pair(vocab, n_pts, precision)
        _stagewise(om, hm, (xyz, rgb, center, mean_rgb, cell_ptr), f"degenerate {n_pts} {precision}")


@pytest.fixture(scope="module")
def model128(vocab):
    return _pair(vocab, 128)


def test_invariance_at_128(model128):
    """Chunking, the second stream and the call size change the schedule only: the same bits."""
    from text2pos_amd import synthetic as S
    _, hm = model128
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(61, 300, n_pts=128)
    dargs = _to_dev(xyz, rgb, center, mean_rgb)
    with torch.no_grad():
        ref = hm.encode_objects_packed(*dargs, cell_ptr, streams=1)
        assert torch.equal(hm.encode_objects_packed(*dargs, cell_ptr, streams=2), ref)
        assert torch.equal(hm.encode_objects_packed(*dargs, cell_ptr, streams=1, chunk_objects=max(97, int(np.diff(cell_ptr).max()))), ref)
        parts = []
        for c0 in range(0, 300, 7):   # calls of a few dozen objects
            c1 = min(c0 + 7, 300)
            o0, o1 = int(cell_ptr[c0]), int(cell_ptr[c1])
            parts.append(hm.encode_objects_packed(*[t[o0:o1] for t in dargs], cell_ptr[c0:c1 + 1] - cell_ptr[c0], streams=1))
    assert torch.equal(torch.cat(parts), ref)


def test_scene_path_equals_host_path_at_128(model128):
    from text2pos_amd import data as D, pipeline as PL, synthetic as S
    from text2pos_amd.scene import DeviceScene
    _, hm = model128
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(63, 24)
    rng = np.random.default_rng(5)
    cells = []
    for c in range(24):
        lo, hi = int(cell_ptr[c]), int(cell_ptr[c + 1])
        objs = []
        for i in range(lo, hi):   # raw objects of 60 .. 300 points: FixedPoints(128) draws with and without replacement
            k = int(rng.integers(60, 300))
            objs.append(D.Object3d(i, i, (xyz[i][rng.integers(0, 256, k)] * 3 + center[i]).astype(np.float64),
                                   rgb[i][rng.integers(0, 256, k)].astype(np.float64), "box"))
        cells.append(D.Cell(c, "s", objs, 30.0, np.arange(6.0)))
    tf = PL.PerCellTransform(128, 3)
    with torch.no_grad():
        scene = hm.encode_scene_cells(DeviceScene(cells, _dev()), tf, cells_per_call=10)
        objs = [c.objects for c in cells]
        host = hm.encode_objects(objs, [D.batch_object_points(o, tf.for_cell(i)) for i, o in enumerate(objs)])
    assert torch.equal(scene.cpu(), host.cpu())


def test_encode_objects_entry_point_at_128(model128):
    """encode_objects(objects, object_points) with PyG-style per-cell batches (models/cell_retrieval.py:77-107) vs the oracle."""
    from text2pos_amd import data as D, synthetic as S
    om, hm = model128
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(65, 5, n_pts=128)
    objects, points = [], []
    for c in range(5):
        lo, hi = int(cell_ptr[c]), int(cell_ptr[c + 1])
        objects.append([D.Object3d(i, i, np.tile(center[i].astype(np.float64), (2, 1)),
                                   np.tile(mean_rgb[i].astype(np.float64), (2, 1)), "box") for i in range(lo, hi)])
        points.append(D.Batch(x=torch.from_numpy(rgb[lo:hi].reshape(-1, 3).copy()), pos=torch.from_numpy(xyz[lo:hi].reshape(-1, 3).copy()),
                              batch=torch.arange(hi - lo).repeat_interleave(128)))
    wtr = []
    want = om.encode_objects_packed(xyz, rgb, center, mean_rgb, cell_ptr, trace=wtr).numpy()
    with torch.no_grad():
        got = hm.encode_objects(objects, points)
        packed, gtr = hm.encode_objects_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, want_trace=LIGHT)
    assert torch.equal(got, packed)                  # (so the packed call's trace is that of encode_objects' result)
    _check_cells(om, got.cpu().numpy(), gtr, want, wtr, cell_ptr, "encode_objects at 128 points")


def test_superglue_objects_only_at_128(vocab):
    """SuperGlueMatch (the fine stage: objects-only encode, embed_dim 128) at 128 points per object vs oracle/fine.py."""
    import weights as W
    import text2pos_amd as t2p
    from oracle import fine as OF, model as OM
    from text2pos_amd import synthetic as S
    args = OM.default_args(embed_dim=128, num_layers=2, sinkhorn_iters=50, pointnet_numpoints=128)
    prod = t2p.SuperGlueMatch(vocab["classes"], vocab["colors"], vocab["words"], args).eval()
    W.fill_state_dict(prod, 14)
    sd = prod.state_dict()
    orc = OF.OracleSuperGlueMatch(vocab["classes"], vocab["colors"], vocab["words"], args).eval()
    orc.load_state_dict({k: sd[k] for k in orc.state_dict() if not k.startswith("superglue.")}, strict=False)
    orc.superglue.load_reference_state(sd)
    prod = prod.to(_dev())
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(707, 3, fixed_n=16, n_pts=128)
    flat = S.make_texts(808, 0, 18, n_hints=1)
    hints = [flat[0:6], flat[6:12], flat[12:18]]
    want = orc.forward_packed(xyz, rgb, center, mean_rgb, cell_ptr, hints)
    with torch.no_grad():
        got = prod.forward_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, hints)
    assert (got.P.cpu() - want["P"]).abs().max().item() < TOL
    assert torch.equal(got.matches0.cpu(), want["matches0"]) and torch.equal(got.matches1.cpu(), want["matches1"])
    assert (got.offsets.cpu() - want["offsets"]).abs().max().item() < TOL


def test_train_then_eval_at_128(vocab):
    """The user story: a model trained in train() mode at pointnet_numpoints = 128 is put in eval() and encodes cells - the same
    embeddings as the oracle loaded with its state_dict."""
    import weights as W
    import text2pos_amd as t2p
    from oracle import model as OM
    from text2pos_amd import data as D, synthetic as S, training as T
    args = S.default_args(pointnet_numpoints=128)
    model = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], args)
    W.fill_state_dict(model, 37)
    model = model.to(_dev())

    def batch(seed, n_cells):
        xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(seed, n_cells, n_pts=128)
        objects, points = [], []
        for c in range(n_cells):
            lo, hi = int(cell_ptr[c]), int(cell_ptr[c + 1])
            objects.append([D.Object3d(i, i, np.tile(center[i].astype(np.float64), (2, 1)),
                                       np.tile(mean_rgb[i].astype(np.float64), (2, 1)), "box") for i in range(lo, hi)])
            points.append(D.Batch(x=torch.from_numpy(rgb[lo:hi].reshape(-1, 3).copy()), pos=torch.from_numpy(xyz[lo:hi].reshape(-1, 3).copy()),
                                  batch=torch.arange(hi - lo).repeat_interleave(128)))
        return dict(texts=S.make_texts(seed, 0, n_cells, n_hints=2), objects=objects, object_points=points)

    loader = [batch(51, 6), batch(52, 5)]
    crit = T.make_criterion(S.default_args(margin=0.35, ranking_loss="pairwise"))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    first, _ = T.train_epoch(model, loader, opt, crit)
    last, _ = T.train_epoch(model, loader, opt, crit)
    assert np.isfinite(first) and np.isfinite(last)
    model.eval()
    om = OM.OracleCellRetrieval(vocab["classes"], vocab["colors"], vocab["words"], OM.default_args(pointnet_numpoints=128)).eval()
    om.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, strict=True)
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(53, 6, n_pts=128)
    wtr = []
    want = om.encode_objects_packed(xyz, rgb, center, mean_rgb, cell_ptr, trace=wtr).numpy()
    with torch.no_grad():
        got, gtr = model.encode_objects_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, want_trace=LIGHT)
    _check_cells(om, got.cpu().numpy(), gtr, want, wtr, cell_ptr, "trained at 128 points")


@pytest.mark.parametrize("row", ["sa1 output", "sa2 output", "sa3 output", "sa1 hidden", "sa2 hidden", "sa3 hidden", "ga hidden"])
def test_guard_at_128(vocab, model128, row):
    """tests/guard_rescale.py's exact rescalings of the SA levels and GA layer 1 at 128 points: at s = 2^20 the stage's bit fires,
    at s = 2^-20 the low side (bit 7) does, at s = 1 the guard is silent; fp32 stays within the bar throughout."""
    import text2pos_amd as t2p
    import guard_rescale as GR
    from text2pos_amd import packing, synthetic as S
    om, _ = model128
    cells = S.make_cells(91, 6, n_pts=128)
    xyz, rgb, center, mean_rgb, cell_ptr = cells
    wtr = []
    want = om.encode_objects_packed(*cells, trace=wtr).numpy()
    exact = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(pointnet_numpoints=128),
                                     precision="fp32").to(_dev()).eval()
    x3 = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(pointnet_numpoints=128)).to(_dev()).eval()
    sd0 = om.state_dict()
    r = GR.ROWS[row]
    for k in (0, 20, -20):
        sd, rgb_s = GR.apply(sd0, rgb, row, 2.0 ** k)
        args = _to_dev(xyz, rgb_s, center, mean_rgb)
        exact.load_state_dict(sd, strict=True)
        x3.load_state_dict(sd, strict=True)
        with torch.no_grad():
            ex, etr = exact.encode_objects_packed(*args, cell_ptr, want_trace=LIGHT)
        _check_cells(om, ex.cpu().numpy(), etr, want, wtr, cell_ptr, f"{row} fp32 s=2^{k}")
        try:
            with torch.no_grad():
                got, gtr = x3.encode_objects_packed(*args, cell_ptr, want_trace=LIGHT)
            code = 0
        except packing.Fp16RangeError:   # a folded weight itself left fp16's range: refused before any launch
            assert k != 0, f"{row}: refused at s = 1"
            continue
        except FloatingPointError as e:
            code = int(re.search(r"guard code (0x[0-9a-f]+)", str(e)).group(1), 16)
        if k == 0:
            assert code == 0, f"{row}: guard fired at s = 1 ({code:#x})"
            _check_cells(om, got.cpu().numpy(), gtr, want, wtr, cell_ptr, f"{row} f16x3 s=1")
        elif k > 0:
            assert code & r.bit, f"{row} s=2^{k}: code {code:#x} lacks {r.bit:#x}"
        else:
            assert code & 0x80, f"{row} s=2^{k}: code {code:#x} lacks the low-side bit 0x80"


@pytest.mark.parametrize("n_pts", [7, 257, 512])
def test_refused_sizes(vocab, n_pts):
    """Outside 8 .. 256 points the library refuses before it launches anything, with a message that names the range."""
    import text2pos_amd as t2p
    from text2pos_amd import _lib as L, ops, synthetic as S
    hm = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(pointnet_numpoints=n_pts))
    hm = hm.to(_dev()).eval()
    xyz = torch.zeros((3, n_pts, 3), device=_dev())
    center = torch.zeros((3, 3), device=_dev())
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        with pytest.raises(L.T2PError, match=r"8 <= n_pts <= 256"), torch.no_grad():
            hm.encode_objects_packed(xyz, torch.zeros_like(xyz), center, center.clone(), np.array([0, 3], np.int32))
    finally:
        ops.profile_enable(False)
    assert ops.profile_report() == {}


def test_generic_kernel_only_at_other_sizes(vocab):
    """At 256 points the specialised f16x3 SA kernels run exactly as before; at 128 the generic one takes all three levels, at 255
    the first level only (levels 2 and 3 then have the 256-point shapes)."""
    from text2pos_amd import ops, synthetic as S
    names = {}
    for n_pts in (256, 255, 128):
        _, hm = _pair(vocab, n_pts)
        cells = _to_dev(*S.make_cells(5, 20, n_pts=n_pts)[:4])
        cell_ptr = S.make_cells(5, 20, n_pts=n_pts)[4]
        with torch.no_grad():
            hm.encode_objects_packed(*cells, cell_ptr)
        torch.cuda.synchronize()
        ops.profile_report()
        ops.profile_enable(True)
        try:
            with torch.no_grad():
                hm.encode_objects_packed(*cells, cell_ptr)
        finally:
            ops.profile_enable(False)
        names[n_pts] = set(ops.profile_report())
    assert not any(k.startswith("sa_x3") for k in names[256])
    assert {"ws_edge_sa_k32_n64", "ws_edge_sa_k128_n128", "ws_edge_sa_k256_n256"} <= names[256]
    assert {"sa_x3_k32_n64", "sa_x3_k128_n128", "sa_x3_k256_n256"} <= names[128]
    assert {"sa_x3_k32_n64", "ws_edge_sa_k128_n128", "ws_edge_sa_k256_n256"} <= names[255]
    assert not {"sa_x3_k128_n128", "sa_x3_k256_n256"} & names[255]
