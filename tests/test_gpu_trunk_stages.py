"""The cell encoder's trunk held to float64, STAGE BY STAGE: grouping, SA levels 1-3 (k_sa_points / k_sa_rows / k_sa3 /
k_sa_stream behind the k_ws DENSE_STORE tables), GA (GA1 store + k_ga2), lin1, lin2 and the object head, each on the kernel's own
traced upstream output (t2p_cell_trace through encode_objects_packed(want_trace=...)), against tests/trunk_ref.py:
  grouping  fps_idx / nbr / cnt bit-equal to oracle/primitives.c; the [xyz 0] tail of every sa_out row bit-equal to the gathered
            centroid, column C + 3 and the pad columns 0;
  (A)       |kernel - ref64| <= 2 x bound for every element of every stage (bounds derived in trunk_ref.py, proved on the CPU
            by tests/test_trunk_ref_host.py);
  (B)       max|kernel - ref64| <= R max(max|emul - ref64|, u max|ref64|) for SA1-3, GA, lin1, lin2 and the object head - the
            assertion that sees a lost fp16 plane, a mis-scaled drain or a dropped row, and names the stage (R and its margins: the
            host test).  The emulation runs in 16-k tiles, the order of the MFMA steps; R covers the other orders by construction;
  guard     the f16x3 guard word stays 0 in every case, the rescaled ones included (they stay inside the silent band).
Cases: trunk_ref.CASES - 40 objects (ordinary synthetic ones next to fuzz_cells' "few", "dense" and "sparse") in cells of
1, 2, 5, 9 and 23; both precisions, both self_loops values, the full-trace plan (list-mode scan) and the default plan (hit masks,
pruned lists), tuning 0xD and bits 0, 2, 3, n_pts 256 / 100 / 64 / 8, pointnet_features 0 / 1 / 2, chunk_objects 8, a second weight
fill, guard_rescale at 2^4 and 2^-3 on three stages, and the 40 objects as ONE cell, whose features t2p_pointnet2_forward must return
bit for bit.  Stage references are cached by the bits of the stage's inputs: cases that differ only in their execution plan hand
the same bits to a stage and share them.

  (C)       exact inputs (trunk_ref.exact_objects / exact_weights: points on the 2^-4 grid, colours on the 2^-8 grid, two taps of
            +-1/2 or +-1/4 per output column, BatchNorms already folded): every stage from the points to features2 returns fp32(ref64)
            BIT FOR BIT in f16x3 and in fp32, with and without self loops - gather, aliasing, max, bias, ReLU, drain, tails, hi.hi and
            lo.hi; channel 0 carries a value that only a split to nearest keeps exact.  One two-plane set per MFMA stage (SA1, SA2,
            SA3, GA layer 2: w = r + t 2^-13 behind single-plane activations) does the same up to its stage, for hi.lo.  The host
            test proves these inputs exact under every summation order, and that an emulation without lo.hi, without hi.lo or with a
            truncating split does not return their bits.
obj_emb has no exact form (F.normalize rounds): (C) ends at features2.

Every check prints `TRUNK | case | stage | err / bound | max err / (B) threshold` before it asserts (pytest -s; docs/notebook.md,
"The trunk held to float64 bounds, stage by stage", records a run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunk_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
_REFS = {}
TRACE_NO_TABLES = ("fps_idx", "sa_out", "features0", "features1", "features2", "obj_emb")


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _numpy_pack(p):
    out = {}
    for k, v in p.items():
        if isinstance(v, (list, tuple)):
            out[k] = [_np(t) if torch.is_tensor(t) else t for t in v]
        else:
            out[k] = _np(v) if torch.is_tensor(v) else v
    return out


@functools.lru_cache(maxsize=None)
def _model(seed, features, rescale, precision):
    """The product model with a deterministic fill (tests/golden/weights.py), optionally rescaled by tests/guard_rescale.py."""
    import guard_rescale as GR
    import weights as W
    import text2pos_amd as t2p
    from oracle import model as OM
    from text2pos_amd import synthetic as S
    classes, colors, words = S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words()
    om = OM.OracleCellRetrieval(classes, colors, words, OM.default_args(pointnet_features=features)).eval()
    W.fill_state_dict(om, seed)
    sd = om.state_dict()
    if rescale is not None:
        sd, _ = GR.apply(sd, None, rescale[0], rescale[1])
    hm = t2p.CellRetrievalNetwork(classes, colors, words, S.default_args(pointnet_features=features), precision=precision)
    hm.load_state_dict(sd, strict=True)
    return hm.to(_dev()).eval()


@functools.lru_cache(maxsize=None)
def _objects(n_pts, one_cell):
    return T.case_objects(n_pts, one_cell)


@functools.lru_cache(maxsize=None)
def _groups(n_pts):
    return T.oracle_groups(_objects(n_pts, False)[0])


def _run(case):
    """One call with the trace; returns (trace as NumPy, the folded pack as NumPy, inputs)."""
    hm = _model(case["seed"], case["features"], case["rescale"], case["precision"])
    xyz, rgb, center, mean_rgb, cell_ptr = _objects(case["n_pts"], case["one_cell"])
    hm.add_self_loops, hm.tuning = case["self_loops"], case["tuning"]
    try:
        with torch.no_grad():
            _, tr = hm.encode_objects_packed(*[torch.from_numpy(a).to(_dev()) for a in (xyz, rgb, center, mean_rgb)], cell_ptr,
                                             want_trace=True if case["full_trace"] else TRACE_NO_TABLES,
                                             chunk_objects=case["chunk"], check_overflow=False, streams=1)
        torch.cuda.synchronize()
        guard = hm.overflow_detected() if case["precision"] == "f16x3" else 0
    finally:
        hm.add_self_loops, hm.tuning = True, 0
    trace = {k: ([_np(t) for t in v] if isinstance(v, list) else _np(v)) for k, v in tr.items()}
    # (hm._pack[1] is the model's cached dict of folded tensors - a private name, like packing._pack_cell_weights_fp32 and
    # packing._add_x3_images below: these tests read exactly what the library was handed, and move with a refactor of those)
    return trace, _numpy_pack(hm._pack[1]), guard, hm


def _cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _report(case, stage, got, ref, bound, emul):
    """Prints, then asserts (A) and - with an emulation - (B); an exact case: bit equality with fp32(ref64)."""
    precision = case["precision"]
    if case.get("exact"):
        same = T.G.bits_equal(got, np.asarray(ref, np.float64).astype(F32))
        print("TRUNK | %s | %s | %s | -" % (case["name"], stage, "bit-equal" if same else "max err %.3g" % T.max_err(got, ref)))
        assert same, "%s %s: not the exact result bit for bit (max error %.3g)" % (case["name"], stage, T.max_err(got, ref))
        return
    ratio = T.worst_ratio(got, ref, bound)
    if emul is None:
        print("TRUNK | %s | %s | %.3g | -" % (case["name"], stage, ratio))
    else:
        thr = T.sharp_threshold(emul, ref, precision, stage)
        sharp = T.max_err(got, ref) / thr
        print("TRUNK | %s | %s | %.3g | %.3g" % (case["name"], stage, ratio, sharp))
    assert T.within(got, ref, bound, T.FACTOR_GPU), "%s %s: (A) an element at %.3g x bound" % (case["name"], stage, ratio)
    if emul is not None:
        assert sharp <= 1.0, "%s %s: (B) max error %.3g = %.3g x R max(emulation's %.3g, u max|ref|)" % (
            case["name"], stage, T.max_err(got, ref), sharp, T.max_err(emul, ref))


def check_trace(case, trace, p, inputs):
    """Every stage of one call against trunk_ref, each on the traced output of the stage before."""
    xyz, rgb, center, mean_rgb, cell_ptr = inputs
    precision, n_pts, n = case["precision"], case["n_pts"], xyz.shape[0]
    x3 = precision == "f16x3"
    geo = T.level_geometry(n_pts)
    g = T.oracle_groups(xyz) if case.get("exact") else _groups(n_pts)
    exact = bool(case.get("exact"))
    # ---- grouping: bit for bit ----
    for l in range(3):
        assert np.array_equal(trace["fps_idx"][l].astype(np.int32), g["fps_idx"][l]), (case["name"], "fps_idx", l)
        if case["full_trace"]:
            assert np.array_equal(trace["cnt"][l].astype(np.int32), g["cnt"][l]), (case["name"], "cnt", l)
            assert np.array_equal(trace["nbr"][l].astype(np.int32), g["nbr"][l]), (case["name"], "nbr", l)
    feat, pos = rgb.reshape(-1, 3), xyz.reshape(-1, 3)
    for l, (nd, nc) in enumerate(geo):
        stage, c = "sa%d" % (l + 1), T.C[l]
        so = trace["sa_out"][l]
        assert so.shape == (n * nc, T.LD[l])
        idx = trace["fps_idx"][l].astype(np.int64)
        want_tail = np.take_along_axis(pos.reshape(n, nd, 3), idx[:, :, None], axis=1).reshape(-1, 3)
        assert T.G.bits_equal(so[:, c: c + 3], want_tail), (case["name"], stage, "centroid xyz of the row tail")
        assert not so[:, c + 3:].view(np.int32).any(), (case["name"], stage, "column C + 3 and the pad columns must hold +0")
        tables = trace if case["full_trace"] else g
        src, dst = T.edge_rows(tables["nbr"][l], tables["cnt"][l], cell_ptr, nd, nc, case["self_loops"])
        cin = feat.shape[1]
        args = (feat, pos, so[:, c: c + 3], src, dst, p["sa_w1"][l][: cin + 3], p["sa_b1"][l], p["sa_w2"][l], p["sa_b2"][l])
        scale = float(p["sa_w2_scale"][l]) if x3 else 1.0
        pk = x3 and l == 0 and T.specialised(n_pts)
        key = T.digest(*args)
        ref = _cached(("ref", key), lambda: T.sa_ref64(*args))
        bound = None if exact else _cached(("bound", key, precision, scale, pk), lambda: T.sa_bound(ref, *args, precision, scale, pk))
        emul = None if exact else _cached(("emul", key, precision, scale, pk), lambda: T.sa_emul(*args, precision, scale, pk, "tile"))
        _report(case, stage, so[:, :c], ref["out"], bound, emul)
        if case.get("stop_after") == stage:
            return
        feat, pos = so[:, :c], so[:, c: c + 3]
    # ---- GA ----
    args = (feat, pos, n, p["ga_w1"][:259], p["ga_b1"], p["ga_w2"], p["ga_b2"])
    key = T.digest(*args[:2], *args[3:])
    ref = _cached(("ref", key), lambda: T.ga_ref64(*args))
    bound = None if exact else _cached(("bound", key, precision), lambda: T.ga_bound(ref, *args, precision))
    emul = None if exact else _cached(("emul", key, precision), lambda: T.ga_emul(*args, precision, "tile"))
    _report(case, "ga", trace["features0"], ref["out"], bound, emul)
    if case.get("stop_after") == "ga":
        return
    # ---- lin1, lin2 ----
    for name, a, got in (("lin1", trace["features0"], trace["features1"]), ("lin2", trace["features1"], trace["features2"])):
        w, b = p[name + "_w"], p[name + "_b"]
        scale = float(p[name + "_scale"]) if x3 else 1.0
        key = T.digest(a, w, b)
        ref = _cached(("ref", key), lambda: T.dense_ref64(a, w, b))
        bound = None if exact else _cached(("bound", key, precision, scale), lambda: T.dense_bound(ref, a, w, b, precision, scale))
        emul = None if exact else _cached(("emul", key, precision, scale), lambda: T.dense_emul(a, w, b, precision, scale, "tile"))
        _report(case, name, got, ref, bound, emul)
    if exact:      # F.normalize rounds: the object head has no exact form
        return
    # ---- object head: (A) ----
    f = trace["features%d" % case["features"]]
    key = T.digest(f, center, mean_rgb, p["pn_w"], p["merge_w"], p["col_w2"], p["pos_w2"])
    pieces = _cached(("ref", key), lambda: T.object_head_ref64(f, center, mean_rgb, p))
    bound = _cached(("bound", key, precision), lambda: T.object_head_bound(pieces, f, center, mean_rgb, p, precision))
    emul = _cached(("emul", key, precision), lambda: T.object_head_emul(f, center, mean_rgb, p, precision, "tile"))
    _report(case, "head", trace["obj_emb"], pieces["out"], bound, emul)


@pytest.mark.parametrize("case", T.CASES, ids=[c["name"] for c in T.CASES])
def test_trunk_stage_by_stage(case):
    trace, p, guard, hm = _run(case)
    assert guard == 0, "%s: guard word %#x (the case must stay inside the silent band)" % (case["name"], guard)
    inputs = _objects(case["n_pts"], case["one_cell"])
    check_trace(case, trace, p, inputs)
    if case["one_cell"]:
        # t2p_pointnet2_forward: the same 40 objects as one batch, the trunk alone - the trace's features bit for bit
        from text2pos_amd import ops
        xyz, rgb = (torch.from_numpy(a).to(_dev()) for a in inputs[:2])
        hm.add_self_loops, hm.tuning = case["self_loops"], case["tuning"]
        try:
            out = ops.pointnet2_forward(xyz, rgb, hm._cell_pack(), hm._cell_config(case["n_pts"]))
            torch.cuda.synchronize()
        finally:
            hm.add_self_loops, hm.tuning = True, 0
        for name in ("features0", "features1", "features2"):
            assert T.G.bits_equal(_np(out[name]), trace[name]), (case["name"], "t2p_pointnet2_forward", name)
        assert (hm.overflow_detected() if case["precision"] == "f16x3" else 0) == 0


# ---- (C) exact inputs: points to features2 without a rounding, both precisions must return the same bits ------------------------------

@pytest.mark.parametrize("which", [(None, True), (None, False)] + [(st, True) for st in T.TWO_PLANE_STAGES],
                         ids=["loops", "noloops"] + ["two-plane-" + st for st in T.TWO_PLANE_STAGES])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_exact_inputs_bit_for_bit(precision, which):
    """trunk_ref.exact_objects / exact_weights: every stage from the points to features2 must return fp32(ref64) bit for bit, in
    f16x3 and in fp32 - the gather, PyG's aliasing, the max, bias, ReLU, the drain's 1 / s, the row tails, hi.hi and lo.hi (the
    weights are single-plane: hi.lo is zero) and, through the probe channel 0, the split to nearest.  The two-plane set of a stage
    (SA1, SA2, SA3, GA layer 2): single-plane activations in front of w = r + t 2^-13, checked up to that stage - hi.lo.  The
    designed matrices go to the library as they are: the pack is assembled here, not folded from a state dict.  Guard word 0."""
    from text2pos_amd import ops, packing
    two_plane, self_loops = which
    hm = _model(11, 2, None, precision)
    dev = _dev()
    designed = T.exact_weights(two_plane=two_plane)
    p = packing._pack_cell_weights_fp32(hm, dev)
    for k, v in designed.items():
        p[k] = [torch.from_numpy(t).to(dev) for t in v] if isinstance(v, list) else torch.from_numpy(v).to(dev)
    if precision == "f16x3":
        packing._add_x3_images(p, dev, True)
        images = dict(sa1=p["sa_w2_x3"][0], sa2=p["sa_w2_x3"][1], sa3=p["sa_w2_x3"][2], ga=p["ga_w2_x3"], ga1=p["ga_w1_x3"],
                      lin1=p["lin1_x3"], lin2=p["lin2_x3"])
        for name, img in images.items():
            assert bool(_np(img[1]).any()) == (name == two_plane), "the lo plane of an image is zero unless it is the two-plane stage's"
    pn = _numpy_pack(p)
    for k, v in designed.items():
        for got, want in zip(pn[k] if isinstance(v, list) else [pn[k]], v if isinstance(v, list) else [v]):
            assert T.G.bits_equal(got, want), ("the matrices handed to the library are the designed ones", k)
    inputs = T.exact_objects(two_plane)
    xyz, rgb, center, mean_rgb, cell_ptr = inputs
    hm.add_self_loops, hm.tuning = self_loops, 0
    try:
        cfg = hm._cell_config(256)
        with torch.no_grad():
            _, tr = ops.encode_cells(*[torch.from_numpy(a).to(dev) for a in (xyz, rgb, center, mean_rgb)], cell_ptr,
                                     torch.from_numpy(cell_ptr).to(dev), ops.make_cell_weights(p), cfg, True, ws_tag="trunk_exact")
        torch.cuda.synchronize()
        guard = hm.overflow_detected() if precision == "f16x3" else 0
    finally:
        hm.add_self_loops = True
    assert guard == 0, "guard word %#x" % guard
    trace = {k: ([_np(t) for t in v] if isinstance(v, list) else _np(v)) for k, v in tr.items()}
    case = dict(T.CASES[0], name="exact-%s-%s" % (precision, two_plane or ("loops" if self_loops else "noloops")), precision=precision,
                self_loops=self_loops, exact=True, stop_after=two_plane)
    check_trace(case, trace, pn, inputs)
    if two_plane is None:
        assert (trace["features2"][:, 0] == F32(T.EXACT_PROBE)).all() and (trace["features2"] == 0).any()


# ---- t2p_knn beyond its one test (tests/test_gpu_parity.py::test_knn_bit_exact: dim 256, k 8, segments up to 40 rows) -------------------

def _oracle_knn(x, ptr, k):
    import ctypes as C
    from oracle import lib
    want = np.zeros((x.shape[0], k), np.int32)
    fp = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    lib().t2p_oracle_knn(fp(x, C.c_float), fp(ptr, C.c_int32), C.c_int32(len(ptr) - 1), C.c_int32(x.shape[1]), C.c_int32(k),
                         fp(want, C.c_int32))
    return want


def _knn_rows(sizes, dim, seed):
    rng = np.random.default_rng([seed, dim, len(sizes)])
    ptr = np.zeros(len(sizes) + 1, np.int32)
    ptr[1:] = np.cumsum(sizes)
    x = rng.standard_normal((int(ptr[-1]), dim)).astype(F32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    for s in range(len(sizes)):                      # duplicate rows: distance ties inside every segment of 3 rows and more
        if sizes[s] >= 3:
            x[ptr[s] + sizes[s] // 2] = x[ptr[s]]
            x[ptr[s + 1] - 1] = x[ptr[s] + 1]
    return np.ascontiguousarray(x), ptr


# launch_knn stages the rows of segments of <= 64 rows in LDS while the largest segment's distance matrix leaves room for them (and
# dim is a multiple of 4): "mixed" (largest 100) has staged and unstaged segments side by side, a 192-row segment leaves no room
KNN_SIZES = {"mixed": [1, 63, 64, 65, 100, 2, 9], "with192": [1, 63, 64, 65, 100, 192], "unstaged": [192, 192, 150]}


@pytest.mark.parametrize("dim", [256, 64, 128, 512, 10])
@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("sizes", sorted(KNN_SIZES))
def test_knn_segments_dims_and_k(sizes, k, dim):
    """Bit-exact against t2p_oracle_knn: staged and unstaged segments side by side (1 .. 192 rows, max_seg_rows above the staging
    limit), a launch without any staged segment, k = 1 / 8 / 32 and k larger than a segment (-1 past its size), dims that are
    and (10) are not a multiple of 4, duplicate rows in every segment."""
    from text2pos_amd import ops
    x, ptr = _knn_rows(KNN_SIZES[sizes], dim, 5)
    got = ops.knn(torch.from_numpy(x).to(_dev()), torch.from_numpy(ptr).to(_dev()), k)
    assert np.array_equal(_np(got), _oracle_knn(x, ptr, k))


def test_knn_max_seg_rows_limit():
    """max_seg_rows = 192 is served, 193 is T2P_E_ARG (through ops: a RuntimeError naming t2p_knn)."""
    from text2pos_amd import ops
    x, ptr = _knn_rows([192, 5], 64, 6)
    xd, pd = torch.from_numpy(x).to(_dev()), torch.from_numpy(ptr).to(_dev())
    assert np.array_equal(_np(ops.knn(xd, pd, 8, max_seg_rows=192)), _oracle_knn(x, ptr, 8))
    with pytest.raises(RuntimeError, match="t2p_knn"):
        ops.knn(xd, pd, 8, max_seg_rows=193)
