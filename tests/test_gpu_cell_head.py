"""The cell head held to float64, STAGE BY STAGE: everything behind obj_emb (Chunk::cell_head of csrc/cell_encoder.hip: k_rownorm,
the split products P and Q, k_knn, the WS_EDGE_KNN stream of csrc/ws_gemm.hip, k_segpool, the two lin GEMMs, the final k_rownorm),
each on the kernel's own traced upstream output (t2p_cell_trace.head_in / head_edge / head_pool / head_l1 / head_l2), against
tests/cell_head_ref.py:
  in, out   (A) against F.normalize in float64;
  knn       knn_idx bit-equal to oracle/primitives.c's kNN on the traced head_in, and inside each object's cell - every object of
            every cell, no near-tie allowance: the table is a pure function of head_in's bits;
  edge      (A) |kernel - ref64| <= 2 x bound on every element and (B) max|kernel - ref64| <= R max(max|emul - ref64|, u max|ref64|)
            on the traced graph, max and mean aggregation; pool (A) - the max pool has bound 0: bit equality; l1, l2 (A) and (B);
  guard     the f16x3 guard word stays 0; traced and untraced calls return the same `out` bits.
R = cell_head_ref.R_SHARP, derived on the CPU by tests/test_cell_head_ref_host.py, which also shows that every wrong emulation of a
stage's list lands above (B) on these very cases.  Nothing is skipped or excused: every object, cell and case is asserted.

Cases (cell_head_ref): the full path (40 objects through trunk, object head and cell head, cells of 1, 2, 5, 9, 23, chunk_objects
8: three chunks write their own cell rows; both precisions, both aggregations, a second weight fill); the embedding path
(class_embed only: obj_emb is a normalised table row, no trunk) at D = 256, 128, 64 and 300 with cells of 1 .. 192 objects that
straddle the 8-destination groups, the D = 300 case with and without the 192-object cell that switches k_knn's LDS staging off; one
call of 32 x multi_processor_count + 40 objects, whose knn_group is 32; the exact family, bit for bit; refusals and NaN.

Every check prints `HEAD | case | stage | err / bound | max err / (B) threshold` before it asserts (pytest -s; docs/notebook.md,
"The cell head held to float64 bounds", records a run)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cell_head_ref as H  # noqa: E402
import trunk_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
G = T.G
TRACE = ("obj_emb", "knn_idx") + H.HEAD_TRACE
_REFS = {}


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _numpy_pack(p):
    return {k: (_np(v) if torch.is_tensor(v) else v) for k, v in p.items() if not isinstance(v, (list, tuple))}


@functools.lru_cache(maxsize=None)
def _model(d, variation, precision, seed, embed):
    """The product model with a deterministic fill (tests/golden/weights.py); embed: the single-feature class_embed model."""
    import weights as W
    import text2pos_amd as t2p
    from oracle import model as OM
    from text2pos_amd import synthetic as S
    kw = dict(embed_dim=d, variation=variation)
    if embed:
        kw.update(use_features=["class"], class_embed=True)
    classes, colors, words = S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words()
    om = OM.OracleCellRetrieval(classes, colors, words, OM.default_args(**kw)).eval()
    W.fill_state_dict(om, seed)
    hm = t2p.CellRetrievalNetwork(classes, colors, words, S.default_args(**kw), precision=precision)
    hm.load_state_dict(om.state_dict(), strict=True)
    return hm.to(_dev()).eval()


def _cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _report(name, stage, precision, got, ref, bound, emul=None, rows=None):
    """Prints, then asserts (A) on every element and - with an emulation (of `rows`, or of everything) - (B)."""
    ratio = T.worst_ratio(got, ref, bound)
    sharp = None
    if emul is not None:
        g, r = (got, ref) if rows is None else (got[rows], ref[rows])
        sharp = T.max_err(g, r) / H.sharp_threshold(emul, r, precision, stage)
    print("HEAD | %s | %s | %.3g | %s" % (name, stage, ratio, "-" if sharp is None else "%.3g" % sharp))
    assert T.within(got, ref, bound, H.FACTOR_GPU), "%s %s: (A) an element at %.3g x bound" % (name, stage, ratio)
    if sharp is not None:
        assert sharp <= 1.0, "%s %s: (B) max error at %.3g x R max(emulation's, u max|ref|)" % (name, stage, sharp)


def check_head(case, out, trace, p, cp, num_cus, dsts=None):
    """Every stage of one call against cell_head_ref, each on the traced output of the stage before.  dsts: the destinations whose
    edge rows the ordered emulation covers ((B); None = all)."""
    name, precision, mean, chunk = case["name"], case["precision"], case["variation"] == 1, case.get("chunk", 0)
    d, dk = case["d"], H.kernel_dim(case["d"])
    n, nb = int(cp[-1]), len(cp) - 1
    shapes = dict(obj_emb=(n, dk), knn_idx=(n, H.KNN_K), head_in=(n, dk), head_edge=(n, dk), head_pool=(nb, dk), head_l1=(nb, dk),
                  head_l2=(nb, dk))
    for k, shp in shapes.items():
        assert trace[k].shape == shp, (name, k, trace[k].shape)
        if k != "knn_idx" and dk != d:
            assert not trace[k][:, d:].view(np.int32).any(), (name, k, "the pad columns hold +0")
    assert out.shape == (nb, dk) and not out[:, d:].view(np.int32).any()
    # ---- in ----
    emb, xn = trace["obj_emb"], trace["head_in"]
    _report(name, "in", precision, xn, H.norm_ref64(emb), H.norm_bound(emb))
    # ---- knn: bit for bit, every object ----
    knn = H.global_rows(trace["knn_idx"], cp, chunk)
    cell_of = np.repeat(np.arange(nb), np.diff(cp))
    assert ((knn < 0) | (cell_of[np.maximum(knn, 0)] == cell_of[:, None])).all(), (name, "a neighbour outside its object's cell")
    want = _cached(("knn", T.digest(xn, cp)), lambda: H.knn_oracle(xn, cp))
    differ = np.flatnonzero((knn != want).any(1))
    print("HEAD | %s | knn | %d of %d objects differ | -" % (name, len(differ), n))
    assert len(differ) == 0, "%s: knn_idx of objects %s is not oracle/primitives.c's on the traced head_in" % (name, differ[:8].tolist())
    # ---- edge ----
    key = T.digest(xn, knn, p["g_wp"], p["g_bp"], p["g_wq"], p["g_w2"], p["g_b2"]) + str(mean)
    ref = _cached(("edge", key), lambda: H.edge_ref64(xn, knn, p, mean))
    bound = _cached(("edge-bound", key, precision), lambda: H.edge_bound(ref, xn, p, precision, mean))
    emul = _cached(("edge-emul", key, precision, None if dsts is None else T.digest(dsts)),
                   lambda: H.edge_emul(xn, knn, p, precision, mean, "tile", None, dsts))
    _report(name, "edge", precision, trace["head_edge"], ref["out"], bound, emul, dsts)
    # ---- pool ----
    pr = H.pool_ref64(trace["head_edge"], cp, mean)
    _report(name, "pool", precision, trace["head_pool"], pr, H.pool_bound(pr, trace["head_edge"], cp, mean))
    # ---- l1, l2: launch_gemm, fp32 on both precisions ----
    for st, a, got in (("l1", trace["head_pool"], trace["head_l1"]), ("l2", trace["head_l1"], trace["head_l2"])):
        w, b = p["lin_w" + st[1]], p["lin_b" + st[1]]
        lkey = T.digest(a, w, b)
        lr = _cached(("lin", lkey), lambda: H.lin_ref64(a, w, b))
        _report(name, st, precision, got, lr, _cached(("lin-bound", lkey), lambda: H.lin_bound(lr, a, w, b)),
                _cached(("lin-emul", lkey), lambda: H.lin_emul(a, w, b, "tile")))
    # ---- out ----
    _report(name, "out", precision, out, H.norm_ref64(trace["head_l2"]), H.norm_bound(trace["head_l2"]))
    # ---- the case reaches what it is there for ----
    return H.branches_reached(dict(case, sizes=tuple(np.diff(cp).tolist())), num_cus)


# ---- the embedding path: ops.encode_cells with a table row per object -----------------------------------------------------------------

def _embed_pack(hm, table=None, designed=None):
    """The model's folded pack with the class table (and, exact family, the head's matrices) replaced; f16x3 images rebuilt."""
    from text2pos_amd import packing
    dev = _dev()
    p = packing._pack_cell_weights_fp32(hm, dev)
    if hm.kernel_dim != hm.embed_dim:
        packing._pad_cell_pack(p, hm.embed_dim, hm.kernel_dim, True)
    if designed is not None:
        for k, v in designed.items():
            if isinstance(v, np.ndarray):
                p[k] = torch.from_numpy(v).to(dev)
    if table is not None:
        p["class_embedding"] = torch.from_numpy(np.ascontiguousarray(table, F32)).to(dev)
    if hm.precision == "f16x3":
        packing._add_x3_images(p, dev, True)
    return p


def _embed_call(hm, p, idx, cp, variation, chunk=0, want_trace=TRACE):
    """One ops.encode_cells call of the single-feature embedding path (no trunk: 8 dummy points per object).  Returns
    (out, trace, guard word) as NumPy."""
    from text2pos_amd import ops
    dev = _dev()
    n = len(idx)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if hm.precision == "f16x3" else None
    cfg = ops.make_cell_config(n_pts=8, embed_dim=hm.kernel_dim, use_features=("class",), variation=variation, chunk_objects=chunk,
                               precision=hm.precision, class_idx=torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev),
                               overflow_flag=flag)
    pts = torch.zeros((n, 8, 3), dtype=torch.float32, device=dev)
    three = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    cp = np.ascontiguousarray(cp, np.int32)
    with torch.no_grad():
        res = ops.encode_cells(pts, pts, three, three, cp, torch.from_numpy(cp).to(dev), ops.make_cell_weights(p), cfg, want_trace,
                               ws_tag="cell_head_test")
    torch.cuda.synchronize()
    guard = int(flag.item()) if flag is not None else 0
    if not want_trace:
        return _np(res), None, guard
    return _np(res[0]), {k: _np(v) for k, v in res[1].items()}, guard


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _embed_result(name):
    """(out, cell_ptr) of an embedding-path case, after all of its checks."""
    case = next(c for c in H.EMBED_CASES if c["name"] == name)
    hm = _model(case["d"], case["variation"], case["precision"], case["seed"], True)
    # the table of the FULL size list, so that the staged D = 300 case reads the very rows of the one with the 192-object cell
    table, idx, cp_full = H.embed_table(case, H.EMBED_SIZES)
    cp = cp_full[: len(case["sizes"]) + 1]
    n = int(cp[-1])
    p = _embed_pack(hm, table)
    out, trace, guard = _embed_call(hm, p, idx[:n], cp, case["variation"], case["chunk"])
    assert guard == 0, "%s: guard word %#x" % (name, guard)
    reached = check_head(case, out, trace, H.head_pack(_numpy_pack(p)), cp, _num_cus())
    assert reached["group"] == {8} and reached["straddle"] and reached["ragged"] and reached["short_cell"], reached
    assert reached["knn"] == ({"unstaged"} if 192 in case["sizes"] and not case["chunk"] else {"staged", "unstaged"}), reached
    plain, _, guard = _embed_call(hm, p, idx[:n], cp, case["variation"], case["chunk"], want_trace=False)
    assert guard == 0 and G.bits_equal(plain, out), "%s: traced and untraced calls differ" % name
    return out, cp


@pytest.mark.parametrize("name", [c["name"] for c in H.EMBED_CASES])
def test_embedding_path_stage_by_stage(name):
    out, cp = _embed_result(name)
    if name.endswith("-staged"):
        # the same cells with k_knn's rows staged in LDS and read from global memory (the 192-object cell in the chunk): same bits
        other, _ = _embed_result(name[: -len("-staged")])
        assert G.bits_equal(out, other[: len(cp) - 1]), "%s: staging changes a cell's bits" % name
    if name.endswith("-chunk100"):
        other, _ = _embed_result(name[: -len("-chunk100")])
        assert G.bits_equal(out, other), "%s: the chunking changes a cell's bits" % name


def test_trimmed_trace_through_the_model():
    """CellRetrievalNetwork.encode_objects_packed cuts the pad columns off the head's stages as it does off obj_emb (D = 300 runs
    at 384): the trimmed stages are the untrimmed ones' first 300 columns."""
    hm = _model(300, 0, "f16x3", 11, True)
    dev = _dev()
    rows = hm.object_encoder.class_embedding.weight.shape[0]
    cp = np.array([0, 3, 12], np.int32)
    idx = (np.arange(12) * 5 % rows).astype(np.int32)
    pts, three = torch.zeros((12, 8, 3), device=dev), torch.zeros((12, 3), device=dev)
    with torch.no_grad():
        out, tr = hm.encode_objects_packed(pts, pts, three, three, cp, want_trace=TRACE, class_idx=torch.from_numpy(idx).to(dev),
                                           check_overflow=False, streams=1)
    assert hm.overflow_detected() == 0
    full_out, full, _ = _embed_call(hm, _embed_pack(hm), idx, cp, 0)
    assert tuple(out.shape) == (2, 300) and G.bits_equal(_np(out), full_out[:, :300])
    for k in ("obj_emb",) + H.HEAD_TRACE:
        assert tr[k].shape[1] == 300 and tr[k].is_contiguous() and G.bits_equal(_np(tr[k]), full[k][:, :300]), k


# ---- the full path -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", H.FULL_CASES, ids=[c["name"] for c in H.FULL_CASES])
def test_full_path_stage_by_stage(case):
    hm = _model(256, case["variation"], case["precision"], case["seed"], False)
    xyz, rgb, center, mean_rgb, cp = T.case_objects()
    dev_in = [torch.from_numpy(a).to(_dev()) for a in (xyz, rgb, center, mean_rgb)]
    with torch.no_grad():
        out, tr = hm.encode_objects_packed(*dev_in, cp, want_trace=TRACE, chunk_objects=case["chunk"], check_overflow=False, streams=1)
        torch.cuda.synchronize()
        guard = hm.overflow_detected() if case["precision"] == "f16x3" else 0
        plain = hm.encode_objects_packed(*dev_in, cp, chunk_objects=case["chunk"], check_overflow=False, streams=1)
        torch.cuda.synchronize()
        guard |= hm.overflow_detected() if case["precision"] == "f16x3" else 0
    assert guard == 0, "%s: guard word %#x" % (case["name"], guard)
    assert G.bits_equal(_np(plain), _np(out)), "%s: traced and untraced calls differ" % case["name"]
    reached = check_head(case, _np(out), {k: _np(v) for k, v in tr.items()}, H.head_pack(_numpy_pack(hm._pack[1])), cp, _num_cus())
    assert reached["chunks"] == 3 and reached["group"] == {8}


# ---- knn_group = 32 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", H.GROUP32_CASES, ids=[c["name"] for c in H.GROUP32_CASES])
def test_group_of_32_destinations(case):
    cus = _num_cus()
    sizes = H.group32_sizes(cus)
    case = dict(case, sizes=sizes)
    hm = _model(256, case["variation"], case["precision"], case["seed"], True)
    table, idx, cp = H.embed_table(case)
    p = _embed_pack(hm, table)
    out, trace, guard = _embed_call(hm, p, idx, cp, case["variation"])
    assert guard == 0
    dsts = H.sample_dsts(cp, 32, seed=1)          # (B) on the first, the last and four seeded groups; (A) on every element
    reached = check_head(case, out, trace, H.head_pack(_numpy_pack(p)), cp, cus, dsts)
    assert reached["group"] == {32} and reached["straddle"] and reached["ragged"], reached
    # the first 1,000 objects as a call of their own run in groups of 8: the same bits for their cells
    nb = int(np.searchsorted(cp, 1000, side="right")) - 1
    small, _, guard = _embed_call(hm, p, idx[: cp[nb]], cp[: nb + 1], case["variation"], want_trace=False)
    assert H.branches_reached(dict(case, sizes=sizes[:nb]), cus)["group"] == {8}
    assert guard == 0 and G.bits_equal(small, out[:nb]), "groups of 8 and of 32 destinations differ"


# ---- the exact family: bit for bit -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("case", H.EXACT_CASES, ids=[c["name"] for c in H.EXACT_CASES])
def test_exact_family_bit_for_bit(case, precision):
    """cell_head_ref.exact_rows / exact_weights: every stage from head_in to head_l2 must return fp32(ref64) bit for bit, in f16x3
    and in fp32, on max and on mean; `out` is held to normalize_bound on the exact head_l2.  Guard word 0."""
    hm = _model(case["d"], case["variation"], precision, 11, True)
    table, idx, cp = H.exact_rows(case)
    designed = H.exact_weights(case)
    p = _embed_pack(hm, table, designed)
    pn = H.head_pack(_numpy_pack(p))
    for k, v in designed.items():
        if isinstance(v, np.ndarray):
            assert G.bits_equal(pn[k], v), ("the matrices handed to the library are the designed ones", k)
    if precision == "f16x3":
        lo = {k: bool(_np(p[k + "_x3"][1]).any()) for k in ("g_wp", "g_wq", "g_w2")}
        assert lo == dict(g_wp=case["kind"] == "wpq2", g_wq=case["kind"] == "wpq2", g_w2=case["kind"] == "w22"), lo
    out, trace, guard = _embed_call(hm, p, idx, cp, case["variation"])
    assert guard == 0, "guard word %#x" % guard
    rows = table[idx]
    assert G.bits_equal(trace["obj_emb"], rows) and G.bits_equal(trace["head_in"], rows), "both normalisations return the row"
    knn = H.global_rows(trace["knn_idx"], cp)
    assert np.array_equal(knn, H.knn_oracle(rows, cp)), "knn_idx (distance-0 ties are broken by index)"
    ref = _cached(("exact", case["name"]), lambda: H.exact_headroom(case, rows, knn, cp, designed))
    assert ref is not None, "a value or a sum leaves the exact range"
    name = "%s-%s" % (case["name"], precision)
    for k in H.HEAD_TRACE:
        same = G.bits_equal(trace[k], ref[k].astype(F32))
        print("HEAD | %s | %s | %s | -" % (name, k[5:], "bit-equal" if same else "max err %.3g" % T.max_err(trace[k], ref[k])))
        assert same, "%s %s: not the exact result bit for bit (max error %.3g)" % (name, k, T.max_err(trace[k], ref[k]))
    _report(name, "out", precision, out, H.norm_ref64(ref["head_l2"]), H.norm_bound(ref["head_l2"]))
    if case["kind"] == "single" and case["variation"] == 0:
        assert (trace["head_l2"][:, 0] == F32(T.EXACT_PROBE)).all()


# ---- refusals and degenerate input -------------------------------------------------------------------------------------------------------

def _raw_call(hm, p, idx, cp, variation, out, trace):
    """t2p_encode_cells itself, on buffers the caller owns (ops.encode_cells allocates its own); len(cp) - 1 cells of cp[-1] objects.
    Returns the return code."""
    from text2pos_amd import _lib as L
    from text2pos_amd import ops
    dev = _dev()
    n, nb = int(cp[-1]), len(cp) - 1
    cfg = ops.make_cell_config(n_pts=8, embed_dim=hm.kernel_dim, use_features=("class",), variation=variation, precision=hm.precision,
                               class_idx=torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev))
    tr = L.CellTrace()
    for k, t in trace.items():
        setattr(tr, k, t.data_ptr())
    pts = torch.zeros((max(n, 1), 8, 3), dtype=torch.float32, device=dev)
    three = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    cp = np.ascontiguousarray(cp, np.int32)
    big = L.CellConfig.from_buffer_copy(cfg)
    big.chunk_objects = max(int(np.diff(cp).max()) if nb else 1, 1)
    nbytes = max(L.lib().t2p_encode_cells_workspace_bytes(max(n, 1), max(nb, 1), C.byref(cfg)),
                 L.lib().t2p_encode_cells_workspace_bytes(max(n, 1), max(nb, 1), C.byref(big)))
    ws = ops.workspace(dev, nbytes, "cell_head_test")
    cpd = torch.from_numpy(cp).to(dev)
    rc = L.lib().t2p_encode_cells(ops._ptr(pts), ops._ptr(pts), ops._ptr(three), ops._ptr(three), cp.ctypes.data_as(C.c_void_p),
                                  ops._ptr(cpd), n, nb, C.byref(ops.make_cell_weights(p)), C.byref(cfg), ops._ptr(out), C.byref(tr),
                                  ops._ptr(ws), ws.numel(), ops._stream(dev))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_cell_of_193_objects_is_refused_and_nothing_is_written(precision):
    from text2pos_amd import _lib as L
    hm = _model(256, 0, precision, 11, True)
    dev = _dev()
    sizes = (5, 193, 3)
    cp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(cp[-1])
    table = np.random.default_rng(4).standard_normal((n, 256)).astype(F32)
    p = _embed_pack(hm, table)
    before = dict(out=G.poison(3, 256), obj_emb=G.poison(n, 256), head_in=G.poison(n, 256), head_edge=G.poison(n, 256),
                  head_pool=G.poison(3, 256), head_l1=G.poison(3, 256), head_l2=G.poison(3, 256))
    bufs = {k: torch.from_numpy(v).to(dev) for k, v in before.items()}
    knn = torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    rc = _raw_call(hm, p, np.arange(n, dtype=np.int32), cp, 0, bufs["out"], dict({k: v for k, v in bufs.items() if k != "out"}, knn_idx=knn))
    assert rc == L.DEFINES["T2P_E_ARG"], rc
    assert "193" in L.lib().t2p_last_error().decode()
    for k, v in before.items():
        assert G.bits_equal(_np(bufs[k]), v), (k, "written by a refused call")
    assert (_np(knn) == 0x5A5A5A5A).all()
    # 192 objects are served
    cp2 = np.array([0, 5, 197, 200], np.int32)
    out, _, _ = _embed_call(hm, p, np.arange(200, dtype=np.int32), cp2, 0, want_trace=False)
    assert np.isfinite(out).all()


def test_no_cells_is_success():
    hm = _model(256, 0, "f16x3", 11, True)
    assert _raw_call(hm, _embed_pack(hm), np.zeros(1, np.int32), np.zeros(1, np.int32), 0, None, {}) == 0


@pytest.mark.parametrize("variation", [0, 1], ids=["max", "mean"])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_nan_in_an_embedding_row_reaches_its_cell(precision, variation):
    """A NaN in one object's embedding row, in a cell of 9 and in a cell of 1.  What happens, pinned: every distance to that object
    is NaN, so k_knn lists no neighbour for it (its row of knn_idx is -1) and no other object lists it; WS_EDGE_KNN leaves its row
    of head_edge at 0 - fmaxf and the int atomicMax would drop the NaN anyway.  Without more, the cell came back finite, computed
    from its other objects (the cell of 1: from nothing), with the guard word 0 - in both precisions.  k_segpool now reads the first
    neighbour slot: the pooled row of such a cell is NaN, lin and the final F.normalize carry it to `out`, and on the f16x3 path
    bit 6 of the guard word is raised (include/t2p.h).  Cells without such an object keep their bits."""
    hm = _model(256, variation, precision, 11, True)
    sizes = (9, 1, 4)
    cp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(cp[-1])
    table = np.random.default_rng(9).standard_normal((n, 256)).astype(F32)
    clean, _, guard = _embed_call(hm, _embed_pack(hm, table), np.arange(n, dtype=np.int32), cp, variation, want_trace=False)
    assert guard == 0 and np.isfinite(clean).all()
    bad = table.copy()
    bad[3, 5] = np.nan
    bad[9, 0] = np.nan
    out, tr, guard = _embed_call(hm, _embed_pack(hm, bad), np.arange(n, dtype=np.int32), cp, variation)
    knn = H.global_rows(tr["knn_idx"], cp)
    print("HEAD | nan-%s-%d | guard %#x | knn rows %s %s | out finite per cell %s" % (
        precision, variation, guard, knn[3].tolist(), knn[9].tolist(), np.isfinite(out).all(1).tolist()))
    assert (knn[[3, 9]] == -1).all() and not np.isin(knn, [3, 9]).any()
    assert not tr["head_edge"][[3, 9]].view(np.int32).any()
    assert np.isnan(tr["head_pool"][:2]).all() and np.isnan(out[:2]).all(), "a cell with a NaN object came back finite"
    if precision == "f16x3":
        assert guard & 64, "guard word %#x: bit 6 not raised" % guard
    assert G.bits_equal(out[2], clean[2]), "a cell without a NaN object changed"
