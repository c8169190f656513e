"""tests/cell_head_ref.py proved on the CPU, so that tests/test_gpu_cell_head.py means what it says.  On the GPU test's own
embedding-path cases (the same tables and weight fills, at D = 256, 128, 64 and 300, both precisions, max and mean; a subset of
the destinations - up to 9 objects of every cell - keeps the ordered emulations within seconds):
  * every stage's emulation stays within 1 x its bound of ref64 under the five summation orders of trunk_ref.ORDERS;
  * cell_head_ref.R_SHARP is what the rule gives: derive_r over the orders' maxima, the largest over the cases;
  * every order of the RIGHT arithmetic lies below the (B) threshold of its stage and every wrong emulation of the stage's list
    above it - so substituting any one of them for the right emulation fails that stage - and the variants of NOT_SEPARATED do
    not (they are carried by the exact family, or by nothing: pool_from_zero);
  * the exact family is exact: premises checked on the data (exact_headroom), the emulation bit-equal to fp32(ref64) under every
    order, with and without fma, in both precisions; every wrong emulation but pool_from_zero returns other bits on some set;
  * the float64 reference chained over the oracle's own obj_emb IS oracle64.cell_head (1e-12), on variation 0 and 1;
  * the case list reaches what it claims to reach (branches_reached)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cell_head_ref as H  # noqa: E402
import trunk_ref as T  # noqa: E402

F32 = np.float32
HOST_CASES = [c for c in H.EMBED_CASES if c["sizes"] == H.EMBED_SIZES and c["chunk"] == 0]


def _oracle(d, variation, seed, **kw):
    import weights as W
    import text2pos_amd  # noqa: F401
    from oracle import model as OM
    from text2pos_amd import synthetic as S
    args = OM.default_args(embed_dim=d, variation=variation, **kw)
    om = OM.OracleCellRetrieval(S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words(), args).eval()
    W.fill_state_dict(om, seed)
    return om


@functools.lru_cache(maxsize=None)
def _weights(d, variation, seed):
    """The head's folded fp32 pack at the kernels' width, as the product packs it for the class_embed model of that width."""
    from text2pos_amd import packing
    om = _oracle(d, variation, seed, use_features=["class"], class_embed=True)
    om.kernel_dim = packing.kernel_embed_dim(d)
    p = packing.pack_cell_weights(om, "cpu", x3=False)
    return H.head_pack({k: (v.numpy() if torch.is_tensor(v) else v) for k, v in p.items()})


def _host_dsts(cp):
    return np.concatenate([np.arange(cp[c], cp[c] + min(cp[c + 1] - cp[c], 9)) for c in range(len(cp) - 1)])


@functools.lru_cache(maxsize=None)
def _measured(name):
    """Per stage of a case: the orders' (max error, worst error / bound), the (B) threshold of the tile emulation, and the wrong
    emulations' maxima.  Every stage reads the fp32 image of the stage before's float64 reference."""
    case = next(c for c in HOST_CASES if c["name"] == name)
    d, precision, mean = case["d"], case["precision"], case["variation"] == 1
    p = _weights(d, case["variation"], case["seed"])
    table, idx, cp = H.embed_table(case)
    emb = H.norm_emul(table[idx]).astype(F32)               # obj_emb as k_gather_rownorm leaves it
    out = {}

    def stage(name_, ref, bound, emul, wrongs, ordered=True):
        orders = {o: emul(o, None) for o in (T.ORDERS if ordered else ("tile",))}
        rec = dict(orders={o: (T.max_err(e, ref), T.worst_ratio(e, ref, bound)) for o, e in orders.items()},
                   umax=H.U * float(np.abs(ref).max()), wrong={w: T.max_err(emul("tile", w), ref) for w in wrongs})
        rec["base"] = max(rec["orders"]["tile"][0], rec["umax"])
        out[name_] = rec

    stage("in", H.norm_ref64(emb), H.norm_bound(emb), lambda o, w: H.norm_emul(emb), (), False)
    xn = H.norm_emul(emb).astype(F32)
    knn = H.knn_oracle(xn, cp)
    ds = _host_dsts(cp)
    ref = H.edge_ref64(xn, knn, p, mean, ds)
    wrongs = [w for w in H.EDGE_WRONG[precision] + H.NOT_SEPARATED["edge"] if mean or w != "mean_over_k"]
    stage("edge", ref["out"], H.edge_bound(ref, xn, p, precision, mean),
          lambda o, w: H.edge_emul(xn, knn, p, precision, mean, o, w, ds), wrongs)
    edge = H.edge_ref64(xn, knn, p, mean)["out"].astype(F32)
    pr = H.pool_ref64(edge, cp, mean)
    stage("pool", pr, H.pool_bound(pr, edge, cp, mean), lambda o, w: H.pool_emul(edge, cp, mean, w), H.NOT_SEPARATED["pool"], False)
    a = pr.astype(F32)
    for st in ("l1", "l2"):
        w_, b_ = p["lin_w" + st[1]], p["lin_b" + st[1]]
        lr = H.lin_ref64(a, w_, b_)
        stage(st, lr, H.lin_bound(lr, a, w_, b_), lambda o, w, a=a, w_=w_, b_=b_: H.lin_emul(a, w_, b_, o, w),
              H.LIN_WRONG + H.NOT_SEPARATED[st])
        a = lr.astype(F32)
    stage("out", H.norm_ref64(a), H.norm_bound(a), lambda o, w: H.norm_emul(a), (), False)
    return out


@pytest.mark.parametrize("name", [c["name"] for c in HOST_CASES])
def test_emulations_stay_within_their_bounds_and_wrong_ones_leave_the_threshold(name):
    precision = next(c for c in HOST_CASES if c["name"] == name)["precision"]
    m = _measured(name)
    for stage, rec in m.items():
        for order, (err, ratio) in rec["orders"].items():
            assert ratio <= 1.0, "%s %s %s: the emulation at %.3g x bound" % (name, stage, order, ratio)
        if stage not in H.SHARP_STAGES:
            continue
        r = H.R_SHARP[precision][stage]
        assert T.derive_r([e for e, _ in rec["orders"].values()]) <= r, (name, stage)
        thr = r * rec["base"]
        for order, (err, _) in rec["orders"].items():
            assert err <= thr, "%s %s: the right arithmetic in order %s lies above the (B) threshold" % (name, stage, order)
        listed = (H.EDGE_WRONG[precision] if stage == "edge" else H.LIN_WRONG)
        for w, err in rec["wrong"].items():
            print("HEAD-HOST | %s | %s | %s | %.3g x threshold" % (name, stage, w, err / thr))
            if w in listed:
                assert err > thr, "%s %s: wrong=%s passes (B): %.3g <= %.3g" % (name, stage, w, err, thr)
            else:
                assert w in H.NOT_SEPARATED[stage] and err <= thr, (name, stage, w, "separates after all: move it to the stage's list")
    assert m["pool"]["wrong"]["pool_from_zero"] == m["pool"]["orders"]["tile"][0], "head_edge >= 0: a max from 0 is the same max"


def test_r_sharp_is_what_the_rule_gives():
    """R of a stage and precision: derive_r over the five orders' maxima, the largest over the cases (printed with -s: the maxima
    of docs/notebook.md)."""
    for precision in ("f16x3", "fp32"):
        for stage in H.SHARP_STAGES:
            rs = []
            for c in HOST_CASES:
                if c["precision"] == precision:
                    errs = {o: e for o, (e, _) in _measured(c["name"])[stage]["orders"].items()}
                    rs.append(T.derive_r(list(errs.values())))
                    print("HEAD-R | %s | %s | R %g | %s" % (c["name"], stage, rs[-1], " ".join("%s %.3g" % kv for kv in errs.items())))
            assert max(rs) == H.R_SHARP[precision][stage], (precision, stage, rs)
            assert T.R_SHARP[precision]["head_" + stage] == max(rs)


# ---- the exact family -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact(name):
    case = next(c for c in H.EXACT_CASES if c["name"] == name)
    table, idx, cp = H.exact_rows(case)
    p = H.exact_weights(case)
    rows = table[idx]
    knn = H.knn_oracle(rows, cp)
    return case, rows, cp, p, knn, H.exact_headroom(case, rows, knn, cp, p)


def _exact_chain(case, rows, cp, p, knn, precision, order, wrong=None):
    """The emulations chained from the table rows; wrong goes to the stage it belongs to."""
    mean = case["variation"] == 1
    xn = H.norm_emul(H.norm_emul(rows))
    edge = H.edge_emul(xn, knn, p, precision, mean, order, wrong if wrong != "pool_from_zero" else None)
    pool = H.pool_emul(edge, cp, mean, wrong)
    l1 = H.lin_emul(pool, p["lin_w1"], p["lin_b1"], order)
    return dict(head_in=xn, head_edge=edge, head_pool=pool, head_l1=l1, head_l2=H.lin_emul(l1, p["lin_w2"], p["lin_b2"], order))


@pytest.mark.parametrize("name", [c["name"] for c in H.EXACT_CASES])
def test_exact_family_is_exact(name):
    case, rows, cp, p, knn, ref = _exact(name)
    assert ref is not None, "%s: a value or a sum leaves the exact range (exact_units)" % name
    assert len(np.unique(rows, axis=0)) < len(rows) or max(case["sizes"]) < 3, "repeated rows: distance-0 ties inside a cell"
    if case["variation"] == 1:
        assert all(s & (s - 1) == 0 for s in case["sizes"]), "mean cases divide by powers of two only"
    else:
        assert (ref["head_edge"] == 0).any() and (knn < 0).any()
    for precision in ("f16x3", "fp32"):
        for order in T.ORDERS:
            for fma in ((True, False) if order in ("seq", "random") else (True,)):   # (tile and pairwise have no fma form)
                T._FMA[0] = fma
                try:
                    got = _exact_chain(case, rows, cp, p, knn, precision, order)
                finally:
                    T._FMA[0] = True
                for k in H.HEAD_TRACE:
                    assert np.array_equal(ref[k].astype(F32).astype(np.float64), ref[k]), (name, k, "ref64 is an fp32 number")
                    assert T.G.bits_equal(got[k].astype(F32), ref[k].astype(F32)), (name, precision, order, fma, k)
    bound = H.norm_bound(ref["head_l2"])
    assert T.within(H.norm_emul(ref["head_l2"]), H.norm_ref64(ref["head_l2"]), bound, 1.0)


def test_no_wrong_emulation_returns_the_exact_bits():
    """Every wrong emulation changes the bits of some exact set's stage (pool_from_zero of none); a single-plane set is blind
    to a lost cross plane, the two-plane sets and the probe channel are not."""
    rejected = {}
    for c in H.EXACT_CASES:
        case, rows, cp, p, knn, ref = _exact(c["name"])
        for precision in ("f16x3", "fp32"):
            for w in H.EDGE_WRONG[precision] + (("trunc_split",) if precision == "f16x3" else ()) + ("pool_from_zero",):
                got = _exact_chain(case, rows, cp, p, knn, precision, "tile", w)
                if not all(T.G.bits_equal(got[k].astype(F32), ref[k].astype(F32)) for k in H.HEAD_TRACE):
                    rejected.setdefault((precision, w), []).append(c["name"])
    for precision in ("f16x3", "fp32"):
        for w in H.EDGE_WRONG[precision]:
            assert rejected.get((precision, w)), (precision, w, "no exact set sees it")
    assert rejected.get(("f16x3", "trunc_split")), "the probe channel sees a truncating split"
    assert any("wpq2" in n for n in rejected[("f16x3", "no_hi_lo")]) and any("w22" in n for n in rejected[("f16x3", "no_hi_lo")])
    assert any("lowbias" in n for n in rejected[("f16x3", "no_lo_hi")])
    assert not rejected.get(("f16x3", "pool_from_zero")) and not rejected.get(("fp32", "pool_from_zero"))


# ---- the reference is the oracle's head -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variation", [0, 1])
def test_chained_reference_is_the_oracles_cell_head(variation):
    """head_ref64 over the oracle's own obj_emb, with the oracle's layers folded in float64, against oracle64.cell_head on the same
    graph: 1e-12 - the stage references are the oracle's head, not a second opinion of it."""
    import knn_graph as KG
    from text2pos_amd import packing
    from text2pos_amd import synthetic as S
    om = _oracle(256, variation, 11)
    xyz, rgb, center, mean_rgb, _ = S.make_cells(31, 6)
    cell_ptr = np.array([0, 1, 3, 10, 18, 27, 50, xyz.shape[0]], np.int32)      # cells of 1, 2, 7, 8, 9, 23 and the rest
    tr = []
    with torch.no_grad():
        om.encode_objects_packed(xyz, rgb, center, mean_rgb, cell_ptr, trace=tr)
    emb = next(d["object_embeddings"] for d in tr if "object_embeddings" in d).numpy().astype(F32)
    assert emb.shape == (int(cell_ptr[-1]), 256)
    knn = KG.oracle_knn(emb, cell_ptr)
    d = 256
    k = lambda w: w.double().t().contiguous().numpy()
    w1, b1 = packing.fold_linear_bn(om.graph1.nn[0])
    w2, b2 = packing.fold_linear_bn(om.graph1.nn[1])
    l1w, l1b = packing.fold_linear_bn(om.lin[0])
    l2w, l2b = packing.fold_linear_bn(om.lin[1])
    p = dict(g_wp=k(w1[:, :d] - w1[:, d:]), g_bp=b1.numpy(), g_wq=k(w1[:, d:]), g_w2=k(w2), g_b2=b2.numpy(), lin_w1=k(l1w),
             lin_b1=l1b.numpy(), lin_w2=k(l2w), lin_b2=l2b.numpy())
    got = H.head_ref64(emb, cell_ptr, knn, p, variation == 1)["out"]
    want = KG.cell_head64(KG.float64_oracle(om), emb, cell_ptr, knn=knn)
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
    assert (np.diff(cell_ptr) < 8).any() and (np.diff(cell_ptr) > 8).any(), "cells below and above k"


# ---- what the cases reach ---------------------------------------------------------------------------------------------------------------

def test_case_list_reaches_every_branch():
    cus = T.G.NUM_CUS
    cases = H.EMBED_CASES + H.FULL_CASES + [dict(c, sizes=H.group32_sizes(cus)) for c in H.GROUP32_CASES] + \
        [dict(c, precision=pr) for c in H.EXACT_CASES for pr in ("f16x3", "fp32")]
    reached = [(c, H.branches_reached(c, cus)) for c in cases]
    assert set().union(*[b["group"] for _, b in reached]) == {8, 32}
    assert {b["build"] for _, b in reached} == {"ws_edge_knn<%d, %s, %s>" % (dk, how, pr) for dk, how in (
        (256, "256 columns on 8 waves"), (128, "128 columns on 4 waves"), (384, "3 slices of 128 columns on 4 waves")) for pr in ("x3", "fp32")}
    for build in {b["build"] for _, b in reached}:
        assert {b["agg"] for _, b in reached if b["build"] == build} == {"max", "mean"}, build
    by_name = {c["name"]: b for c, b in reached}
    for pr in ("x3", "fp32"):
        for agg in ("max", "mean"):
            assert by_name["emb-300-%s-%s" % (pr, agg)]["knn"] == {"unstaged"}, "a 192-object cell switches staging off for its chunk"
            assert by_name["emb-300-%s-%s-staged" % (pr, agg)]["knn"] == {"staged", "unstaged"}, "cells of 65 rows next to staged ones"
    for c, b in reached:
        if c in H.EMBED_CASES:
            assert b["straddle"] and b["ragged"] and b["short_cell"], c["name"]
    assert by_name["emb-256-x3-max-chunk100"]["chunks"] == 4 and all(by_name[c["name"]]["chunks"] == 3 for c in H.FULL_CASES)
    for c in H.GROUP32_CASES:
        assert by_name[c["name"]]["group"] == {32} and by_name[c["name"]]["straddle"] and by_name[c["name"]]["ragged"]
        first = [s for s in np.cumsum(H.group32_sizes(cus)) if s <= 1000]
        assert H.branches_reached(dict(c, sizes=H.group32_sizes(cus)[: len(first)]), cus)["group"] == {8}
    assert H.knn_stage_rows(192, 384) == 0 and H.knn_stage_rows(65, 384) == 64 and H.knn_stage_rows(9, 256) == 9
