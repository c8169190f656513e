"""tests/trunk_ref.py proved on the CPU, so that the GPU tests built on it (tests/test_gpu_trunk_stages.py) mean what they say:
  * the row sets (traced tables + the self-loop rule) ARE the edge lists oracle/pyg_restated.py's PointConv aggregates over,
    for cells of 1, 2 and 5 objects, both self_loops values, 256 and 100 points per object (an odd level size);
  * the correct emulation of every stage stays within 1 x bound under five summation orders, both precisions, on the oracle's own
    activations (golden weights seed 11, synthetic.make_cells(31, 2));
  * R_SHARP is what the rule gives: 4 x the largest ratio between the five orders' maxima, rounded up to a power of two;
  * every wrong= variant is rejected and TIERS names the first tier that rejects it, per variant and stage: "a" = an element
    beyond 2 x bound, "b" = the maximum beyond R max(max|emul - ref64|, u max|ref64|), "c" = the variant's emulation does not
    return the exact inputs' bits.
    Margins of tier b (how far beyond the threshold the variant's maximum lies; measured here, printed with -s): SA2, SA3, lin2
    and the head leave 10 x and more for a lost fp16 plane.  GA and lin1 leave LESS than 8 x (4.1 - 4.2 x and 4.3 - 7.8 x: at
    K = 512 and 1,024 the sequential and the pairwise order of the CORRECT arithmetic already differ by 9 - 11 x, so R = 64
    there); LOW_MARGIN lists them, and tier c carries them: test_exact_inputs_are_exact shows that a lost lo.hi changes the
    single-plane set's bits at every stage, test_two_plane_sets_are_exact that a lost hi.lo changes the two-plane set's at SA1,
    SA2, SA3 and GA (lin1's kernel, k_gemm_x3, has its two-plane inputs in tests/test_gpu_gemm_family.py).
    `trunc_split` (activations split by truncation) only doubles the error on ordinary activations (0.7 - 2.2 x the correct
    emulation's: inside any R) - tier c: the probe channel of the exact inputs returns other bits under truncation, at every stage;
  * the exact inputs are exact: premises checked on the data, the emulation bit-equal to fp32(ref64) under every order, with and
    without fma, in both precisions;
  * the kernel and template each case reaches, restated from the launchers."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunk_ref as T  # noqa: E402

F32 = np.float32
SA = ("sa1", "sa2", "sa3")
# variant -> tier per stage (see the module text)
TIERS = {
    "sa1": dict(no_lo_hi="a", no_hi_lo="a", trunc_split="c", no_drain_scale="a", bias_unscaled="a", max_from_zero="a", self_own="a",
                drop33="a"),
    "sa2": dict(no_lo_hi="b", no_hi_lo="b", trunc_split="c", no_drain_scale="a", bias_unscaled="a", max_from_zero="a", self_own="a",
                drop33="a"),
    "sa3": dict(no_lo_hi="b", no_hi_lo="b", trunc_split="c", no_drain_scale="a", bias_unscaled="a", max_from_zero="a", self_own="a",
                drop33="a"),
    "ga": dict(no_lo_hi="b", no_hi_lo="b", trunc_split="c", ga_one_plane="b", max_from_zero="a"),
    "lin1": dict(no_lo_hi="b", no_hi_lo="b", trunc_split="c", no_drain_scale="a"),
    "lin2": dict(no_lo_hi="b", no_hi_lo="b", trunc_split="c", no_drain_scale="a"),
    "head": dict(no_lo_hi="b", no_hi_lo="b", no_drain_scale="a"),      # (its GEMMs' kernel, k_gemm_x3, is lin1's and lin2's)
}
# tier b with less than 8 x of room
LOW_MARGIN = {("ga", "no_lo_hi"), ("ga", "no_hi_lo"), ("ga", "ga_one_plane"), ("lin1", "no_lo_hi"), ("lin1", "no_hi_lo")}


def _numpy_pack(p):
    out = {}
    for k, v in p.items():
        if isinstance(v, (list, tuple)):
            out[k] = [t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in v]
        else:
            out[k] = v.detach().cpu().numpy() if torch.is_tensor(v) else v
    return out


@functools.lru_cache(maxsize=None)
def _oracle(seed=11):
    import weights as W
    import text2pos_amd  # noqa: F401
    from oracle import model as OM
    from text2pos_amd import packing
    from text2pos_amd import synthetic as S
    om = OM.OracleCellRetrieval(S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words(), OM.default_args()).eval()
    W.fill_state_dict(om, seed)
    p = packing.pack_cell_weights(om, "cpu", x3=False)
    scales = dict(sa=[packing.f16x3_scale(t) for t in p["sa_w2"]], lin1=packing.f16x3_scale(p["lin1_w"]),
                  lin2=packing.f16x3_scale(p["lin2_w"]))
    return om, _numpy_pack(p), scales


@functools.lru_cache(maxsize=None)
def _activations():
    """The oracle's activations of make_cells(31, 2) at every stage boundary, and the groups of oracle/primitives.c."""
    from text2pos_amd import synthetic as S
    om, p, scales = _oracle()
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(31, 2)
    tr = []
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # one thread: the activations, and with them the maxima R is derived from, do not depend on
    try:                              # what ran before (other tests set the thread count)
        om.encode_objects_packed(xyz, rgb, center, mean_rgb, cell_ptr, trace=tr)
    finally:
        torch.set_num_threads(threads)
    pn = [d for d in tr if "sa" in d]
    cat = lambda f: np.concatenate([f(d).numpy() for d in pn])
    return dict(xyz=xyz, rgb=rgb, cell_ptr=cell_ptr, groups=T.oracle_groups(xyz),
                sa_out=[cat(lambda d, l=l: d["sa"][l]["out"]) for l in range(3)],
                f0=cat(lambda d: d["features0"]), f1=cat(lambda d: d["features1"]), f2=cat(lambda d: d["features2"]))


def _sa_args(level, n_objects=2, self_loops=True, wrong=None, act=None, p=None):
    """(feat, pos, cpos, src, dst, w1, b1, w2, b2) of a level on the oracle's activations, the centroids of the first n_objects."""
    act = act or _activations()
    p = p or _oracle()[1]
    g = act["groups"]
    n_pts = act["xyz"].shape[1]
    nd, nc = T.level_geometry(n_pts)[level]
    feat = act["rgb"].reshape(-1, 3) if level == 0 else act["sa_out"][level - 1]
    pos = act["xyz"].reshape(-1, 3) if level == 0 else g["pos"][level - 1].reshape(-1, 3)
    cpos = g["pos"][level].reshape(-1, 3)
    src, dst = T.edge_rows(g["nbr"][level], g["cnt"][level], act["cell_ptr"], nd, nc, self_loops, wrong)
    if n_objects is not None:
        keep = dst < n_objects * nc
        src, dst, cpos = src[keep], dst[keep], cpos[: n_objects * nc]
    cin = feat.shape[1]
    return (feat, pos, cpos, src, dst, p["sa_w1"][level][: cin + 3], p["sa_b1"][level], p["sa_w2"][level], p["sa_b2"][level])


def _ga_args(n_objects=8):
    act, p = _activations(), _oracle()[1]
    nc = T.level_geometry(256)[2][1]
    return (act["sa_out"][2][: n_objects * nc], act["groups"]["pos"][2].reshape(-1, 3)[: n_objects * nc], n_objects,
            p["ga_w1"][:259], p["ga_b1"], p["ga_w2"], p["ga_b2"])


def _lin_args(name):
    act, p = _activations(), _oracle()[1]
    return (act["f0"] if name == "lin1" else act["f1"]), p[name + "_w"], p[name + "_b"]


@functools.lru_cache(maxsize=None)
def _stage(stage, precision):
    """(ref64, bound, emul(order, wrong)) of a stage on the oracle's activations."""
    scales = _oracle()[2]
    if stage in SA:
        l = SA.index(stage)
        args, pk = _sa_args(l), precision == "f16x3" and l == 0
        ref = T.sa_ref64(*args)
        return (ref["out"], T.sa_bound(ref, *args, precision, scales["sa"][l], pk),
                lambda order, wrong=None: T.sa_emul(*args, precision, scales["sa"][l], pk, order, wrong))
    if stage == "ga":
        args = _ga_args()
        ref = T.ga_ref64(*args)
        return ref["out"], T.ga_bound(ref, *args, precision), lambda order, wrong=None: T.ga_emul(*args, precision, order, wrong)
    if stage == "head":
        from text2pos_amd import packing
        from text2pos_amd import synthetic as S
        act, p = _activations(), dict(_oracle()[1])
        _, _, center, mean_rgb, _ = S.make_cells(31, 2)
        p.update(pn_scale=packing.f16x3_scale(torch.from_numpy(p["pn_w"])), merge_scale=packing.f16x3_scale(torch.from_numpy(p["merge_w"])))
        pieces = T.object_head_ref64(act["f2"], center, mean_rgb, p)
        return (pieces["out"], T.object_head_bound(pieces, act["f2"], center, mean_rgb, p, precision),
                lambda order, wrong=None: T.object_head_emul(act["f2"], center, mean_rgb, p, precision, order, wrong))
    a, w, b = _lin_args(stage)
    ref = T.dense_ref64(a, w, b)
    return (ref, T.dense_bound(ref, a, w, b, precision, scales[stage]),
            lambda order, wrong=None: T.dense_emul(a, w, b, precision, scales[stage], order, wrong))


@functools.lru_cache(maxsize=None)
def _order_maxima(stage, precision):
    ref, bound, emul = _stage(stage, precision)
    out = {}
    for order in T.ORDERS:
        e = emul(order)
        out[order] = (T.max_err(e, ref), T.worst_ratio(e, ref, bound))
    return out


STAGES = SA + ("ga", "lin1", "lin2")
ALL_STAGES = STAGES + ("head",)


# ---- row sets ---------------------------------------------------------------------------------------------------------------------------

class _Capture(torch.nn.Module):
    """local_nn of a PointConv that records the messages it is handed."""

    def __init__(self):
        super().__init__()
        self.msg = None

    def forward(self, msg):
        self.msg = msg.clone()
        return msg


def _pyg_edges(pos, idx, batch, radius, self_loops):
    """The (source dense row, target centroid row) list PointConv aggregates over, read out of oracle/pyg_restated.py itself: the
    features carry the dense row number, the centroid 'positions' minus the centroid row number."""
    from oracle import pyg_restated as gnn
    cent, dense = gnn.radius(pos, pos[idx], radius, batch_x=batch, batch_y=batch[idx])
    cap = _Capture()
    conv = gnn.PointConv(local_nn=cap, add_self_loops=self_loops)
    nd, nc = pos.shape[0], idx.shape[0]
    x = torch.arange(nd, dtype=torch.float64)[:, None]
    zero = torch.zeros((nd, 3), dtype=torch.float64)
    cpos = torch.zeros((nc, 3), dtype=torch.float64)
    cpos[:, 0] = -torch.arange(nc, dtype=torch.float64)
    conv(x, (zero, cpos), torch.stack((dense, cent), dim=0))
    return cap.msg[:, 0].long().numpy(), cap.msg[:, 1].long().numpy()


@pytest.mark.parametrize("n_pts", [256, 100])
@pytest.mark.parametrize("self_loops", [True, False])
@pytest.mark.parametrize("cell_size", [1, 2, 5])
def test_row_sets_are_pyg_restated_edge_lists(cell_size, self_loops, n_pts):
    from oracle import pyg_restated as gnn
    from text2pos_amd import synthetic as S
    xyz = S.make_objects(77, 0, 3 + cell_size, 256)[0][:, :n_pts].copy()
    xyz[1] = xyz[1, np.arange(n_pts) % 3]                      # three distinct points: tail centroids
    cell_ptr = np.array([0, 3, 3 + cell_size])                 # the cell under test is NOT the first: global rows differ from local
    lo = 3
    g = T.oracle_groups(xyz)
    pos = torch.from_numpy(xyz[lo:].reshape(-1, 3).copy())
    batch = torch.arange(cell_size).repeat_interleave(n_pts)
    for l, (nd, nc) in enumerate(T.level_geometry(n_pts)):
        idx = gnn.fps(pos, batch, 0.5)
        assert np.array_equal(idx.numpy().reshape(cell_size, nc) - np.arange(cell_size)[:, None] * nd, g["fps_idx"][l][lo:])
        want_src, want_dst = _pyg_edges(pos, idx, batch, T.RADIUS[l], self_loops)
        src, dst = T.edge_rows(g["nbr"][l], g["cnt"][l], cell_ptr, nd, nc, self_loops)
        mine = dst >= lo * nc
        got = sorted(zip((src[mine] - lo * nd).tolist(), (dst[mine] - lo * nc).tolist()))
        assert got == sorted(zip(want_src.tolist(), want_dst.tolist())), (l, "edge multiset")
        assert np.all(np.diff(dst) >= 0)
        pos, batch = pos[idx], batch[idx]


# ---- bounds, R, wrong variants ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("stage", ALL_STAGES)
def test_correct_emulation_within_one_bound(stage, precision):
    ref, bound, emul = _stage(stage, precision)
    for order, (err, ratio) in _order_maxima(stage, precision).items():
        print("%-5s %-6s %-9s max err %.3g  err / bound %.3g" % (stage, precision, order, err, ratio))
        assert ratio <= 1.0, (stage, precision, order, ratio)
    assert T.within(emul("tile"), ref, bound, 1.0)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("stage", ALL_STAGES)
def test_r_is_four_times_the_spread_of_the_orders(stage, precision):
    maxima = [m for m, _ in _order_maxima(stage, precision).values()]
    print("%-5s %-6s largest / smallest %.2f -> R %g" % (stage, precision, max(maxima) / min(maxima), T.derive_r(maxima)))
    assert T.R_SHARP[precision][stage] == T.derive_r(maxima)      # (_activations pins the oracle run to one thread: reproducible)


def _tier(stage, got, ref, bound, emul_tile):
    """(tier, margin over the threshold of tier b)."""
    thr = T.sharp_threshold(emul_tile, ref, "f16x3", stage)
    margin = T.max_err(got, ref) / thr
    if not T.within(got, ref, bound, T.FACTOR_GPU):
        return "a", margin
    return ("b" if margin > 1.0 else None), margin


@pytest.mark.parametrize("stage", ALL_STAGES)
def test_arithmetic_wrong_variants_are_rejected(stage):
    ref, bound, emul = _stage(stage, "f16x3")
    good = emul("tile")
    assert _tier(stage, good, ref, bound, good)[0] is None
    for wrong, want in TIERS[stage].items():
        if wrong in T.ROW_WRONG:
            continue
        tier, margin = _tier(stage, emul("tile", wrong), ref, bound, good)
        print("%-5s %-15s tier %-4s max err = %.3g x threshold of (b)" % (stage, wrong, tier, margin))
        if want == "c":       # neither (a) nor (b) sees it on ordinary activations; test_exact_inputs_are_exact proves (c) does
            assert tier is None, (stage, wrong, tier, margin)
            continue
        assert tier == want, (stage, wrong, tier, margin)
        if tier == "b":
            assert margin >= (2.0 if (stage, wrong) in LOW_MARGIN else 8.0), (stage, wrong, margin)
        else:
            assert (stage, wrong) not in LOW_MARGIN


@functools.lru_cache(maxsize=None)
def _case_chain(self_loops=True):
    """The GPU cases' objects (odd kinds among them) with activations of their own: the fp32 emulation, level after level."""
    p = _oracle()[1]
    xyz, rgb, _, _, cell_ptr = T.case_objects()
    act = dict(xyz=xyz, rgb=rgb, cell_ptr=cell_ptr, groups=T.oracle_groups(xyz), sa_out=[])
    for l in range(3):
        args = _sa_args(l, None, self_loops, None, act, p)
        act["sa_out"].append(T.sa_emul(*args, "fp32", 1.0, False, "tile").astype(F32))
    return act


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("wrong", T.ROW_WRONG)
def test_row_set_wrong_variants_are_rejected(wrong, level):
    """A loop row taken from the object's own points, or a full centroid's 33rd row dropped, moves outputs far beyond the bound
    (tier a) - on the cases' objects, which hold centroids at the 32-hit cap and single-row centroids."""
    act, p, scales = _case_chain(), _oracle()[1], _oracle()[2]
    args = _sa_args(level, None, True, None, act, p)
    bad = _sa_args(level, None, True, wrong, act, p)
    cnt = act["groups"]["cnt"][level]
    assert (cnt == 32).any() and (cnt == 1).any(), "the cases must hold centroids at the cap and centroids of one hit"
    ref = T.sa_ref64(*args)
    for precision in ("f16x3", "fp32"):
        bound = T.sa_bound(ref, *args, precision, scales["sa"][level], precision == "f16x3" and level == 0)
        got = T.sa_ref64(*bad)["out"]
        worst = T.worst_ratio(got, ref["out"], bound)
        print("SA%d %-8s %-6s err / bound %.3g" % (level + 1, wrong, precision, worst))
        assert not T.within(got, ref["out"], bound, T.FACTOR_GPU)
        assert TIERS[SA[level]][wrong] == "a"


def test_channels_negative_on_every_row_exist():
    """What `max_from_zero` hides must be there to hide: (centroid, channel) pairs whose every row is negative before the ReLU,
    among them centroids of a single row."""
    act, p = _case_chain(False), _oracle()[1]
    for l in range(3):
        args = _sa_args(l, None, False, None, act, p)
        ref = T.sa_ref64(*args)
        top = T.segmax(ref["pre2"], args[4], args[2].shape[0], empty=np.inf)
        assert (top < 0.0).any(), l
        single = np.flatnonzero(np.bincount(args[4], minlength=args[2].shape[0]) == 1)
        assert len(single) and (top[single] < 0.0).any(), l


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact_chain(two_plane=None):
    """ref64 of the exact inputs, stage by stage (each stage on fp32(ref64) of the one before), with the stage arguments; a
    two-plane set up to its stage."""
    xyz, rgb, _, _, cell_ptr = T.exact_objects(two_plane)
    p = T.exact_weights(two_plane=two_plane)
    act = dict(xyz=xyz, rgb=rgb, cell_ptr=cell_ptr, groups=T.oracle_groups(xyz), sa_out=[])
    stages = {}
    for l in range(3):
        args = _sa_args(l, None, True, None, act, p)
        ref = T.sa_ref64(*args)
        stages[SA[l]] = (ref, _sa_args(l, 2, True, None, act, p), args)
        act["sa_out"].append(ref["out"].astype(F32))
        if two_plane == SA[l]:
            return act, p, stages
    n = xyz.shape[0]
    args = (act["sa_out"][2], act["groups"]["pos"][2].reshape(-1, 3), n, p["ga_w1"][:259], p["ga_b1"], p["ga_w2"], p["ga_b2"])
    ref = T.ga_ref64(*args)
    stages["ga"] = (ref, (args[0][:128], args[1][:128], 4) + args[3:], args)
    a = ref["out"].astype(F32)
    for name in () if two_plane else ("lin1", "lin2"):
        out = T.dense_ref64(a, p[name + "_w"], p[name + "_b"])
        stages[name] = (out, (a[:8], p[name + "_w"], p[name + "_b"]), (a, p[name + "_w"], p[name + "_b"]))
        a = out.astype(F32)
    return act, p, stages


EXACT_UNITS = dict(sa1=(2.0 ** -10, 2.0 ** -12), sa2=(2.0 ** -13, 2.0 ** -14), sa3=(2.0 ** -15, 2.0 ** -16), ga=(2.0 ** -17, 2.0 ** -18),
                   lin1=(None, 2.0 ** -19), lin2=(None, 2.0 ** -20))


def _emul_of(stage, args, precision, order, scale, wrong=None):
    if stage in SA:
        return T.sa_emul(*args, precision, scale if precision == "f16x3" else 1.0, precision == "f16x3" and stage == "sa1", order, wrong)
    if stage == "ga":
        return T.ga_emul(*args, precision, order, wrong)
    return T.dense_emul(*args, precision, scale, order, wrong)


def _exact_under_every_order(stage, small, full, want, scale):
    """16-k tiles on every row, the one-term-at-a-time orders (with and without fma in fp32) on the first objects' rows."""
    for precision in ("f16x3", "fp32"):
        assert T.G.bits_equal(_emul_of(stage, full, precision, "tile", scale).astype(F32), want), (stage, precision, "tile")
    n_small = small[2].shape[0] if stage in SA else (small[2] if stage == "ga" else small[0].shape[0])
    for precision in ("f16x3", "fp32"):
        for order in T.ORDERS:
            for fma in ((True, False) if precision == "fp32" else (True,)):
                T._FMA[0] = fma
                try:
                    got = _emul_of(stage, small, precision, order, scale)
                finally:
                    T._FMA[0] = True
                assert T.G.bits_equal(got.astype(F32), want[:n_small]), (stage, precision, order, fma)


@pytest.mark.parametrize("stage", STAGES)
def test_exact_inputs_are_exact(stage):
    """The premises (units, magnitudes below 4, hi + lo = the value, the probe in channel 0) hold on the data; the emulation
    equals fp32(ref64) bit for bit under every order, with and without fma, in both precisions; the inputs hold what they must:
    dead channels, single-row centroids, centroids at the cap.  Tier (c) for the wrong variants: an emulation that splits by
    truncation, or drops lo.hi, does NOT return those bits - at every stage."""
    from text2pos_amd import packing
    act, p, stages = _exact_chain()
    ref, small, full = stages[stage]
    out = ref["out"] if isinstance(ref, dict) else ref
    h_unit, o_unit = EXACT_UNITS[stage]
    assert T.exact_headroom(out[:, 1:], o_unit, 4.0) and np.all(out[:, 0] == T.EXACT_PROBE)
    if isinstance(ref, dict):
        assert T.exact_headroom(ref["h"][:, 1:], h_unit, 4.0) and np.all(ref["h"][:, 0] == T.EXACT_PROBE)
        hi, lo = T.split_f16(ref["h"])
        assert np.array_equal(hi + lo, ref["h"])
        assert (out.max(0) == 0.0).any() and (out > 0).any(), "channels that are negative on every row, and live ones"
    assert T.exact_headroom(act["xyz"], T.EXACT_GRID, 2.0) and T.exact_headroom(act["rgb"], T.EXACT_GRID_RGB, 1.0 + 2.0 ** -8)
    assert all(packing.f16x3_scale(torch.from_numpy(w)) == 2.0 ** 14 for w in p["sa_w2"] + [p["lin1_w"], p["lin2_w"]])
    if stage in SA:
        cnt = act["groups"]["cnt"][SA.index(stage)]
        assert (cnt == 32).any() and (cnt == 1).any() and len(np.unique(act["xyz"][20], axis=0)) == 3
    want = out.astype(F32)
    _exact_under_every_order(stage, small, full, want, 2.0 ** 14)
    for wrong in ("trunc_split", "no_lo_hi"):
        got = _emul_of(stage, full, "f16x3", "tile", 2.0 ** 14, wrong).astype(F32)
        assert not T.G.bits_equal(got, want), (stage, wrong, "tier c must see it")
        if wrong == "trunc_split":
            assert TIERS[stage][wrong] == "c" and (got[:, 0] != want[:, 0]).any(), "the probe channel is where truncation shows"


@pytest.mark.parametrize("stage", T.TWO_PLANE_STAGES)
def test_two_plane_sets_are_exact(stage):
    """The two-plane set of a stage: activations in front of it single-plane (8 bits), the stage's outputs multiples of 2^-17 below
    17, the emulation bit-equal to fp32(ref64) under every order in both precisions - and NOT bit-equal once hi.lo is dropped
    (tier c for `no_hi_lo` at SA1, SA2, SA3 and GA layer 2), while the single-plane set cannot tell."""
    from text2pos_amd import packing
    act, p, stages = _exact_chain(stage)
    ref, small, full = stages[stage]
    assert T.exact_headroom(ref["h"], 2.0 ** -4, 16.0) and T.exact_headroom(ref["out"], 2.0 ** -17, 17.0)
    hi, lo = T.split_f16(ref["h"])
    assert not lo.any(), "single-plane activations"
    w2 = p["ga_w2"] if stage == "ga" else p["sa_w2"][SA.index(stage)]
    scale = packing.f16x3_scale(torch.from_numpy(w2))
    assert scale == 2.0 ** 13
    wh, wl = T.split_f16(w2.astype(np.float64) * (1.0 if stage == "ga" else scale), False, 2048.0 if stage == "ga" else 1.0)
    assert np.array_equal(wh + wl, w2.astype(np.float64) * (1.0 if stage == "ga" else scale)) and (wl != 0).sum() == w2.shape[1]
    for before in list(stages)[:-1]:
        r = stages[before][0]
        assert T.exact_headroom(r["out"], 2.0 ** -4, 16.0), before
    want = ref["out"].astype(F32)
    assert (want > 0).any() and (ref["out"].max(0) == 0.0).any()
    _exact_under_every_order(stage, small, full, want, scale)
    assert not T.G.bits_equal(_emul_of(stage, full, "f16x3", "tile", scale, "no_hi_lo").astype(F32), want)
    single = _exact_chain()[2][stage]
    assert T.G.bits_equal(_emul_of(stage, single[2], "f16x3", "tile", 2.0 ** 14, "no_hi_lo").astype(F32),
                          (single[0]["out"]).astype(F32)), "single-plane weights: hi.lo is zero there"


# ---- dispatch, restated ------------------------------------------------------------------------------------------------------------------

def test_kernels_each_case_reaches():
    reach = {c["name"]: T.kernels_reached(c["n_pts"], c["precision"], c["self_loops"], c["tuning"], c["full_trace"]) for c in T.CASES}
    assert len(reach) == len(T.CASES), "case names are unique"
    assert reach["x3"]["sa1"] == "k_sa_points" and reach["x3"]["sa2"] == "k_sa_rows" and reach["x3"]["sa3"] == "k_sa3"
    assert reach["x3"]["ga2"] == "k_ga2<32>" and reach["x3"]["scan"] == "list" and reach["x3"]["sa1_rows"] == "k_dedup_rows"
    assert reach["x3"]["share_tail"] and not reach["x3-tuning-4"]["share_tail"] and not reach["x3-100"]["share_tail"]
    assert reach["fp32"]["sa3"] == "k_sa_stream<256,256,fp32>" and reach["fp32"]["heads"] == "k_gemm"
    assert reach["x3-maskplan"]["scan"] == "mask" and reach["x3-maskplan"]["sa1_rows"] == "k_build_rows"
    assert reach["x3-maskplan-noloops"]["prune_dup"] and not reach["x3-maskplan"]["prune_dup"]
    assert not reach["x3-noloops-tuning-4"]["prune_dup"] and reach["x3-noloops-tuning-4"]["scan"] == "mask"
    assert reach["x3-tuning-8"]["scan"] == "list" and reach["x3-tuning-8"]["sa1_rows"] == "k_dedup_rows"
    assert reach["x3-tuning-1"]["sa1_rows"] == "full" and reach["x3-tuning-d"]["sa1_rows"] == "full"
    assert reach["x3-100"]["sa1"] == "k_sa_stream<32,64,x3>" and reach["x3-100"]["ga2"] == "k_ga2<16>"
    assert [T.ga_group(n) for n in (256, 100, 64, 8)] == [32, 16, 8, 1]
    assert [T.level_geometry(100)[l] for l in range(3)] == [(100, 50), (50, 25), (25, 13)]
    for want in ("fp32", "f16x3"):
        assert sum(c["precision"] == want for c in T.CASES) >= 8
    assert {c["tuning"] for c in T.CASES} == {0, 0xD, 1, 4, 8} and {c["n_pts"] for c in T.CASES} == {256, 100, 64, 8}
    assert {c["features"] for c in T.CASES} == {0, 1, 2} and {c["chunk"] for c in T.CASES} == {0, 8}
    assert {c["rescale"] for c in T.CASES if c["rescale"]} == {(r, s) for r in ("sa2 hidden", "sa3 output", "ga hidden")
                                                              for s in (16.0, 0.125)}
    xyz, _, _, _, ptr = T.case_objects()
    assert xyz.shape[0] == 40 <= 48 and list(np.diff(ptr)) == list(T.CELL_SIZES)
    assert len(np.unique(xyz[20], axis=0)) == 3
