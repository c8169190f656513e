"""The forward kernels of the fine matcher on the MI355X, each against tests/fine_forward_ref.py:
  1. k_attn_sets (ops.match_attention) against float64 softmax attention, |kernel - ref64| <= 2 x bound, element by element;
  2. k_head_sets (ops.match_head), float64 inside: P within u P64 + 4 delta64, every decision whose margin is at least 1e-3, the
     scores, three thresholds, ties;
  3. k_match_final alone (ops.match without a GNN layer, final_proj the identity), float64 inside since this file found the fp32
     recurrence wanting: the bound and the decisions of 2., the offset MLP at D = 64, 128 and 256, the head of the training path on
     the same tokens, k_concat's grid stride, ops.match_indexed;
  4. k_attn through one layer pair with weights under which the attention matters: |P - P64| <= 4 e32 with no floor, both
     precisions, the item loop's second pass, the largest token sets the LDS takes and the refusal of the next size up.
Every test prints what it measures before it asserts (pytest -s); docs/notebook.md, "The fine matcher's forward kernels against
float64", is where the figures are recorded."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fine_backward_ref as FB  # noqa: E402
import fine_forward_ref as FF  # noqa: E402
from train_ops_ref import F32, within, worst_ratio  # noqa: E402

pytestmark = pytest.mark.gpu

F16X3_FACTOR = 1.0       # on the fp32 bar of part 4 (at most 2), see test_matcher_with_attention_that_matters
OUTPUTS = ("P", "matches0", "matches1", "matching_scores0", "matching_scores1")


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a)).to(_dev())


def _cpu(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _weights(kind, d, arg, precision="fp32", offsets=None):
    """kind "head": no layer, identity final_proj, bin_score arg; kind "match": arg layer pairs of the part-4 weights."""
    from text2pos_amd import ops, packing
    if kind == "head":
        h = FF.head_only_holder(d, arg, None if offsets is None else FF.offset_weights(d, *offsets))
    else:
        h = FF.match_holder(d, arg)
    return ops.make_match_weights(packing.pack_match_weights(h, "cuda:0", precision)), h


def _check_decisions(got, z, thresh, score_ok, ties=False):
    """matches0 / matches1 equal to the float64 decisions wherever the margin is at least 1e-3; the scores exp of the winning log
    coupling where the match is mutual and exactly 0 elsewhere; `> thresh` exactly where the match is >= 0.  Returns the shares of
    entries below the margin."""
    m0, m1, s0, s1 = FF.decisions(z, thresh)
    g0, g1 = FF.margins(z, thresh, ties)
    shares = []
    for got_m, got_s, want_m, want_s, g in ((got["matches0"], got["matching_scores0"], m0, s0, g0),
                                            (got["matches1"], got["matching_scores1"], m1, s1, g1)):
        ok = g >= FF.MARGIN
        shares.append(float((~ok).mean()))
        assert shares[-1] <= FF.MARGIN_CAP
        assert got_m.dtype == np.int64 and np.array_equal(got_m[ok], want_m[ok])
        assert np.array_equal(got_s[ok] == 0.0, want_s[ok] == 0.0)
        assert score_ok(got_s[ok], want_s[ok])
        assert np.array_equal(got_s > F32(thresh), got_m >= 0)              # on the kernel's own outputs: exact
        assert ((got_m >= -1) & (got_m < z.shape[2 if got_m is got["matches0"] else 1] - 1)).all()
    return shares


# ---- 1. attention forward, the kernel alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("shape", FB.ATTN_SHAPES)
def test_attention_forward_kernel(shape, cross):
    from text2pos_amd import _lib as L, ops
    B, M, N, D = shape
    for family in FF.ATTN_FAMILIES:
        qkv = FF.attn_fwd_inputs(*shape, family)
        ref, bound = FF.attn_fwd_ref64(qkv, *shape, cross), FF.attn_fwd_bounds(qkv, *shape, cross)
        q = _t(qkv)
        out = torch.full((B * (M + N), D), float("nan"), device=_dev())    # an element the kernel does not write shows as NaN
        L.check(L.lib().t2p_match_attention(ops._ptr(q), B, M, N, D, cross, ops._ptr(out), ops._stream(_dev())), "t2p_match_attention")
        got = out.cpu().numpy()
        again = ops.match_attention(q, B, M, N, bool(cross))
        print(f"attention forward {shape} cross={cross} {family}: {worst_ratio(got, ref, bound):.3f} x bound, largest error "
              f"{np.nanmax(np.abs(got - ref)):.2e} at scale {np.abs(ref).max():.2e}")
        assert not np.isnan(got).any()
        assert within(got, ref, bound, 2.0)
        assert torch.equal(out, again)                           # bit for bit
        if family == "shifted":      # the unshifted reference: 2 x for the kernel, 1 x for the rounding of k + shift (host test)
            assert within(got, FF.attn_fwd_ref64(FF.attn_fwd_inputs(*shape, "unshifted"), *shape, cross), bound, 3.0)


# ---- 2. head forward, the kernel alone ----------------------------------------------------------------------------------------------
def _head_score_ok(ref):
    return lambda got, want: within(got, want, FF.head_score_bound(ref, want), 2.0)


@pytest.mark.parametrize("case", FF.HEAD_CASES, ids=FF.head_case_id)
def test_head_forward_kernel(case):
    from text2pos_amd import ops
    (B, M, N, D), iters, alpha, _ = case
    ref = FF.head_reference(case)
    x = _t(ref["md"])
    bound = FF.head_p_bound(ref)
    for thresh in FF.THRESHOLDS:
        got = _cpu(ops.match_head(x, B, M, N, alpha, iters, thresh))
        shares = _check_decisions(got, ref["z64"], thresh, _head_score_ok(ref))
        if thresh == 0.2:
            print(f"head forward {FF.head_case_id(case)}: P {worst_ratio(got['P'], ref['p64'], bound):.3f} x bound (largest error "
                  f"{np.abs(got['P'] - ref['p64']).max():.2e}, delta64 {ref['delta64']:.2e}); below the margin {shares[0]:.3f} / "
                  f"{shares[1]:.3f}; {(got['matches0'] >= 0).sum()} matches")
        if thresh == FF.THRESHOLDS[0]:
            first = got
        assert got["P"].shape == (B, M + 1, N + 1) and within(got["P"], ref["p64"], bound, 2.0)
        assert np.array_equal(got["P"], first["P"])              # the threshold moves no coupling
        if thresh == 1e9:
            assert (got["matches0"] == -1).all() and (got["matches1"] == -1).all()
        if thresh == 0.0:                                        # every mutual pair is a match
            assert np.array_equal(got["matches0"] >= 0, got["matching_scores0"] > 0)
            assert np.array_equal(got["matches1"] >= 0, got["matching_scores1"] > 0)


def test_head_forward_leaves_the_rows_behind_its_outputs_alone():
    from text2pos_amd import _lib as L, ops
    case = ((3, 5, 7, 64), 50, 1.0, 1.0)
    (B, M, N, D), iters, alpha, _ = case
    ref = FF.head_reference(case)
    x = _t(ref["md"])
    sizes = dict(P=B * (M + 1) * (N + 1), matches0=B * M, matches1=B * N, matching_scores0=B * M, matching_scores1=B * N)
    buf = {}
    for k, n in sizes.items():
        if k.startswith("matches"):
            buf[k] = torch.full((n + 16,), -9, dtype=torch.int64, device=_dev())
        else:
            buf[k] = torch.full((n + 16,), float("nan"), device=_dev())
            buf[k][n:] = -7.0
    L.check(L.lib().t2p_match_head(ops._ptr(x), B, M, N, D, alpha, iters, 0.2, *(ops._ptr(buf[k]) for k in OUTPUTS), ops._stream(_dev())),
            "t2p_match_head")
    want = ops.match_head(x, B, M, N, alpha, iters, 0.2)
    for k, n in sizes.items():
        assert torch.equal(buf[k][:n], want[k].reshape(-1)), k                  # written everywhere, and the same bits twice
        assert bool((buf[k][n:] == (-9 if k.startswith("matches") else -7.0)).all()), k
    assert not torch.isnan(buf["P"]).any() and not torch.isnan(buf["matching_scores0"]).any()


@pytest.mark.parametrize("tie", FF.TIE_CASES, ids=lambda t: f"side{t[0]}-planted{int(t[1])}")
def test_ties_go_to_the_first_index_in_both_heads(tie):
    """A hint (object) row duplicated bit for bit: the object (hint) keeps the lower index, the higher duplicate gets -1 and a score
    of exactly 0 - in k_head_sets and in k_match_final alike, whose five outputs are equal bit for bit."""
    from text2pos_amd import ops
    side, planted = tie
    B, M, N, D = FF.TIE_SHAPES[side]
    ref = FF.tie_case(side, planted)
    dup, z, src, dst = ref["md"], ref["z64"], ref["src"], ref["dst"]
    lo, hi = min(src, dst), max(src, dst)
    w, _ = _weights("head", D, FF.TIE_ALPHA)
    d0, d1 = (_t(a) for a in FF.to_sample_major(dup, B, M, N))
    for thresh in (0.0, 0.2):
        both = {}
        for name, got, score_ok in (("k_head_sets", ops.match_head(_t(dup), B, M, N, FF.TIE_ALPHA, FF.TIE_ITERS, thresh), _head_score_ok(ref)),
                                    ("k_match_final", ops.match(d0, d1, w, FF.TIE_ITERS, thresh), _head_score_ok(ref))):
            got = both[name] = _cpu(got)
            _check_decisions(got, z, thresh, score_ok, ties=True)
            p = got["P"]
            assert np.array_equal(p[:, lo, :], p[:, hi, :]) if side == 0 else np.array_equal(p[:, :, lo], p[:, :, hi]), name
            own, own_s, other = (("matches0", "matching_scores0", "matches1") if side == 0 else ("matches1", "matching_scores1", "matches0"))
            assert (got[own][:, hi] == -1).all() and (got[own_s][:, hi] == 0.0).all(), name
            assert not (got[other] == hi).any(), name
            want = FF.decisions(z, thresh)
            for k, v in zip(OUTPUTS[1:3], want[:2]):              # all five outputs of the rows the tie touches
                rows = [lo, hi] if k == own else slice(None)
                assert np.array_equal(got[k][:, rows], v[:, rows]), (name, k)
        for k in OUTPUTS:                                        # the two heads agree on all five outputs, bit for bit
            assert np.array_equal(both["k_head_sets"][k], both["k_match_final"][k]), k
    print(f"tie {tie}: token {src} copied over {dst}; matches0 {got['matches0'][0]}, matches1 {got['matches1'][0]}")


# ---- 3. the inference head alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FF.HEAD_CASES, ids=FF.head_case_id)
def test_inference_head_kernel(case):
    """k_match_final carries its recurrence in float64, as k_head_sets does, and is held to the same bound: u P64 + 4 delta64.
    Measured on an MI355X: 0.997 x the bound at most (the one rounding of P).  At the first threshold all five outputs are the
    training head's on the same tokens, bit for bit and everywhere, not only above the margin: the two kernels run one body.  With the
    fp32 recurrence it had before, log P lay up to 3.2e-5 from float64 (spread 8, 63 + 63 tokens; at most 2.004 x the distance of
    a NumPy fp32 recurrence, no decision flipped) - 45 to 470 of these bounds at spread 8 - and the matcher of
    test_matcher_with_attention_that_matters missed its bar through it."""
    from text2pos_amd import ops
    (B, M, N, D), iters, alpha, _ = case
    ref = FF.head_reference(case)
    w, _ = _weights("head", D, alpha)
    d0, d1 = (_t(a) for a in FF.to_sample_major(ref["md"], B, M, N))
    bound = FF.head_p_bound(ref)
    for thresh in FF.THRESHOLDS:
        got = _cpu(ops.match(d0, d1, w, iters, thresh))
        shares = _check_decisions(got, ref["z64"], thresh, _head_score_ok(ref))
        if thresh == FF.THRESHOLDS[0]:
            first = got
            # the head of the training path on the same tokens, set-major: one body (csrc/match_common.h), so the same bits everywhere
            other = _cpu(ops.match_head(_t(ref["md"]), B, M, N, alpha, iters, thresh))
            differ = {k: int((got[k] != other[k]).sum()) for k in OUTPUTS}
            print(f"inference head {FF.head_case_id(case)}: P {worst_ratio(got['P'], ref['p64'], bound):.3f} x bound (largest error "
                  f"{np.abs(got['P'] - ref['p64']).max():.2e}, delta64 {ref['delta64']:.2e}, smallest P64 {ref['p64'].min():.1e}); below the "
                  f"margin {shares[0]:.3f} / {shares[1]:.3f}; entries that differ from the training head's: {differ}")
            for k in OUTPUTS:
                assert got[k].dtype == other[k].dtype and np.array_equal(got[k], other[k]), k
            assert within(got["P"], other["P"], 2.0 * bound, 2.0)
            g0, g1 = FF.margins(ref["z64"], thresh)
            assert np.array_equal(got["matches0"][g0 >= FF.MARGIN], other["matches0"][g0 >= FF.MARGIN])
            assert np.array_equal(got["matches1"][g1 >= FF.MARGIN], other["matches1"][g1 >= FF.MARGIN])
        assert got["P"].shape == (B, M + 1, N + 1) and within(got["P"], ref["p64"], bound, 2.0)
        assert np.array_equal(got["P"], first["P"])              # the threshold moves no coupling
        if thresh == 1e9:
            assert (got["matches0"] == -1).all() and (got["matches1"] == -1).all()


@pytest.mark.parametrize("neg_bias", [False, True])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_offset_mlp(D, neg_bias):
    """H = D / 2 = 32 (fewer units than lanes), 64, 128 (two passes).  The bound is a worst case, nothing is measured: factor 1."""
    from text2pos_amd import ops
    B, M, N = 3, 5, 7
    w, h = _weights("head", D, 1.0, "fp32", (5, neg_bias))
    ow = FF.holder_offset_weights(h)
    d0, d1 = FF.to_sample_major(FF.head_inputs(B, M, N, D, 1.0)[0], B, M, N)
    x = d1.reshape(-1, D)
    ref, bound = FF.offsets_ref64(x, *ow), FF.offsets_bounds(x, *ow)
    got = ops.match(_t(d0), _t(d1), w, 1, 0.2)["offsets"].cpu().numpy()
    clamped = float((FF.offsets_hidden64(x, ow[0], ow[1]) < -1e-3).mean())       # (the fp32 sum is within 1e-5 of it)
    print(f"offsets D={D} negative bias={neg_bias}: {worst_ratio(got.reshape(-1, 2), ref, bound):.3f} x bound, "
          f"{clamped:.2f} of the hidden units clamped to 0")
    assert got.shape == (B, N, 2) and within(got.reshape(-1, 2), ref, bound, 1.0)
    assert clamped > (0.5 if neg_bias else 0.05)


def test_concat_grid_stride():
    """3,000 samples of 16 + 6 tokens at D = 256 are 16.9 M elements, more than k_concat's 65,535 x 256 threads: the stride is taken.
    The batch is 8 samples tiled; every output of sample b equals that of sample b mod 8 of the 8-sample call, bit for bit."""
    from text2pos_amd import ops
    B, M, N, D, reps = 8, 16, 6, 256, 375
    assert B * reps * (M + N) * D > 65535 * 256
    w, _ = _weights("head", D, 1.0)
    d0, d1 = (_t(a) for a in FF.to_sample_major(FF.head_inputs(B, M, N, D, 1.0)[0], B, M, N))
    small = ops.match(d0, d1, w, FF.MATCH_ITERS, 0.2)
    big = ops.match(d0.repeat(reps, 1, 1), d1.repeat(reps, 1, 1), w, FF.MATCH_ITERS, 0.2)
    for k, v in small.items():
        assert big[k].shape[0] == B * reps
        assert torch.equal(big[k].reshape((reps,) + tuple(v.shape)), v[None].expand((reps,) + tuple(v.shape))), k
    assert torch.isfinite(small["P"]).all() and int((small["matches0"] >= 0).sum()) > 0
    ops.release_workspaces()                                     # (0.6 GB of scratch for this one call)


def test_match_indexed_equals_match_on_the_gathered_rows():
    from text2pos_amd import ops
    case = ((3, 5, 7, 64), 50, 1.0, 1.0)
    (B, M, N, D), iters, alpha, _ = case
    w, _ = _weights("head", D, alpha)
    obj, hint = (_t(a) for a in FF.to_sample_major(FF.head_reference(case)["md"], B, M, N))
    obj_row = torch.tensor([2, 0, 0, 1, 2, 1, 0], dtype=torch.int32, device=_dev())
    hint_row = torch.tensor([1, 1, 0, 2, 0, 1, 2], dtype=torch.int32, device=_dev())
    got = ops.match_indexed(obj, hint, obj_row, hint_row, w, iters, 0.2)
    want = ops.match(obj[obj_row.long()].contiguous(), hint[hint_row.long()].contiguous(), w, iters, 0.2)
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert int((want["matches0"] >= 0).sum()) > 0


# ---- 4. the inference attention, through one layer pair -----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("shape", FF.all_match_shapes(), ids=lambda s: "B%dM%dN%dD%dL%d" % s)
def test_matcher_with_attention_that_matters(shape, precision):
    """|P - P64| <= 4 e32 (fp32; f16x3: F16X3_FACTOR times that), e32 the fp32 oracle's own distance from the float64 oracle - no
    floor.  The host test shows that a wrong scale, a plain mean, contiguous heads, a dropped token or the wrong source set move
    the float64 P by at least ten of these bars.  Measured on an MI355X: 0.04 to 0.25 e32 in both precisions (f16x3 needs no factor
    of its own).  With the fp32 head of before: 0.54 to 4.05 e32 - (2, 60, 5, 128) at 2.51e-6 against a bar of 2.48e-6, on the
    dustbin coupling P = 4.9, where one fp32 ulp is 4.8e-7."""
    from text2pos_amd import ops
    b, m, n, d, layers = shape
    ref = FF.match_reference(shape)
    bar = ref["bar"] * (F16X3_FACTOR if precision == "f16x3" else 1.0)
    w, _ = _weights("match", d, layers, precision)
    got = _cpu(ops.match(*(_t(a) for a in FF.match_inputs(b, m, n, d)), w, FF.MATCH_ITERS, 0.2))
    err = float(np.abs(got["P"] - ref["p64"]).max())
    shares = _check_decisions(got, ref["z64"], 0.2, lambda g, want: bool(np.all(np.abs(g - want) <= bar)))
    print(f"matcher {shape} {precision}: |P - P64| {err:.2e} = {err / ref['e32']:.2f} e32 = {err / bar:.3f} x bound (e32 {ref['e32']:.2e}); "
          f"below the margin {shares[0]:.3f} / {shares[1]:.3f}; {(got['matches0'] >= 0).sum()} matches")
    assert F16X3_FACTOR <= 2.0
    assert err <= bar


@pytest.mark.parametrize("edge", FF.edge_shapes(), ids=lambda s: "B%dM%dN%dD%dL%d" % s)
def test_next_size_past_the_lds_edge_is_refused_and_launches_nothing(edge):
    from text2pos_amd import _lib as L, ops
    b, m, n, d, layers = edge
    m, n = (m + 1, n + 1) if m == n else (m + 1, n)
    assert FF.lds_floats(m, n, d) > FF.LDS_FLOATS and m <= 63
    w, _ = _weights("match", d, layers)
    d0, d1 = (_t(a) for a in FF.match_inputs(b, m, n, d))
    sizes = dict(P=b * (m + 1) * (n + 1), matches0=b * m, matches1=b * n, matching_scores0=b * m, matching_scores1=b * n, offsets=b * n * 2)
    buf = {k: torch.full((s,), -9, dtype=torch.int64 if k.startswith("matches") else torch.float32, device=_dev()) for k, s in sizes.items()}
    ws = torch.empty((L.lib().t2p_match_workspace_bytes(b, m, n, d),), dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        rc = L.lib().t2p_match(ops._ptr(d0), ops._ptr(d1), b, m, n, d, C.byref(w), FF.MATCH_ITERS, 0.2, *(ops._ptr(buf[k]) for k in sizes),
                               ops._ptr(ws), ws.numel(), ops._stream(_dev()))
        with pytest.raises(L.T2PError, match=r"need %d B of LDS per sample \(> 160 KiB\)" % (4 * FF.lds_floats(m, n, d))):
            L.check(rc, "t2p_match")
    finally:
        ops.profile_enable(False)
    assert rc == -3                                              # T2P_E_UNSUPPORTED
    assert ops.profile_report() == {}
    torch.cuda.synchronize()
    assert all(bool((v == -9).all()) for v in buf.values())
