"""CPU tests of the references the GPU tests of the fine matcher's forward rely on (tests/fine_forward_ref.py): every float64 statement
reproduces oracle/fine.py in float64, every fp32 emulation lies within its own bound (within half of it where the bound is first
order), `within` rejects every deliberately wrong formula, the committed inputs leave at most 2 % of their decisions below the
margin, a wrong attention moves the float64 P of part 4 by at least ten bars, and the LDS edge of t2p_match is where the formula
puts it - refused on the host, before anything touches a device.  Every test prints what it measures (pytest -s); docs/notebook.md,
"The fine matcher's forward kernels against float64", is where the figures are recorded."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from text2pos_amd import _lib  # noqa: E402
from oracle import fine as OF  # noqa: E402

import fine_backward_ref as FB  # noqa: E402
import fine_forward_ref as FF  # noqa: E402
import fine_train_ref as R  # noqa: E402
from train_ops_ref import F32, U, within, worst_ratio  # noqa: E402

TWO_SHAPES = [(2, 4, 2, 128), (3, 5, 7, 64)]


# ---- the float64 statements against oracle/fine.py ------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("shape", TWO_SHAPES)
def test_attention_reference_is_the_oracles_attention(shape, cross):
    """The einsum lines of oracle.fine.Propagation.forward (oracle/fine.py:49-54) on the q | k | v columns, set by set."""
    B, M, N, D = shape
    qkv = torch.from_numpy(np.array(FF.attn_fwd_inputs(*shape, "plain"))).double()
    dh = D // OF.NUM_HEADS
    sets = [qkv[:B * M].reshape(B, M, 3 * D), qkv[B * M:].reshape(B, N, 3 * D)]
    want = []
    for ts in (0, 1):
        x, source = sets[ts], sets[1 - ts if cross else ts]
        n, m = x.shape[1], source.shape[1]
        q = x[:, :, :D].reshape(B, n, dh, OF.NUM_HEADS)
        k = source[:, :, D:2 * D].reshape(B, m, dh, OF.NUM_HEADS)
        v = source[:, :, 2 * D:].reshape(B, m, dh, OF.NUM_HEADS)
        scores = torch.einsum("bndh,bmdh->bhnm", q, k) / dh ** 0.5
        prob = torch.nn.functional.softmax(scores, dim=-1)
        want.append(torch.einsum("bhnm,bmdh->bndh", prob, v).reshape(B * n, D))
    want = torch.cat(want).numpy()
    got = FF.attn_fwd_ref64(qkv.float().numpy(), *shape, cross)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("shape", TWO_SHAPES)
def test_head_reference_is_the_oracles_head(shape):
    """OracleSuperGlue without a layer, final_proj the identity, in float64: P, both match lists and both score lists."""
    B, M, N, D = shape
    case = (shape, 50, -2.0, 8.0)
    ref = FF.head_reference(case)
    sg = OF.OracleSuperGlue(D, 0, 50).double().eval()
    with torch.no_grad():
        sg.final_proj.weight.copy_(torch.eye(D))
        sg.final_proj.bias.zero_()
        sg.bin_score.fill_(-2.0)
        want = sg(*(torch.from_numpy(a).double() for a in FF.to_sample_major(ref["md"], B, M, N)))
    m0, m1, s0, s1 = FF.decisions(ref["z64"], OF.MATCH_THRESHOLD)
    assert np.abs(ref["p64"] - want["P"].numpy()).max() <= 1e-12
    assert np.array_equal(m0, want["matches0"].numpy()) and np.array_equal(m1, want["matches1"].numpy())
    assert (m0 >= 0).any()
    assert np.abs(s0 - want["matching_scores0"].numpy()).max() <= 1e-12 and np.abs(s1 - want["matching_scores1"].numpy()).max() <= 1e-12
    a0, a1 = FF.margins(ref["z64"], 0.2)
    b0, b1 = R.decision_margins(ref["p64"])
    assert np.allclose(a0, b0, rtol=0, atol=1e-9) and np.allclose(a1, b1, rtol=0, atol=1e-9)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_offsets_reference_is_the_oracles_mlp(D):
    w = FF.offset_weights(D, 5)
    x = FF.to_sample_major(FF.head_inputs(3, 5, 7, D, 1.0)[0], 3, 5, 7)[1].reshape(-1, D)
    mlp = torch.nn.Sequential(torch.nn.Linear(D, D // 2), torch.nn.ReLU(), torch.nn.Linear(D // 2, 2)).double()
    with torch.no_grad():
        for lin, (wt, b) in zip((mlp[0], mlp[2]), ((w[0], w[1]), (w[2], w[3]))):
            lin.weight.copy_(torch.from_numpy(np.array(wt)).double().t())
            lin.bias.copy_(torch.from_numpy(np.array(b)).double())
        want = mlp(torch.from_numpy(x).double()).numpy()
    assert np.abs(FF.offsets_ref64(x, *w) - want).max() <= 1e-13


# ---- emulations inside, mutants outside -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("shape", FB.ATTN_SHAPES)
def test_attention_emulation_inside_its_bound_and_every_mutant_outside(shape, cross):
    """"drop_last" is held to the plain family only: in a peaked row the last source token can carry no weight at all, and leaving
    it out is then within rounding by nature ((2, 63, 1, 64) cross, where eight rows in all have more than one source token)."""
    for family in FF.ATTN_FAMILIES:
        qkv = FF.attn_fwd_inputs(*shape, family)
        ref, bound = FF.attn_fwd_ref64(qkv, *shape, cross), FF.attn_fwd_bounds(qkv, *shape, cross)
        r = worst_ratio(FF.attn_fwd_emul(qkv, *shape, cross), ref, bound)
        print(f"attention forward {shape} cross={cross} {family}: emulation {r:.3f} x bound")
        assert not np.isnan(ref).any() and r <= 0.5
        for wrong in FF.ATTN_MUTANTS:
            if wrong == "no_max" and family != "shifted":
                continue
            if not FF.attn_mutant_can_differ(shape, wrong) or (wrong == "drop_last" and family != "plain"):
                continue
            assert not within(FF.attn_fwd_emul(qkv, *shape, cross, wrong=wrong), ref, bound, 2.0), (family, wrong)
        if family == "shifted":                              # the shift itself costs one rounding of k: inside 1 x the bound
            plain = FF.attn_fwd_ref64(FF.attn_fwd_inputs(*shape, "unshifted"), *shape, cross)
            assert within(plain, ref, bound, 1.0)


@pytest.mark.parametrize("case", FF.HEAD_CASES, ids=FF.head_case_id)
def test_head_inputs_bounds_and_margins(case):
    """The float64 evaluation rounded once lies inside the float64 head's bound; the fp32 recurrence does not where the scores are
    peaked (which is what the bound is there to tell apart); at most 2 % of the decisions lie below the margin."""
    ref = FF.head_reference(case)
    (B, M, N, D), iters, alpha, spread = case
    bound = FF.head_p_bound(ref)
    assert within(ref["p64"].astype(F32), ref["p64"], bound, 1.0)
    with np.errstate(over="ignore"):
        p32 = np.exp(ref["z32"])
    share0, share1 = FF.below_margin(ref["z64"])
    print(f"head {FF.head_case_id(case)}: delta64 {ref['delta64']:.2e}, d32 {ref['d32']:.2e}, an fp32 recurrence "
          f"{worst_ratio(p32, ref['p64'], bound):.1f} x the bound; below the margin {share0:.3f} / {share1:.3f}; "
          f"smallest P {ref['p64'].min():.1e}")
    if spread > 1.0 and max(M, N) > 1:
        assert not within(p32, ref["p64"], bound, 2.0)
    assert share0 <= FF.MARGIN_CAP and share1 <= FF.MARGIN_CAP
    for thresh in (0.0, 1e9):                                # a threshold out of reach only widens the margins
        t0, t1 = FF.below_margin(ref["z64"], thresh)
        assert t0 <= share0 and t1 <= share1
    m0 = FF.decisions(ref["z64"], 0.0)[0]
    assert (FF.decisions(ref["z64"], 1e9)[0] == -1).all() and (m0 >= 0).any()


@pytest.mark.parametrize("tie", FF.TIE_CASES)
def test_tie_cases_walk_the_mutual_logic(tie):
    """A duplicated token ties two columns (rows) bit for bit: the first index wins, the second duplicate is nobody's partner.  The
    last-index rule gives other lists; the margins of everything the tie does not decide hold."""
    side, planted = tie
    B, M, N, D = FF.TIE_SHAPES[side]
    ref = FF.tie_case(side, planted)
    z, src, dst = ref["z64"], ref["src"], ref["dst"]
    lo, hi = min(src, dst), max(src, dst)
    for thresh in (0.0, 0.2):
        m0, m1, s0, s1 = FF.decisions(z, thresh)
        own, other = (m0, m1) if side == 0 else (m1, m0)
        own_s = s0 if side == 0 else s1
        assert (own[:, hi] == -1).all() and (own_s[:, hi] == 0.0).all()       # the higher duplicate never wins a tie
        assert not (other == hi).any()
        assert max(FF.below_margin(z, thresh, ties=True)) <= FF.MARGIN_CAP
        w0, w1, _, _ = FF.decisions(z, thresh, wrong="last_index")
        if thresh == 0.0 and planted:
            assert (own[:, lo] >= 0).any()                                      # and the lower one does, somewhere
            assert not (np.array_equal(m0, w0) and np.array_equal(m1, w1))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_offsets_emulation_inside_its_bound_and_every_mutant_outside(D):
    x = FF.to_sample_major(FF.head_inputs(3, 5, 7, D, 1.0)[0], 3, 5, 7)[1].reshape(-1, D)
    for neg in (False, True):
        w = FF.offset_weights(D, 5, neg)
        ref, bound = FF.offsets_ref64(x, *w), FF.offsets_bounds(x, *w)
        r = worst_ratio(FF.offsets_emul(x, *w), ref, bound)
        pre = FF.offsets_hidden64(x, w[0], w[1])
        clamped = float((pre < 0).mean())
        print(f"offsets D={D} negative bias={neg}: emulation {r:.3f} x bound, {clamped:.2f} of the hidden units clamped")
        assert r <= 1.0
        assert 0.05 <= clamped <= 0.95
        for wrong in ("no_relu", "relu_out", "no_bias1"):
            assert not within(FF.offsets_emul(x, *w, wrong=wrong), ref, bound, 2.0), wrong


# ---- part 4: attention that matters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FF.all_match_shapes(), ids=lambda s: "B%dM%dN%dD%dL%d" % s)
def test_a_wrong_attention_moves_the_float64_couplings_by_ten_bars(shape):
    """Each mutant is a monkeypatch of oracle.fine.Propagation.forward (FF.oracle_p restores it)."""
    ref = FF.match_reference(shape)
    share0, share1 = FF.below_margin(ref["z64"])
    moves = {}
    for wrong in FF.ORACLE_MUTANTS:
        before = OF.Propagation.forward
        moves[wrong] = float(np.abs(FF.oracle_p(shape, torch.float64, wrong)["P"].numpy() - ref["p64"]).max())
        assert OF.Propagation.forward is before
    print(f"matcher {shape}: e32 {ref['e32']:.2e}, bar {ref['bar']:.2e}, below the margin {share0:.3f} / {share1:.3f}; moved by "
          + ", ".join(f"{k} {v:.1e} ({v / ref['bar']:.0f} bars)" for k, v in moves.items()))
    assert share0 <= FF.MARGIN_CAP and share1 <= FF.MARGIN_CAP
    assert 0.0 < ref["e32"] < 1e-4
    if max(shape[1], shape[2]) > 1:
        for wrong, v in moves.items():
            assert v >= FF.SEPARATION * ref["bar"], wrong
    else:                                                    # one token a side: a softmax over one logit is exempt by nature
        assert all(moves[w] == 0.0 for w in FF.ORACLE_MUTANTS if w != "wrong_source")


@pytest.mark.parametrize("shape", [(7, 9, 4, 64, 1), (33, 3, 11, 128, 2)], ids=lambda s: "B%dM%dN%dD%dL%d" % s)
def test_golden_weights_alone_do_not_see_the_attention(shape):
    """The table of the notebook, at the shapes of test_match_other_shapes_vs_oracle: without the gain on q and k a wrong scale and no
    softmax at all move P by less than the 1e-4 those tests allow."""
    p = FF.oracle_p(shape, torch.float64, gain=1.0)["P"].numpy()
    moves = {w: float(np.abs(FF.oracle_p(shape, torch.float64, w, gain=1.0)["P"].numpy() - p).max())
             for w in ("scale_d", "uniform", "contiguous_heads")}
    print(f"gain 1 {shape}: " + ", ".join(f"{k} {v:.1e}" for k, v in moves.items()))
    assert moves["scale_d"] < 1e-4 and moves["uniform"] < 1e-4


# ---- the LDS edge of t2p_match ---------------------------------------------------------------------------------------------------
def test_lds_edge_is_refused_on_the_host():
    lib = _lib.lib()
    p = C.c_void_p(64)
    w = _lib.MatchWeights()
    cross = (C.c_int32 * 2)(0, 1)
    w.n_layers, w.cross = 2, C.cast(cross, C.c_void_p)
    for (_, m, n, d, _) in FF.edge_shapes():
        up = (m + 1, m + 1) if m == n else (m + 1, n)
        assert FF.lds_floats(m, n, d) <= FF.LDS_FLOATS < FF.lds_floats(*up, d) and up[0] <= 63
        rc = lib.t2p_match(p, p, 2, up[0], up[1], d, C.byref(w), 20, 0.2, p, p, p, p, p, p, p, 1 << 40, None)
        assert rc == -3                                      # T2P_E_UNSUPPORTED
        msg = lib.t2p_last_error().decode()
        assert f"{up[0] + up[1]} tokens x D={d} need {4 * FF.lds_floats(*up, d)} B of LDS per sample (> 160 KiB)" in msg
