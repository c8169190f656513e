"""CPU only: proves the yardstick of tests/text_train_ref.py before tests/test_gpu_text_train.py relies on it.
  * every *_ref64 is what torch's float64 autograd gives for the reference's statements (training/losses.py:139-164, :173-200;
    nn.Embedding + pack_padded_sequence + nn.LSTM(...).double()) on inputs without ties;
  * every fp32 emulation of a kernel's documented order stays within 1 x bound (bit-equal on the exact family) on every GPU case;
  * every `wrong=` variant is rejected, by the same check function the GPU test applies, on at least one case;
  * the caps of the loops hold, the near-hinge share of the bounded ranking cases is zero for the chosen seeds, the exact
    family's headroom holds and its plants are there."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_ref as LR  # noqa: E402
import text_train_ref as R  # noqa: E402

F64 = torch.double


def _td(a):
    return torch.from_numpy(np.asarray(a, np.float64).copy())


# ---- A ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", R.RANK_SIZES[1:])
def test_ranking_refs_are_torch_float64_autograd(b):
    s = R.rank_scores(b)
    m = float(R.MARGIN)
    eye = torch.eye(b, dtype=torch.bool)
    x = _td(s).requires_grad_(True)
    diag = x.diag()
    cost_s = torch.max(torch.zeros(b, b, dtype=F64), (m - diag).expand_as(x) + x).masked_fill(eye, 0)
    cost_im = torch.max(torch.zeros(b, b, dtype=F64), (m - diag).expand_as(x).transpose(1, 0) + x).masked_fill(eye, 0)
    ((cost_s.sum() + cost_im.sum()) / b).backward()
    ref = R.rank_ref64(s, R.MARGIN)
    assert np.abs((cost_s.sum(1) + cost_im.sum(1)).detach().numpy() - ref["row_loss"]).max() <= 1e-12 * b
    assert np.abs(x.grad.numpy() - ref["d_scores"]).max() <= 1e-15
    assert np.array_equal(ref["row_count"], (cost_im.detach().numpy() > 0).sum(1))
    y = _td(s).requires_grad_(True)
    ci = torch.relu((m + y - y.diag().view(b, 1)).masked_fill(eye, 0)).max(dim=1)
    cc = torch.relu((m + y.transpose(1, 0) - y.diag().view(b, 1)).masked_fill(eye, 0)).max(dim=1)
    (ci.values.mean() + cc.values.mean()).backward()
    href = R.hardest_ref64(s, R.MARGIN)
    best = torch.cat([ci.values, cc.values]).detach().numpy()
    idx = torch.cat([ci.indices, cc.indices]).numpy()
    assert np.abs(best - href["best"]).max() <= 1e-15
    assert np.array_equal(np.where(best > 0, idx, -1), href["where"])
    assert np.abs(y.grad.numpy() - href["d_scores"]).max() <= 1e-15


def test_nan_follows_torch():
    """torch.max(zeros, x) and relu + max keep a NaN: the refs mark the same rows and columns."""
    for b in R.RANK_NAN_SIZES:
        for kind in R.RANK_NAN_KINDS:
            s = R.rank_nan_scores(b, kind)
            m = float(R.MARGIN_EXACT)
            x = _td(s)
            eye = torch.eye(b, dtype=torch.bool)
            cs = torch.max(torch.zeros(b, b, dtype=F64), (m - x.diag()).expand_as(x) + x).masked_fill(eye, 0)
            ci = torch.max(torch.zeros(b, b, dtype=F64), (m - x.diag()).expand_as(x).transpose(1, 0) + x).masked_fill(eye, 0)
            ref, href = R.rank_ref64(s, R.MARGIN_EXACT), R.hardest_ref64(s, R.MARGIN_EXACT)
            assert np.array_equal(np.isnan((cs.sum(1) + ci.sum(1)).numpy()), np.isnan(ref["row_loss"])) and np.isnan(ref["row_loss"]).any()
            hi = torch.relu((m + x - x.diag().view(b, 1)).masked_fill(eye, 0)).max(dim=1).values
            hc = torch.relu((m + x.transpose(1, 0) - x.diag().view(b, 1)).masked_fill(eye, 0)).max(dim=1).values
            assert np.array_equal(np.isnan(torch.cat([hi, hc]).numpy()), np.isnan(href["best"])) and np.isnan(href["best"]).any()


def _rank_cases():
    for b in R.RANK_SIZES:
        yield f"bounded B={b}", R.rank_scores(b), R.MARGIN, False
        yield f"exact B={b}", R.rank_exact_scores(b), R.MARGIN_EXACT, True
    for b in R.RANK_NAN_SIZES:
        for kind in R.RANK_NAN_KINDS:
            yield f"nan {kind} B={b}", R.rank_nan_scores(b, kind), R.MARGIN_EXACT, True


def test_ranking_emulations_pass_and_wrong_variants_fail():
    rejected = {("rank", w): [] for w in R.RANK_WRONG}
    rejected.update({("hardest", w): [] for w in R.HARDEST_WRONG})
    for label, s, m, exact in _rank_cases():
        ref, href = R.rank_ref64(s, m), R.hardest_ref64(s, m)
        ok, why = R.rank_check(R.rank_emul(s, m), ref, exact, 1.0)
        assert ok, (label, why)
        ok, why = R.hardest_check(R.hardest_emul(s, m), href, exact, 1.0)
        assert ok, (label, why)
        for w in R.RANK_WRONG:
            if not R.rank_check(R.rank_emul(s, m, w), ref, exact, R.FACTOR_GPU)[0]:
                rejected[("rank", w)].append(label)
        for w in R.HARDEST_WRONG:
            if not R.hardest_check(R.hardest_emul(s, m, w), href, exact, R.FACTOR_GPU)[0]:
                rejected[("hardest", w)].append(label)
    assert all(rejected.values()), {k: v for k, v in rejected.items() if not v}
    # an output left at its prefill is refused as well
    s = R.rank_exact_scores(255)
    got = R.rank_emul(s, R.MARGIN_EXACT)
    got["d_scores"][7, 9] = R.SENTINEL
    assert not R.rank_check(got, R.rank_ref64(s, R.MARGIN_EXACT), True, R.FACTOR_GPU)[0]


def test_near_hinge_share_is_zero():
    """Exact comparison of gradients, counts and positions means something only if no hinge of the float64 reference lies within
    FACTOR_GPU bounds of zero (or of the runner-up): none does, for every (B, seed) the GPU test uses."""
    for b in R.RANK_SIZES:
        s = R.rank_scores(b)
        assert R.rank_ref64(s, R.MARGIN)["near"] == 0 and R.hardest_ref64(s, R.MARGIN)["near"] == 0, b
        if b >= 255:                          # and the family does exercise the sums: many hinges above 0 per row
            assert (R.rank_ref64(s, R.MARGIN)["row_count"] > 8).mean() > 0.9


def test_exact_family_headroom_plants_and_reciprocal():
    for b in R.RANK_SIZES:
        assert R.exact_headroom(b) < 2.0 ** 24
        s = R.rank_exact_scores(b)
        assert np.array_equal(s.astype(np.float64) * 1024, np.round(s.astype(np.float64) * 1024)) and np.abs(s).max() <= 1.0
        # count fl(1 / B) and the correctly rounded -(count) / B are the float64 values rounded once
        inv = R.F32(1.0) / R.F32(b)
        cnt = np.arange(0, 2 * b + 1)
        assert np.array_equal(np.arange(3).astype(R.F32) * inv, (np.arange(3) / b).astype(R.F32))
        assert np.array_equal(-cnt.astype(R.F32) / R.F32(b), (-cnt / b).astype(R.F32))
        if b < 255:
            continue
        m = float(R.MARGIN_EXACT)
        s64 = s.astype(np.float64)
        href = R.hardest_ref64(s, R.MARGIN_EXACT)
        assert href["where"][R.X_ROW_NONE] == -1 and href["where"][b + R.X_COL_NONE] == -1
        assert href["best"][R.X_ROW_NONE] == 0.0 and href["best"][b + R.X_COL_NONE] == 0.0
        assert m + s64[R.X_ROW_NONE, 7] - s64[R.X_ROW_NONE, R.X_ROW_NONE] == 0.0          # an exact hinge that must not win
        assert href["where"][R.X_ROW_TIE] == R.X_TIE[0] and href["where"][b + R.X_COL_TIE] == R.X_TIE[0]
        assert s[R.X_ROW_TIE, R.X_TIE[0]] == s[R.X_ROW_TIE, R.X_TIE[1]] and s[R.X_TIE[0], R.X_COL_TIE] == s[R.X_TIE[1], R.X_COL_TIE]
        if b >= 257:
            assert href["where"][R.X_ROW_STRIDE] == 0 and href["where"][b + R.X_COL_STRIDE] == 0
            assert s[R.X_ROW_STRIDE, 0] == s[R.X_ROW_STRIDE, 256] and s[0, R.X_COL_STRIDE] == s[256, R.X_COL_STRIDE]
        (i, j), (k, l) = R.X_ZERO_S, R.X_ZERO_IM
        ref = R.rank_ref64(s, R.MARGIN_EXACT)
        assert (m - s64[j, j]) + s64[i, j] == 0.0 and (m - s64[k, k]) + s64[k, l] == 0.0
        assert ref["d_scores"][i, j] * b in (0.0, 1.0) and ref["d_scores"][k, l] * b in (0.0, 1.0)


# ---- B, C, D ---------------------------------------------------------------------------------------------------------------------------

def test_cell_refs_are_torch_float64_autograd():
    p = R.cell_inputs(5, 6)
    d = 6
    for step, rev in R.cell_steps():
        ref = R.cell_fwd_ref64(p["pre"], p["table"], p["tokens"], p["lengths"], step, rev, p["c_prev"], p["h_prev"])
        ln = p["lengths"]
        col = np.clip(ln - 1 - step, 0, None) if rev else np.full(len(ln), step)
        z = (_td(p["pre"]) + _td(p["table"])[torch.from_numpy(p["tokens"][np.arange(5), col].astype(np.int64))]).requires_grad_(True)
        c_prev = _td(p["c_prev"]).requires_grad_(True)
        i, f, g, o = torch.sigmoid(z[:, :d]), torch.sigmoid(z[:, d: 2 * d]), torch.tanh(z[:, 2 * d: 3 * d]), torch.sigmoid(z[:, 3 * d:])
        c = f * c_prev + i * g
        h = o * torch.tanh(c)
        live = ref["live"]
        assert live.any() and (step == 0 or not live.all())
        assert np.abs(torch.cat([i, f, g, o], 1).detach().numpy() - ref["gates"])[live].max() <= 1e-15
        assert np.abs(c.detach().numpy() - ref["c"])[live].max() <= 1e-15 and np.abs(h.detach().numpy() - ref["h"])[live].max() <= 1e-15
        assert np.array_equal(ref["c"][~live], p["c_prev"][~live]) and np.array_equal(ref["h"][~live], p["h_prev"][~live])
        assert not ref["gates"][~live].any()
        dh = p["dh_gemm"].astype(np.float64) + p["dh_carry_in"].astype(np.float64)
        ((h * _td(dh)).sum() + (c * _td(p["dc_in"])).sum()).backward()
        bref = R.cell_bwd_ref64(p["dh_gemm"], p["dh_carry_in"], p["dc_in"], ref["gates"], p["c_prev"], ref["c"], ln, step)
        assert np.abs(z.grad.numpy() - bref["d_pre"])[live].max() <= 1e-14
        assert np.abs(c_prev.grad.numpy() - bref["dc_out"])[live].max() <= 1e-14
        assert not bref["d_pre"][~live].any() and not bref["dh_carry_out"][live].any()
        assert np.array_equal(bref["dc_out"][~live], p["dc_in"][~live].astype(np.float64)) and np.array_equal(bref["dh_carry_out"][~live], dh[~live])


def _torch_lstm(base, d, v):
    emb = torch.nn.Embedding(v, d, padding_idx=0).double()
    lstm = torch.nn.LSTM(input_size=d, hidden_size=d, bidirectional=True, num_layers=1).double()
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    with torch.no_grad():
        emb.weight.copy_(_td(base["emb"]))
        for i, suf in enumerate(("", "_reverse")):
            for n, k in zip(names, ("w_ih", "w_hh", "b_ih", "b_hh")):
                getattr(lstm, n + suf).copy_(_td(base[k][i]))
    return emb, lstm, [n + suf for suf in ("", "_reverse") for n in names]


@pytest.mark.parametrize("case", [1, 2, 4, 9])
def test_loop_refs_are_torch_float64_lstm(case):
    """The final hidden state of each direction against nn.LSTM(...).double() on the packed sequence; the backward recurrence
    through the two gradients that are plain sums of d_pre: weight_hh = sum_s d_pre[s]^T h[s], bias = sum_s d_pre[s]."""
    b, d, t = R.LOOP_CASES[case][:3]
    inp = R.loop_inputs(*R.LOOP_CASES[case])
    base = inp["base"]
    emb, lstm, names = _torch_lstm(base, d, R.LOOP_VOCAB)
    ln = inp["lengths"]
    tok = inp["tokens"].copy()
    x = emb(torch.from_numpy(tok.astype(np.int64)))
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.from_numpy(ln.astype(np.int64)), batch_first=True, enforce_sorted=False)
    h0 = torch.stack([_td(inp["h0"])] * 2)
    c0 = torch.stack([_td(inp["c0"])] * 2)
    _, (h, _c) = lstm(packed, (h0, c0))
    (h * _td(inp["dh_last"])[None]).sum().backward()
    for i in range(2):
        fwd = R.train_fwd_ref64(inp["table"][i], inp["w_hh_k"][i], inp["tokens"], ln, i == 1, inp["c0"], inp["h0"])
        assert np.abs(h[i].detach().numpy() - fwd["hs"][t]).max() <= 1e-13
        bwd = R.train_bwd_ref64(inp["dh_last"], inp["w_hh_k"][i].T, fwd["gates"], fwd["cs"], ln)
        flat = bwd["d_pre"].reshape(t * b, 4 * d)
        g_hh = getattr(lstm, names[4 * i + 1]).grad.numpy()
        g_b = getattr(lstm, names[4 * i + 2]).grad.numpy()
        assert np.abs(flat.T @ fwd["hs"][:t].reshape(t * b, d) - g_hh).max() <= 1e-12 * max(1.0, np.abs(g_hh).max())
        assert np.abs(flat.sum(0) - g_b).max() <= 1e-12 * max(1.0, np.abs(g_b).max())


@pytest.mark.parametrize("d", R.FALLBACK_DIMS)
def test_fallback_ref_is_torch_float64_autograd(d):
    p = R.fallback_inputs(d)
    ref = R.fallback_ref64(p)
    emb, lstm, names = _torch_lstm(p, d, R.FALLBACK_V)
    x = emb(torch.from_numpy(p["tokens"].astype(np.int64)))
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.from_numpy(p["lengths"].astype(np.int64)), batch_first=True, enforce_sorted=False)
    _, (h, _c) = lstm(packed)
    want = torch.mean(h, dim=0)
    (want * _td(p["coef"])).sum().backward()
    assert np.abs(want.detach().numpy() - ref["out"]).max() <= 1e-14
    for name, g, r, bound in zip(R.GRAD_NAMES, [emb.weight.grad] + [getattr(lstm, n).grad for n in names], ref["grads"], ref["b_grads"]):
        assert np.abs(g.numpy() - r).max() <= 1e-13, name
        assert bound.max() <= 1e-4, (name, bound.max())      # per element what the autograd test of the loops allows per tensor
    assert ref["b_out"].max() <= 1e-5
    assert (p["lengths"] < R.FALLBACK_T).any() and (p["tokens"][0, :p["lengths"][0]] == 0).any()


def test_loop_tables_are_exact():
    for case in R.LOOP_CASES:
        assert LR.table_is_exact(R.loop_inputs(*case)["base"]), case


def test_lstm_emulations_pass_caps_hold_and_wrong_variants_fail():
    rejected = {w: [] for w in R.LSTM_WRONG}
    fwd_wrong = ("finished_row_updated", "reverse_from_T", "gates_not_zeroed_past_end", "g_and_o_swapped")
    bwd_wrong = ("carry_dropped", "dc_not_carried", "tanh_of_c_prev", "forget_grad_uses_c")
    for b in R.CELL_BATCHES:
        for d in R.CELL_DIMS:
            p = R.cell_inputs(b, d)
            for step, rev in R.cell_steps():
                a = (p["pre"], p["table"], p["tokens"], p["lengths"], step, rev, p["c_prev"], p["h_prev"])
                ref = R.cell_fwd_ref64(*a)
                ok, why = R.cell_fwd_check(R.cell_fwd_emul(*a), ref, 1.0)
                assert ok, (b, d, step, rev, why)
                for w in fwd_wrong:
                    if not R.cell_fwd_check(R.cell_fwd_emul(*a, wrong=w), ref, R.FACTOR_GPU)[0]:
                        rejected[w].append(("cell", b, d, step, rev))
            for step in (0, 1, R.CELL_T - 1):
                for dh_gemm in (p["dh_gemm"], None):
                    a = (dh_gemm, p["dh_carry_in"], p["dc_in"], p["gates"], p["c_prev"], p["c"], p["lengths"], step)
                    ref = R.cell_bwd_ref64(*a)
                    ok, why = R.cell_bwd_check(R.cell_bwd_emul(*a), ref, 1.0)
                    assert ok, (b, d, step, why)
                    for w in bwd_wrong:
                        if not R.cell_bwd_check(R.cell_bwd_emul(*a, wrong=w), ref, R.FACTOR_GPU)[0]:
                            rejected[w].append(("cell", b, d, step))
    for case in range(len(R.LOOP_CASES)):
        for rev in (0, 1):
            inp, fwd, bin_, bwd = R.loop_reference(case, rev)
            assert max(fwd["b_gates"].max(), fwd["b_cs"].max(), fwd["b_hs"].max()) <= R.CAP, (case, rev)
            assert bwd["b_d_pre"].max() <= 5e-5 * max(1.0, np.abs(bwd["d_pre"]).max()), (case, rev)
            a = (inp["table"][rev], inp["w_hh_k"][rev], inp["tokens"], inp["lengths"], rev, inp["c0"], inp["h0"])
            ok, why = R.loop_fwd_check(R.train_fwd_emul(*a), fwd, 1.0)
            assert ok, (case, rev, why)
            ba = (inp["dh_last"], bin_["w_hh_t"], bin_["gates"], bin_["cs"], inp["lengths"])
            ok, why = R.loop_bwd_check(R.train_bwd_emul(*ba), bwd, 1.0)
            assert ok, (case, rev, why)
            for w in fwd_wrong + ("initial_state_overwritten",):
                if not R.loop_fwd_check(R.train_fwd_emul(*a, wrong=w), fwd, R.FACTOR_GPU)[0]:
                    rejected[w].append(("loop", case, rev))
            for w in bwd_wrong + ("dh_gemm_read_at_last_step",):
                if not R.loop_bwd_check(R.train_bwd_emul(*ba, wrong=w), bwd, R.FACTOR_GPU)[0]:
                    rejected[w].append(("loop", case, rev))
            # scratch that holds numbers instead of NaN: the stale-slot read still shows against the bound
            if R.LOOP_CASES[case][2] > 1 and R.loop_bwd_check(R.train_bwd_emul(*ba, wrong="dh_gemm_read_at_last_step", ws_fill=1.0), bwd, R.FACTOR_GPU)[0]:
                raise AssertionError(("a stale dh_gemm slot of ones passed", case, rev))
    assert all(rejected.values()), [w for w, v in rejected.items() if not v]


def test_gate_sweep_covers_what_it_says():
    x = R.gate_sweep()
    assert x.shape[1] == 4 * R.GATE_SWEEP_D and x.min() == -30.0 and x.max() == 30.0
    assert np.signbit(x).any() and (x == 0).sum() >= 2 and (np.abs(x[x != 0]).min() < 1e-12)
    f, d = R.gate_functions64(x), R.GATE_SWEEP_D
    tanh_slice = np.zeros(x.shape, bool)
    tanh_slice[:, 2 * d: 3 * d] = True
    assert np.all(f[(x == 0) & ~tanh_slice] == 0.5) and np.all(f[(x == 0) & tanh_slice] == 0.0)
    assert np.array_equal(f[tanh_slice], np.tanh(x.astype(np.float64))[tanh_slice]) and f[~tanh_slice].min() > 0.0 and f.max() <= 1.0
