"""The training-mode text branch and the ranking losses, one entry point at a time through the C ABI, against the float64
statements of tests/text_train_ref.py (which tests/test_text_train_ref_host.py proves on the CPU):
  A  t2p_pairwise_ranking / t2p_hardest_ranking: |row_loss - ref64|, |best - ref64| <= 2 x bound per element on scores of
     L2-normalised rows, gradients / counts / positions exactly; everything bit for bit on the exact family with its planted
     hinge zeros, ties and rows without a positive hinge; NaN kept; B = 0, B = 32769 and NULL pointers; a second call bit-equal.
  B  t2p_lstm_cell_forward / _backward at any width: every element within 2 x bound, carried state / zero gates / passed-through
     gradients of finished rows bit for bit, nothing written past the last row; the gate functions measured in isolation.
  C  t2p_lstm_train_forward / _backward: gates, cs, hs and d_pre within 2 x the running bound; refusals; scratch is scratch.
  D  modules._LstmTrainFn at widths the loops refuse (6, 10), against nn.Embedding + pack_padded_sequence + nn.LSTM in float64 on the
     CPU: the output and all nine gradients per element.
Every output buffer is handed over prefilled with a sentinel and must be written everywhere.  Every test prints its largest
|got - ref64| / bound before it asserts (pytest -s shows them; docs/notebook.md records a run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = R.FACTOR_GPU
E_ARG, E_UNSUPPORTED = -1, -3           # T2P_E_ARG, T2P_E_UNSUPPORTED of include/t2p.h


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=_dev())


def _np(t):
    return t.detach().cpu().numpy()


def _sent(*shape):
    return torch.full(shape, float(R.SENTINEL), dtype=torch.float32, device=_dev())


def _sent_i(*shape):
    return torch.full(shape, int(R.SENTINEL_I), dtype=torch.int32, device=_dev())


def _abi():
    from text2pos_amd import _lib as L
    from text2pos_amd.ops import _ptr, _stream
    return L, _ptr, _stream(_dev())


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t == (int(R.SENTINEL_I) if t.dtype == torch.int32 else float(R.SENTINEL))).all()) for t in tensors)


# ---- A: ranking losses ------------------------------------------------------------------------------------------------------------------

def _pairwise(s, margin):
    L, p, st = _abi()
    b = s.shape[0]
    out = dict(row_loss=_sent(b), row_count=_sent(b), d_scores=_sent(b, b))
    L.check(L.lib().t2p_pairwise_ranking(p(s), b, float(margin), p(out["row_loss"]), p(out["d_scores"]), p(out["row_count"]), st),
            "t2p_pairwise_ranking")
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _hardest(s, margin):
    L, p, st = _abi()
    b = s.shape[0]
    out = dict(best=_sent(2 * b), where=_sent_i(2 * b), d_scores=_sent(b, b))
    L.check(L.lib().t2p_hardest_ranking(p(s), b, float(margin), p(out["best"]), p(out["where"]), p(out["d_scores"]), st),
            "t2p_hardest_ranking")
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _same_bits(x, y):
    return all(np.array_equal(np.ascontiguousarray(x[k]).view(np.int32), np.ascontiguousarray(y[k]).view(np.int32)) for k in x)


def _ranking_case(label, s, margin, exact):
    ref, href = R.rank_ref64(s, margin), R.hardest_ref64(s, margin)
    sd = _t(s)
    got, again = _pairwise(sd, margin), _pairwise(sd, margin)
    hgot, hagain = _hardest(sd, margin), _hardest(sd, margin)
    print(f"ratio pairwise row_loss {label}: {R.worst_ratio(got['row_loss'], ref['row_loss'], ref['b_row_loss']):.3f}; "
          f"hardest best: {R.worst_ratio(hgot['best'], href['best'], href['b_best']):.3f}")
    ok, why = R.rank_check(got, ref, exact, FACTOR)
    assert ok, (label, why)
    ok, why = R.hardest_check(hgot, href, exact, FACTOR)
    assert ok, (label, why)
    assert _same_bits(got, again) and _same_bits(hgot, hagain), (label, "a second call differs")
    return got, hgot, ref, href


@pytest.mark.parametrize("b", R.RANK_SIZES)
def test_ranking_losses_within_float64_bounds(b):
    """Scores of L2-normalised rows, margin float32(0.35): losses within 2 x bound per element; row_count, where and every entry of
    d_scores exactly (no hinge of the reference lies within two bounds of zero for these seeds: the host test asserts it)."""
    s = R.rank_scores(b)
    assert R.rank_ref64(s, R.MARGIN)["near"] == 0 and R.hardest_ref64(s, R.MARGIN)["near"] == 0
    _ranking_case(f"bounded B={b}", s, R.MARGIN, False)


@pytest.mark.parametrize("b", R.RANK_SIZES)
def test_ranking_losses_exact_family_bit_equal(b):
    """Scores in 2^-10 steps, margin 0.375: row_loss, row_count, best, where and d_scores equal the float64 result rounded once, bit
    for bit.  Planted: exact hinge zeros (gradient 0, not counted), equal maxima in one lane's stride and in different lanes
    (the lower index wins), a row and a column without a positive hinge (best 0, where -1, nothing added to d_scores)."""
    s = R.rank_exact_scores(b)
    got, hgot, ref, href = _ranking_case(f"exact B={b}", s, R.MARGIN_EXACT, True)
    if b >= 255:
        assert hgot["where"][R.X_ROW_NONE] == -1 and hgot["where"][b + R.X_COL_NONE] == -1
        assert hgot["best"][R.X_ROW_NONE] == 0.0 and hgot["best"][b + R.X_COL_NONE] == 0.0
        assert hgot["where"][R.X_ROW_TIE] == R.X_TIE[0] and hgot["where"][b + R.X_COL_TIE] == R.X_TIE[0]
        (i, j), (k, l) = R.X_ZERO_S, R.X_ZERO_IM
        assert got["d_scores"][i, j] == ref["d_scores"][i, j].astype(np.float32) and got["d_scores"][k, l] == ref["d_scores"][k, l].astype(np.float32)
    if b >= 257:
        assert hgot["where"][R.X_ROW_STRIDE] == 0 and hgot["where"][b + R.X_COL_STRIDE] == 0


@pytest.mark.parametrize("kind", R.RANK_NAN_KINDS)
@pytest.mark.parametrize("b", R.RANK_NAN_SIZES)
def test_ranking_losses_keep_nan(b, kind):
    """A NaN score makes row_loss / best NaN for every row or column whose terms include it, as torch.max(zeros, x) and relu + max
    do; rows and columns without it keep their exact values; every entry of d_scores is written."""
    s = R.rank_nan_scores(b, kind)
    got, hgot, ref, href = _ranking_case(f"nan {kind} B={b}", s, R.MARGIN_EXACT, True)
    assert np.isnan(ref["row_loss"]).any() and np.array_equal(np.isnan(got["row_loss"]), np.isnan(ref["row_loss"]))
    assert np.isnan(href["best"]).any() and np.array_equal(np.isnan(hgot["best"]), np.isnan(href["best"]))


@pytest.mark.parametrize("hardest", [False, True])
def test_ranking_loss_modules_keep_nan(hardest):
    """PairwiseRankingLoss / HardestRankingLoss on embeddings with one NaN row (a diverged embedding) return NaN, as the reference."""
    import text2pos_amd as t2p
    g = torch.Generator().manual_seed(3)
    im = torch.randn(9, 64, generator=g)
    s = 0.7 * im + 0.6 * torch.randn(9, 64, generator=g)
    crit = (t2p.HardestRankingLoss if hardest else t2p.PairwiseRankingLoss)(0.35)
    assert bool(torch.isfinite(crit(im.to(_dev()), s.to(_dev()))))
    im[4] = float("nan")
    assert bool(torch.isnan(crit(im.to(_dev()), s.to(_dev()))))


def test_ranking_arguments():
    """B = 0 returns 0 and writes nothing; B = 32769 and each NULL pointer return T2P_E_ARG with nothing launched."""
    L, p, st = _abi()
    lib = L.lib()
    s = _t(R.rank_exact_scores(2))
    rl, rc, ds, best, where = _sent(4), _sent(4), _sent(4, 4), _sent(8), _sent_i(8)
    assert lib.t2p_pairwise_ranking(p(s), 0, 0.375, p(rl), p(ds), p(rc), st) == 0
    assert lib.t2p_hardest_ranking(p(s), 0, 0.375, p(best), p(where), p(ds), st) == 0
    assert _untouched(rl, rc, ds, best, where)
    assert lib.t2p_pairwise_ranking(p(s), 32769, 0.375, p(rl), p(ds), p(rc), st) == E_ARG
    assert lib.t2p_hardest_ranking(p(s), 32769, 0.375, p(best), p(where), p(ds), st) == E_ARG
    args = [p(s), p(rl), p(ds), p(rc)]
    for i in range(4):
        a = list(args)
        a[i] = None
        assert lib.t2p_pairwise_ranking(a[0], 2, 0.375, a[1], a[2], a[3], st) == E_ARG, i
    args = [p(s), p(best), p(where), p(ds)]
    for i in range(4):
        a = list(args)
        a[i] = None
        assert lib.t2p_hardest_ranking(a[0], 2, 0.375, a[1], a[2], a[3], st) == E_ARG, i
    assert _untouched(rl, rc, ds, best, where)


# ---- B: the per-step kernels -----------------------------------------------------------------------------------------------------------

GUARD = 2


def _cell_forward(pre, table, tokens, lengths, step, reverse, c_prev, h_prev):
    L, p, st = _abi()
    b, d = c_prev.shape
    out = dict(gates=_sent(b + GUARD, 4 * d), c=_sent(b + GUARD, d), h=_sent(b + GUARD, d))
    ins = [_t(x) for x in (pre, table, tokens, lengths, c_prev, h_prev)]           # (kept alive until the kernel has run)
    L.check(L.lib().t2p_lstm_cell_forward(p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), b, tokens.shape[1], d, step, reverse, p(ins[4]),
                                          p(ins[5]), p(out["gates"]), p(out["c"]), p(out["h"]), st), "t2p_lstm_cell_forward")
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _cell_backward(dh_gemm, dh_carry_in, dc_in, gates, c_prev, c, lengths, step):
    L, p, st = _abi()
    b, d = c.shape
    out = dict(d_pre=_sent(b + GUARD, 4 * d), dc_out=_sent(b + GUARD, d), dh_carry_out=_sent(b + GUARD, d))
    ins = [None if x is None else _t(x) for x in (dh_gemm, dh_carry_in, dc_in, gates, c_prev, c, lengths)]
    L.check(L.lib().t2p_lstm_cell_backward(None if dh_gemm is None else p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), p(ins[5]),
                                           p(ins[6]), b, d, step, p(out["d_pre"]), p(out["dc_out"]), p(out["dh_carry_out"]), st),
            "t2p_lstm_cell_backward")
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("d", R.CELL_DIMS)
@pytest.mark.parametrize("b", R.CELL_BATCHES)
def test_lstm_cell_forward_within_float64_bounds(b, d):
    """Step 0, a middle step (rows past their end, token 0 inside a sentence) and step = max_len - 1, both directions: the reverse
    direction reads token len - 1 - step, the forward one token step; finished rows carry c and h bit for bit and store exact
    zeros in all four gate slices; every element written, none past B rows."""
    p = R.cell_inputs(b, d)
    worst = 0.0
    for step, rev in R.cell_steps():
        a = (p["pre"], p["table"], p["tokens"], p["lengths"], step, rev, p["c_prev"], p["h_prev"])
        ref = R.cell_fwd_ref64(*a)
        got = _cell_forward(*a)
        worst = max([worst] + [R.worst_ratio(got[k][:b], ref[k], ref["b_" + k]) for k in ("gates", "c", "h")])
        ok, why = R.cell_fwd_check(got, ref, FACTOR)
        assert ok, (b, d, step, rev, why, worst)
        done = ~ref["live"]
        assert np.array_equal(_bits(got["c"][:b][done]), _bits(p["c_prev"][done])) and np.array_equal(_bits(got["h"][:b][done]), _bits(p["h_prev"][done]))
        assert not _bits(got["gates"][:b][done]).any()
    print(f"ratio lstm_cell_forward B={b} D={d}: {worst:.3f}")


@pytest.mark.parametrize("d", R.CELL_DIMS)
@pytest.mark.parametrize("b", R.CELL_BATCHES)
def test_lstm_cell_backward_within_float64_bounds(b, d):
    """With and without dh_gemm (NULL = the last step): finished rows have d_pre exactly 0, dc_out == dc_in and dh_carry_out ==
    fl(dh_gemm + dh_carry_in) bit for bit; live rows have dh_carry_out exactly 0; every element written, none past B rows."""
    p = R.cell_inputs(b, d)
    worst = 0.0
    for step in (0, 1, R.CELL_T - 1):
        for dh_gemm in (p["dh_gemm"], None):
            a = (dh_gemm, p["dh_carry_in"], p["dc_in"], p["gates"], p["c_prev"], p["c"], p["lengths"], step)
            ref = R.cell_bwd_ref64(*a)
            got = _cell_backward(*a)
            worst = max([worst] + [R.worst_ratio(got[k][:b], ref[k], ref["b_" + k]) for k in ("d_pre", "dc_out", "dh_carry_out")])
            ok, why = R.cell_bwd_check(got, ref, FACTOR)
            assert ok, (b, d, step, dh_gemm is None, why, worst)
            live = ref["live"]
            dh = p["dh_carry_in"] if dh_gemm is None else (dh_gemm + p["dh_carry_in"]).astype(np.float32)
            assert not _bits(got["d_pre"][:b][~live]).any() and not _bits(got["dh_carry_out"][:b][live]).any()
            assert np.array_equal(_bits(got["dc_out"][:b][~live]), _bits(p["dc_in"][~live]))
            assert np.array_equal(_bits(got["dh_carry_out"][:b][~live]), _bits(dh[~live]))
    print(f"ratio lstm_cell_backward B={b} D={d}: {worst:.3f}")


def test_gate_functions_in_isolation():
    """pre = 0 and a table whose rows sweep [-30, 30] (dense near 0, +-0): the gates output of t2p_lstm_cell_forward is then
    1 / (1 + expf(-x)) in slices i, f, o and tanhf(x) in slice g.  Both stay within EPS_GATE of float64 (absolute)."""
    x = R.gate_sweep()
    v, d = x.shape[0], R.GATE_SWEEP_D
    z = np.zeros
    got = _cell_forward(z((v, 4 * d), np.float32), x, np.arange(v, dtype=np.int32)[:, None], np.ones(v, np.int32), 0, 0,
                        z((v, d), np.float32), z((v, d), np.float32))["gates"][:v].astype(np.float64)
    err = np.abs(got - R.gate_functions64(x))
    e_tanh = err[:, 2 * d: 3 * d].max()
    e_sig = max(err[:, : 2 * d].max(), err[:, 3 * d:].max())
    print(f"gate functions of the training kernels: max |sigmoid - float64| = {e_sig:.3e}, max |tanh - float64| = {e_tanh:.3e} (EPS_GATE {R.EPS_GATE:g})")
    assert e_sig <= R.EPS_GATE and e_tanh <= R.EPS_GATE, (e_sig, e_tanh)


# ---- C: the in-library loops -----------------------------------------------------------------------------------------------------------

def _train_forward(inp, reverse):
    L, p, st = _abi()
    b, d, t = inp["b"], inp["d"], inp["t"]
    i = 1 if reverse else 0
    gates, cs, hs, pre = _sent(t, b, 4 * d), _sent(t + 1, b, d), _sent(t + 1, b, d), _sent(b, 4 * d)
    cs[0], hs[0] = _t(inp["c0"]), _t(inp["h0"])
    ins = [_t(x) for x in (inp["table"][i], inp["w_hh_k"][i], inp["tokens"], inp["lengths"])]
    rc = L.lib().t2p_lstm_train_forward(p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), b, t, d, int(reverse), p(gates), p(cs), p(hs), p(pre), st)
    torch.cuda.synchronize()
    return rc, dict(gates=_np(gates), cs=_np(cs), hs=_np(hs))


def _train_backward(inp, bin_, ws_fill):
    L, p, st = _abi()
    b, d, t = inp["b"], inp["d"], inp["t"]
    d_pre = _sent(t, b, 4 * d)
    ws = torch.full((5, b, d), ws_fill, dtype=torch.float32, device=_dev())
    ins = [_t(x) for x in (inp["dh_last"], bin_["w_hh_t"], bin_["gates"], bin_["cs"], inp["lengths"])]
    rc = L.lib().t2p_lstm_train_backward(p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), b, t, d, p(d_pre), p(ws), st)
    torch.cuda.synchronize()
    return rc, _np(d_pre)


@pytest.mark.parametrize("case", range(len(R.LOOP_CASES)))
def test_lstm_train_loops_within_float64_bounds(case):
    """Forward: gates, cs, hs of both directions against the float64 recurrence with its running bound (slice 0 of cs / hs left as
    given, once non-zero).  Backward, kernel by kernel: d_pre from exact fp32 gates / cs (the float64 forward, rounded) against
    the float64 backward recurrence; ws is scratch: prefilled with NaN, the second call gives the same bits."""
    for rev in (0, 1):
        inp, fwd, bin_, bwd = R.loop_reference(case, rev)
        rc, got = _train_forward(inp, rev)
        assert rc == 0
        rf = max(R.worst_ratio(got[k], fwd[k], fwd["b_" + k]) for k in ("gates", "cs", "hs"))
        ok, why = R.loop_fwd_check(got, fwd, FACTOR)
        assert ok, (R.LOOP_CASES[case], rev, why)
        assert np.array_equal(_bits(got["cs"][0]), _bits(inp["c0"])) and np.array_equal(_bits(got["hs"][0]), _bits(inp["h0"]))
        rc, d_pre = _train_backward(inp, bin_, float(R.SENTINEL))
        assert rc == 0
        rb = R.worst_ratio(d_pre, bwd["d_pre"], bwd["b_d_pre"])
        print(f"ratio lstm_train_forward {R.LOOP_CASES[case]} reverse={rev}: {rf:.3f}; lstm_train_backward: {rb:.3f}")
        ok, why = R.loop_bwd_check(dict(d_pre=d_pre), bwd, FACTOR)
        assert ok, (R.LOOP_CASES[case], rev, why)
        rc, again = _train_backward(inp, bin_, float("nan"))
        assert rc == 0 and np.array_equal(_bits(again), _bits(d_pre)), "d_pre depends on what the scratch held"


def test_lstm_train_loops_refusals():
    """embed_dim = 6 through both loops: T2P_E_UNSUPPORTED, outputs untouched.  batch = 0: returns 0."""
    L, p, st = _abi()
    lib = L.lib()
    b, d, t, v = 5, 6, 3, 4
    table, w, w_t = _t(np.zeros((v, 4 * d), np.float32)), _t(np.zeros((d, 4 * d), np.float32)), _t(np.zeros((4 * d, d), np.float32))
    tok, ln = _t(np.ones((b, t), np.int32)), _t(np.full(b, t, np.int32))
    gates, cs, hs, pre, d_pre, ws = _sent(t, b, 4 * d), _sent(t + 1, b, d), _sent(t + 1, b, d), _sent(b, 4 * d), _sent(t, b, 4 * d), _sent(5, b, d)
    dh = _t(np.zeros((b, d), np.float32))
    assert lib.t2p_lstm_train_forward(p(table), p(w), p(tok), p(ln), b, t, d, 0, p(gates), p(cs), p(hs), p(pre), st) == E_UNSUPPORTED
    assert lib.t2p_lstm_train_backward(p(dh), p(w_t), p(gates), p(cs), p(ln), b, t, d, p(d_pre), p(ws), st) == E_UNSUPPORTED
    assert _untouched(gates, cs, hs, pre, d_pre, ws)
    assert lib.t2p_lstm_train_forward(p(table), p(w), p(tok), p(ln), 0, t, 8, 0, p(gates), p(cs), p(hs), p(pre), st) == 0
    assert lib.t2p_lstm_train_backward(p(dh), p(w_t), p(gates), p(cs), p(ln), 0, t, 8, p(d_pre), p(ws), st) == 0
    assert _untouched(gates, cs, hs, pre, d_pre, ws)


# ---- D: the step-by-step path of _LstmTrainFn ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _torch_reference(d):
    p = R.fallback_inputs(d)
    emb = torch.nn.Embedding(R.FALLBACK_V, d, padding_idx=0).double()
    lstm = torch.nn.LSTM(input_size=d, hidden_size=d, bidirectional=True, num_layers=1).double()
    names = [n + suf for suf in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(p["emb"].astype(np.float64)))
        for j, n in enumerate(names):
            getattr(lstm, n).copy_(torch.from_numpy(p[("w_ih", "w_hh", "b_ih", "b_hh")[j % 4]][j // 4].astype(np.float64)))
    x = emb(torch.from_numpy(p["tokens"].astype(np.int64)))
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.from_numpy(p["lengths"].astype(np.int64)), batch_first=True, enforce_sorted=False)
    _, (h, _c) = lstm(packed)
    want = torch.mean(h, dim=0)
    (want * torch.from_numpy(p["coef"].astype(np.float64))).sum().backward()
    return want.detach().numpy(), [emb.weight.grad.numpy()] + [getattr(lstm, n).grad.numpy() for n in names]


@pytest.mark.parametrize("d", R.FALLBACK_DIMS)
def test_lstm_train_fallback_matches_float64_autograd(d):
    """Widths that are no multiple of 4 take the per-step calls (t2p_lstm_cell_forward / _backward from Python, products through
    ops.matmul): the mean of the two final hidden states and all nine gradients within 2 x the composed per-element bounds of the
    float64 LSTM of torch on the CPU."""
    from text2pos_amd import modules as M, ops
    assert not ops.lstm_train_loops_supported(d)
    p = R.fallback_inputs(d)
    ref = R.fallback_ref64(p)
    want, want_grads = _torch_reference(d)
    assert np.abs(want - ref["out"]).max() <= 1e-13 and all(np.abs(a - b).max() <= 1e-12 for a, b in zip(want_grads, ref["grads"]))
    prm = [p["emb"]] + [p[k][i] for i in range(2) for k in ("w_ih", "w_hh", "b_ih", "b_hh")]
    prm_d = [_t(q).requires_grad_(True) for q in prm]
    got = M._LstmTrainFn.apply(_t(p["tokens"]), _t(p["lengths"]), *prm_d)
    (got * _t(p["coef"])).sum().backward()
    torch.cuda.synchronize()
    ratios = {"out": R.worst_ratio(_np(got), want, ref["b_out"])}
    ratios.update({n: R.worst_ratio(_np(q.grad), w, bnd) for n, q, w, bnd in zip(R.GRAD_NAMES, prm_d, want_grads, ref["b_grads"])})
    print(f"ratio _LstmTrainFn fallback D={d}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert R.within(_np(got), want, ref["b_out"], FACTOR), ratios
    for n, q, w, bnd in zip(R.GRAD_NAMES, prm_d, want_grads, ref["b_grads"]):
        assert R.within(_np(q.grad), w, bnd, FACTOR), (n, ratios)
    assert not _np(prm_d[0].grad)[0].any()          # nn.Embedding(padding_idx=0)
