"""The persistent biLSTM of the inference text branch (csrc/lstm.hip: k_bilstm and k_bilstm_x3 at 128, 256 and 384 units) through
packing.pack_text_weights, ops.make_text_weights and ops.encode_text on a bare LanguageEncoder, against the float64 statement and
the derived bounds of tests/lstm_ref.py:
  * |raw - ref64| <= 2 x bound element by element, no element exempt, and the normalised rows within the propagated bound;
  * the gate functions alone (T = 1) over 4,109 exact pre-activations in [-104, 104];
  * every width in both of its roles (native and zero-padded: the padded columns exactly 0), four multiples of the reference-like
    W_hh that give three values of w_hh_scale, the permuted family;
  * the second and third pass of k_bilstm_x3's group loop (B = 32 x CUs / 2 + 1 and 64 x CUs / 2 + 1), float64 bounds on a row
    subset and, bit for bit, every checked row equal to the same row in a batch of its own group and in a batch of one;
  * the layout contracts (padding ids are never read, the row pitch of tokens is the buffer's T whatever the longest length), T = 162, and the C ABI's workspace contract.
Every test prints its largest |got - ref64| / bound before it asserts (pytest -s shows them; docs/notebook.md records a run)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = R.FACTOR_GPU
F32 = np.float32
_PACKS = {}
_REFS = {}


def _dev():
    return torch.device("cuda:0")


def _per_dir():
    return max(1, torch.cuda.get_device_properties(0).multi_processor_count // 2)


def _encoder(inp):
    """A bare LanguageEncoder (CPU) carrying the case's parameters."""
    from text2pos_amd.modules import LanguageEncoder
    lang = LanguageEncoder([f"w{i}" for i in range(1, inp["vocab"])], inp["d"], bi_dir=True)
    with torch.no_grad():
        lang.word_embedding.weight.copy_(torch.from_numpy(np.array(inp["emb"])))
        for i, suffix in enumerate(("", "_reverse")):
            for name, key in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
                getattr(lang.lstm, name + suffix).copy_(torch.from_numpy(np.array(inp[key][i])))
    return lang.eval()


def _pack(inp, precision):
    """(tensors, TextWeights, kernel width) of the case, packed once."""
    from text2pos_amd import ops, packing
    key = (id(inp), precision)
    if key not in _PACKS:
        dk = packing.kernel_embed_dim(inp["d"])
        assert dk == R.kernel_dim(inp["d"])
        t = packing.pack_text_weights(_encoder(inp), _dev(), x3=precision == "f16x3", pad_to=dk)
        if precision == "f16x3":
            assert t["w_hh_scale"] == R.w_hh_scale(inp)
        w = ops.make_text_weights(t["embedding"], t["w_ih"], t["w_hh"], t["bias"], t.get("w_hh_x3"), t.get("w_hh_scale", 0.0))
        _PACKS[key] = (inp, t, w, dk)
    return _PACKS[key][1:]


def _encode(inp, precision, tokens=None, lengths=None):
    """(out, raw) [B][kernel width] of ops.encode_text, as NumPy."""
    from text2pos_amd import ops
    _, w, dk = _pack(inp, precision)
    tok = torch.from_numpy(np.array(inp["tokens"] if tokens is None else tokens, np.int32)).to(_dev())
    ln = torch.from_numpy(np.array(inp["lengths"] if lengths is None else lengths, np.int32)).to(_dev())
    out, raw = ops.encode_text(tok, ln, w, inp["vocab"], dk, want_raw=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), raw.cpu().numpy()


def _reference(inp, precision, rows=None):
    """(ref64 [n][d], bound dict) of the case, computed once and shared."""
    key = (id(inp), precision, None if rows is None else rows.tobytes())
    if key not in _REFS:
        rkey = (id(inp), "ref", key[2])
        if rkey not in _REFS:
            _REFS[rkey] = R.bilstm_ref64(inp, rows)
            _REFS[rkey].setflags(write=False)
        _REFS[key] = (_REFS[rkey], R.bilstm_bound(inp, precision, rows))
    return _REFS[key]


def _check_bounded(label, inp, precision, out, raw, rows=None):
    """raw and out (the checked rows) against float64 within FACTOR x bound; padded columns exactly 0.  Returns the worst ratio."""
    d = inp["d"]
    ref, bound = _reference(inp, precision, rows)
    ratio = R.worst_ratio(raw[:, :d], ref, bound["raw"][:, :d])
    ratio_n = R.worst_ratio(out[:, :d], R.normalized(ref), bound["out"][:, :d])
    print(f"ratio {label} {precision}: raw {ratio:.3f} (max bound {bound['raw'].max():.3g}, max error {np.abs(raw[:, :d] - ref).max():.3g}), "
          f"normalised {ratio_n:.3f}")
    assert bound["raw"].max() <= R.CAP
    assert np.isfinite(raw).all() and np.isfinite(out).all(), label
    assert R.within(raw[:, :d], ref, bound["raw"][:, :d], FACTOR), (label, precision, ratio)
    assert R.within(out[:, :d], R.normalized(ref), bound["out"][:, :d], FACTOR), (label, precision, ratio_n)
    assert not raw[:, d:].any() and not out[:, d:].any(), (label, "a padded unit is not exactly 0")
    return ratio


# ---- 1. the gate functions in isolation ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", R.PRECISIONS)
def test_gate_functions_in_isolation(precision):
    """T = 1: h_0 = 0, W_hh does not matter; units sweep one gate's pre-activation over [-104, 104] with the others held."""
    inp = R.gate_inputs()
    out, raw = _encode(inp, precision)
    ref, bound = _reference(inp, precision)
    err = np.abs(raw - ref)
    q4 = inp["d"] // 4
    per_gate = ", ".join(f"{g} {err[:, q * q4: (q + 1) * q4].max():.3g}" for q, g in enumerate("ifgo"))
    print(f"gate sweep {precision}: max |raw - ref64| {err.max():.3g} (swept gate: {per_gate}), max bound {bound['raw'].max():.3g}, "
          f"worst ratio {R.worst_ratio(raw, ref, bound['raw']):.3f}")
    assert np.isfinite(raw).all() and np.isfinite(out).all()
    assert R.within(raw, ref, bound["raw"], FACTOR)


# ---- 2. every width and precision, one-and-a-bit groups --------------------------------------------------------------------------------

WIDTH_CASES = dict(R.width_cases())


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("label", list(WIDTH_CASES))
def test_every_width_within_float64_bound(label, precision):
    inp = WIDTH_CASES[label]
    out, raw = _encode(inp, precision)
    assert raw.shape == (len(inp["lengths"]), R.kernel_dim(inp["d"]))
    _check_bounded(label, inp, precision, out, raw)
    out2, raw2 = _encode(inp, precision)
    assert R.bits_equal(raw, raw2) and R.bits_equal(out, out2), (label, "second call differs")


# ---- 3. reference-like weights at T = 2, three values of w_hh_scale -------------------------------------------------------------------

SCALE_CASES = dict(R.scale_cases())


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("label", list(SCALE_CASES))
def test_reference_like_weights_and_scales_within_bound(label, precision):
    inp = SCALE_CASES[label]
    out, raw = _encode(inp, precision)
    _check_bounded(label, inp, precision, out, raw)


@pytest.mark.parametrize("d", [d for d, _ in R.WIDTHS])
def test_the_scales_really_differ(d):
    """The scale each pack carries: x 2^-6 and x 1 both sit at f16x3_scale's upper clip 2^15, x 8 and x 64 below it."""
    scales = [_pack(SCALE_CASES[f"reference x{m:g} d={d} B=37 T=2"], "f16x3")[0]["w_hh_scale"] for m in R.MULTS]
    print(f"w_hh_scale d={d}: {scales}")
    assert len(set(scales)) == 3 and scales[0] == scales[1] > scales[2] > scales[3]


# ---- 4. second and third pass of the group loop -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("passes", [2, 3])
@pytest.mark.parametrize("d,precision", [(128, "f16x3"), (256, "f16x3"), (128, "fp32")])
def test_group_loop_later_passes(d, precision, passes):
    per_dir = _per_dir()
    inp = R.group_inputs(d, per_dir, passes)
    tok, ln = inp["tokens"], inp["lengths"]
    b = len(ln)
    assert b == 32 * per_dir * (passes - 1) + 1
    grid, per_wg = R.schedule(b, precision, 2 * per_dir)
    assert len(per_wg[0]) == (passes if precision == "f16x3" else 1)
    rows = R.group_rows(b, per_dir)
    out, raw = _encode(inp, precision)
    # (a) float64 bound on the row subset
    _check_bounded(f"group loop d={d} B={b} passes={passes}", inp, precision, out[rows], raw[rows], rows)
    # (b) batch invariance, bit for bit: the row's own group alone, and a batch of one
    for g in sorted(set((rows // 32).tolist())):
        lo, hi = 32 * g, min(32 * g + 32, b)
        o_g, r_g = _encode(inp, precision, tok[lo:hi], ln[lo:hi])
        sel = rows[(rows >= lo) & (rows < hi)]
        assert R.bits_equal(r_g[sel - lo], raw[sel]) and R.bits_equal(o_g[sel - lo], out[sel]), ("group alone", g)
    for r in rows:
        o_1, r_1 = _encode(inp, precision, tok[r: r + 1], ln[r: r + 1])
        assert R.bits_equal(r_1[0], raw[r]) and R.bits_equal(o_1[0], out[r]), ("batch of one", int(r))


# ---- 5. layout contracts, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("d", [128, 256])
def test_padding_ids_are_never_read_and_row_pitch_is_the_buffers_T(d, precision):
    base = R.case_inputs(d, 37, 5, 11)
    inp = dict(base)
    emb = np.array(base["emb"])
    emb[-1] = 64.0 * np.where(np.arange(d) % 2, 1.0, -1.0)             # a large table row for the valid id vocab - 1
    inp["emb"] = emb
    tok, ln = base["tokens"], base["lengths"]
    t = tok.shape[1]
    valid = np.arange(t)[None, :] < ln[:, None]
    out, raw = _encode(inp, precision)
    filled = np.where(valid, tok, inp["vocab"] - 1).astype(np.int32)
    assert filled.max() < inp["vocab"] and filled.min() >= 0 and (filled != tok).any()
    out_f, raw_f = _encode(inp, precision, filled, ln)
    assert R.bits_equal(raw_f, raw) and R.bits_equal(out_f, out), "an id behind a sentence's length was read"
    wide = np.full((len(ln), 9), inp["vocab"] - 1, np.int32)
    wide[:, :t] = filled
    out_w, raw_w = _encode(inp, precision, wide, ln)
    assert R.bits_equal(raw_w, raw) and R.bits_equal(out_w, out), "a tokens buffer of T = 9 was not read at a row pitch of 9 (the longest length is 5)"
    assert np.isfinite(raw).all() and np.abs(raw).max() > 0.0


# ---- 6. long sequences ------------------------------------------------------------------------------------------------------------------

LONG_CONTRACTIVE, LONG_REFERENCE = dict(R.long_cases("contractive")), dict(R.long_cases("reference"))


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("label", list(LONG_CONTRACTIVE))
def test_long_sequences_contractive_within_bound(label, precision):
    inp = LONG_CONTRACTIVE[label]
    assert inp["lengths"][0] == R.LONG_T and inp["lengths"][1] == 1
    out, raw = _encode(inp, precision)
    _check_bounded(label, inp, precision, out, raw)


@pytest.mark.parametrize("label", list(LONG_REFERENCE))
def test_long_sequences_reference_like_within_tol(label):
    inp = LONG_REFERENCE[label]
    d = inp["d"]
    ref = R.bilstm_ref64(inp)
    got = {p: _encode(inp, p) for p in R.PRECISIONS}
    for p in R.PRECISIONS:
        out, raw = got[p]
        e_raw, e_out = np.abs(raw[:, :d] - ref).max(), np.abs(out[:, :d] - R.normalized(ref)).max()
        print(f"{label} {p}: max |raw - ref64| {e_raw:.3g}, normalised {e_out:.3g}")
        assert e_raw < R.TOL and e_out < R.TOL, (label, p)
    between = max(np.abs(got["fp32"][i] - got["f16x3"][i]).max() for i in (0, 1))
    print(f"{label} fp32 vs f16x3: {between:.3g}")
    assert between < R.TOL_PRECISIONS


# ---- 7. C ABI ---------------------------------------------------------------------------------------------------------------------------

def _abi_call(inp, w, dk, workspace, workspace_bytes, out, raw, batch=None, embed_dim=None):
    from text2pos_amd import _lib as L
    from text2pos_amd import ops
    tok = torch.from_numpy(np.array(inp["tokens"])).to(_dev())
    ln = torch.from_numpy(np.array(inp["lengths"])).to(_dev())
    b = tok.shape[0] if batch is None else batch
    rc = L.lib().t2p_encode_text(ops._ptr(tok), ops._ptr(ln), b, tok.shape[1], inp["vocab"], dk if embed_dim is None else embed_dim,
                                 C.byref(w), ops._ptr(raw), ops._ptr(out), ops._ptr(workspace), workspace_bytes, ops._stream(_dev()))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("precision", R.PRECISIONS)
def test_c_abi_workspace_contract(precision):
    from text2pos_amd import _lib as L
    inp = WIDTH_CASES["contractive d=256 B=37 T=7"]
    _, w, dk = _pack(inp, precision)
    b = len(inp["lengths"])
    need = int(L.lib().t2p_encode_text_workspace_bytes(b, inp["vocab"], dk))
    outs = []
    for with_raw in (False, True):
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=_dev())
        out = torch.full((b, dk), float("nan"), device=_dev())
        raw = torch.full((b, dk), float("nan"), device=_dev()) if with_raw else None
        assert _abi_call(inp, w, dk, ws, need, out, raw) == 0
        assert bool((ws[need:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
        outs.append(out.cpu().numpy())
        if with_raw:
            ref, bound = _reference(inp, precision)
            assert R.within(raw.cpu().numpy(), ref, bound["raw"], FACTOR)
    assert np.isfinite(outs[0]).all() and R.bits_equal(outs[0], outs[1])
    # one byte less: refused, `out` untouched
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=_dev())
    out = torch.full((b, dk), 7.25, device=_dev())
    assert _abi_call(inp, w, dk, ws, need - 1, out, None) == -2                   # T2P_E_WORKSPACE
    assert b"workspace" in L.lib().t2p_last_error()
    assert bool((out == 7.25).all())
    assert _abi_call(inp, w, dk, ws, need, out, None, batch=0) == 0 and bool((out == 7.25).all())


@pytest.mark.parametrize("precision", R.PRECISIONS)
def test_c_abi_refuses_unsupported_width(precision):
    """embed_dim = 192 is not instantiated: T2P_E_UNSUPPORTED, `out` untouched (weights and workspace sized for 192)."""
    from text2pos_amd import _lib as L
    from text2pos_amd import ops, packing
    d, vocab, b = 192, 11, 5
    rng = np.random.default_rng(8)
    dev = _dev()
    emb = torch.from_numpy(rng.uniform(-1, 1, (vocab, d)).astype(F32)).to(dev)
    w_ih = torch.from_numpy((rng.uniform(-1, 1, (2, d, 4 * d)) / 16).astype(F32)).to(dev)
    w_hh_host = torch.from_numpy((rng.uniform(-1, 1, (2, d, 4 * d)) / 16).astype(F32))
    bias = torch.zeros((2, 4 * d), device=dev)
    x3 = scale = None
    if precision == "f16x3":
        scale = packing.f16x3_scale(w_hh_host)
        x3 = torch.stack([packing.pack_f16x3_scaled(w_hh_host[i], scale) for i in range(2)]).contiguous().to(dev)
    w = ops.make_text_weights(emb, w_ih, w_hh_host.to(dev), bias, x3, scale or 0.0)
    inp = dict(tokens=rng.integers(0, vocab, (b, 4)).astype(np.int32), lengths=np.full(b, 4, np.int32), vocab=vocab)
    need = int(L.lib().t2p_encode_text_workspace_bytes(b, vocab, d))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = torch.full((b, d), 7.25, device=dev)
    assert _abi_call(inp, w, d, ws, need, out, None) == -3                         # T2P_E_UNSUPPORTED
    assert b"192" in L.lib().t2p_last_error()
    assert bool((out == 7.25).all())
