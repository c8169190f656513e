"""Sweep of the fp16-range guard of the f16x3 path, stage by stage, against one float64 oracle evaluation.

The f16x3 path's accuracy claim (1e-4 against the reference) rests on one rule: the guard stays silent only when the result is
accurate; otherwise the call raises (on_overflow="raise") or is recomputed on the exact fp32 path (on_overflow="fp32").  Each row
of tests/guard_rescale.py moves ONE stage's activations by a power of two s = 2^k, k = -20, -18, ..., 20, while the network's
function stays exactly the same, so the float64 oracle's output at s = 1 is the reference at every s.  With m(s) = the stage's
largest activation at s = 1 (oracle, float32) times s, every f16x3 call must

  1. raise FloatingPointError, be refused by packing (Fp16RangeError, only where a folded weight really passes 65504), or return
     a result within 1e-4 of the reference;
  2. raise with the row's own bit where m(s) >= 65504 (fp16's largest finite value), or be refused by packing (the scale that
     moves the stage that far also drives a folded weight past fp16's range: nothing runs, and 1 checks the refusal);
  3. raise with bit 0x80, or be refused, where m(s) < 2^-8 (the low side: fp16 pieces of such activations lose their lo part);
  4. stay silent where m(s) lies in [2^-5, 2^7], the range of a trained, batch-normalised network's activations;
and the exact fp32 path meets the reference at every s (5), and on_overflow="fp32" at the hottest and the coldest raising s of a
row returns exactly the fp32 model's result (6).
"""
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_rescale as GR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
KS = list(range(-20, 21, 2))
FP16_MAX = 65504.0
LOW, BAND = 2.0 ** -8, (2.0 ** -5, 2.0 ** 7)
# folded weights that get an f16x3 image (packing._add_x3_images): a refusal must come from one of them past fp16's range
_X3_WEIGHTS = ("sa_w1", "sa_w2", "ga_w1", "ga_w2", "lin1_w", "lin2_w", "pn_w", "merge_w", "g_wp", "g_wq", "g_w2")


def _dev():
    return torch.device("cuda:0")


def _largest_folded_weight(model):
    from text2pos_amd import packing
    p = packing.pack_cell_weights(model, "cpu", x3=False)
    ts = [t for k in _X3_WEIGHTS for t in (p[k] if isinstance(p[k], list) else [p[k]])]
    return max(float(t.abs().max()) for t in ts)


def _call(m, args, cell_ptr):
    """('ok', result float64 on the host) | ('raise', guard code) | ('refused', largest folded weight)."""
    from text2pos_amd import packing
    try:
        with torch.no_grad():
            return "ok", m.encode_objects_packed(*args, cell_ptr).cpu().double()
    except packing.Fp16RangeError:
        return "refused", _largest_folded_weight(m)
    except FloatingPointError as e:
        return "raise", int(re.search(r"guard code (0x[0-9a-f]+)", str(e)).group(1), 16)


@pytest.fixture(scope="module")
def sweep(oracle_model, vocab):
    """{row: {k: outcome}} over every row and s = 2^k, plus the reference and the per-row maxima at s = 1."""
    import copy
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    cells = S.make_cells(91, 6)
    xyz, rgb, center, mean_rgb, cell_ptr = cells
    _, amax = GR.activation_maxima(oracle_model, *cells)
    om64 = copy.deepcopy(oracle_model).double()
    orig_float = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()     # (the oracle casts some of its inputs with .float())
    try:
        want = om64.encode_objects_packed(xyz.astype(np.float64), rgb.astype(np.float64), center.astype(np.float64),
                                          mean_rgb.astype(np.float64), cell_ptr)
    finally:
        torch.Tensor.float = orig_float

    def build(**kw):
        m = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(), **kw)
        return m.to(_dev()).eval()
    x3, exact, redo = build(), build(precision="fp32"), build(on_overflow="fp32")
    sd0 = oracle_model.state_dict()
    dev_const = [torch.from_numpy(a).to(_dev()) for a in (xyz, center, mean_rgb)]
    out = {}

    def inputs(row, k):
        sd, rgb_s = GR.apply(sd0, rgb, row, 2.0 ** k)
        return sd, [dev_const[0], torch.from_numpy(np.ascontiguousarray(rgb_s)).to(_dev()), dev_const[1], dev_const[2]]
    for row in GR.ROWS:
        out[row] = {}
        for k in KS:
            sd, args = inputs(row, k)
            x3.load_state_dict(sd, strict=True)
            exact.load_state_dict(sd, strict=True)
            kind, val = _call(x3, args, cell_ptr)
            with torch.no_grad():
                ex = exact.encode_objects_packed(*args, cell_ptr).cpu().double()
            out[row][k] = dict(kind=kind, code=val if kind == "raise" else 0,
                               err=(val - want).abs().max().item() if kind == "ok" else None,
                               weight=val if kind == "refused" else None, m=amax[row] * 2.0 ** k,
                               err32=(ex - want).abs().max().item())
        # (6) on_overflow="fp32" at the hottest and the coldest raising s: exactly the fp32 model's result
        raising = [k for k in KS if out[row][k]["kind"] == "raise"]
        for k in sorted({min(raising), max(raising)}) if raising else []:
            sd, args = inputs(row, k)
            redo.load_state_dict(sd, strict=True)
            exact.load_state_dict(sd, strict=True)
            with torch.no_grad(), warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                got = redo.encode_objects_packed(*args, cell_ptr)
                ex = exact.encode_objects_packed(*args, cell_ptr)
            out[row][k]["redo_equal"] = torch.equal(got, ex) and any("recomputing" in str(x.message) for x in w)
    print(_table(out))
    return out


def _cell(o):
    if o["kind"] == "ok":
        return f"{o['err']:.0e}" + ("!" if o["err"] >= TOL else "")
    if o["kind"] == "raise":
        return f"{o['code']:#x}"
    return "refused" + ("" if o["weight"] > FP16_MAX else "!")


def _table(sweep):
    lines = ["row \\ log2 s   " + " ".join(f"{k:>7d}" for k in KS)]
    for row, r in sweep.items():
        lines.append(f"{row:15s} " + " ".join(f"{_cell(r[k]):>7s}" for k in KS))
    for row, r in sweep.items():     # the measured silent band: largest activation of the silent calls
        ms = [r[k]["m"] for k in KS if r[k]["kind"] == "ok"]
        if ms:
            lines.append(f"silent band {row:15s} m(s) in [2^{math.log2(min(ms)):.1f}, 2^{math.log2(max(ms)):.1f}]")
    return "\n".join(lines)


@pytest.mark.parametrize("row", list(GR.ROWS))
def test_guard_sweep(sweep, row):
    table = _table(sweep)
    r, bit, bad = sweep[row], GR.ROWS[row].bit, []
    for k in KS:
        o = r[k]
        if o["kind"] == "ok" and not o["err"] < TOL:
            bad.append(f"2^{k}: silent, max err {o['err']:.2e} (1: safety)")
        if o["kind"] == "refused" and not o["weight"] > FP16_MAX:
            bad.append(f"2^{k}: refused with every folded weight within fp16's range (1)")
        if not o["err32"] < TOL:
            bad.append(f"2^{k}: fp32 path max err {o['err32']:.2e} (5)")
        if "redo_equal" in o and not o["redo_equal"]:
            bad.append(f"2^{k}: on_overflow='fp32' is not the fp32 model's result (6)")
        if bit is None:
            continue
        if o["m"] >= FP16_MAX and not ((o["kind"] == "raise" and o["code"] & bit) or o["kind"] == "refused"):
            bad.append(f"2^{k}: m = {o['m']:.3g} past fp16's range without bit {bit:#x} (2)")
        if o["m"] < LOW and not ((o["kind"] == "raise" and o["code"] & 0x80) or o["kind"] == "refused"):
            bad.append(f"2^{k}: m = {o['m']:.3g} below 2^-8 without bit 0x80 (3)")
        if BAND[0] <= o["m"] <= BAND[1] and o["kind"] != "ok":
            bad.append(f"2^{k}: m = {o['m']:.3g} inside [2^-5, 2^7] but {_cell(o)} (4: false alarm)")
    assert not bad, f"{row}:\n  " + "\n  ".join(bad) + "\n" + table
