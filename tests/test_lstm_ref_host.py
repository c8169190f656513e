"""CPU checks of tests/lstm_ref.py, the yardstick of tests/test_gpu_text_recurrence.py: the float64 statement is what torch's own
nn.Embedding + pack_padded_sequence + nn.LSTM(bidirectional) computes in float64, the exact gate tables are exact, the NumPy
emulation of both kernels stays within 1 x the derived bound on every case, no bound passes CAP = 5e-5 (half the suite's TOL),
and the check the GPU test applies - within(got, ref, bound, 2.0) - rejects every emulated defect on one case or more.
Every test prints its figures before it asserts (pytest -s shows them; docs/notebook.md records a run)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_ref as R  # noqa: E402

HOST_PER_DIR = 2                     # the schedule of a device with 4 CUs: two workgroups per direction
HOST_CUS = 2 * HOST_PER_DIR


def _group_cases():
    return [(f"group loop d={d} passes={p} (per_dir={HOST_PER_DIR})", R.group_inputs(d, HOST_PER_DIR, p)) for d in (128, 256) for p in (2, 3)]


def _bound_cases():
    return R.width_cases() + R.scale_cases() + R.long_cases("contractive") + _group_cases()


CASES = dict(_bound_cases())
ALL_CASES = dict(_bound_cases() + R.long_cases("reference"))
# every case is emulated on both precisions.  The fp32 emulation is an fma chain over k per time step: at T = 162 it runs on eight
# rows at D = 128 and on three past it (the row of length T and the row of length 1 among them); f16x3 runs every row
LONG_ROWS = np.array([0, 1, 2, 3, 5, 8, 13, 39])
LONG_ROWS_WIDE = np.array([0, 1, 39])


def _emulated_rows(label, b, dk, precision):
    """Rows are independent.  The f16x3 emulation (24 k-steps at most) runs every row; the fp32 one, whose cost per row grows with
    the square of the width, runs the first four rows and the last five (the partial group) past 128 units, and LONG_ROWS /
    LONG_ROWS_WIDE at T = 162."""
    if f"T={R.LONG_T}" in label and precision == "fp32":
        return LONG_ROWS if dk == 128 else LONG_ROWS_WIDE
    if precision == "fp32" and dk > 128 and b > 9:
        return np.r_[0:4, b - 5: b]
    return np.arange(b)


_SHARED = {}


def _ref(label, inp):
    """The float64 statement of a case, computed once and handed out read-only."""
    if label not in _SHARED:
        _SHARED[label] = R.bilstm_ref64(inp)
        _SHARED[label].setflags(write=False)
    return _SHARED[label]


def _bound(label, inp, precision):
    if (label, precision) not in _SHARED:
        _SHARED[label, precision] = R.bilstm_bound(inp, precision)
    return _SHARED[label, precision]


def _torch_ref64(inp):
    import torch
    import torch.nn as nn
    d, v = inp["d"], inp["vocab"]
    emb = nn.Embedding(v, d, padding_idx=0).double()
    lstm = nn.LSTM(input_size=d, hidden_size=d, bidirectional=True, num_layers=1).double()
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(np.array(inp["emb"])).double())
        for i, suffix in enumerate(("", "_reverse")):
            for name, key in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
                getattr(lstm, name + suffix).copy_(torch.from_numpy(np.array(inp[key][i])).double())
        x = emb(torch.from_numpy(np.array(inp["tokens"])).long())                       # [B][T][d]
        packed = nn.utils.rnn.pack_padded_sequence(x, torch.from_numpy(np.array(inp["lengths"])).long(), batch_first=True,
                                                   enforce_sorted=False)
        _, (h, _) = lstm(packed)
        return h.mean(0).numpy()


@pytest.mark.parametrize("label", list(ALL_CASES) + ["gates"])
def test_ref64_is_torch_float64_lstm(label):
    inp = R.gate_inputs() if label == "gates" else ALL_CASES[label]
    ref, want = _ref(label, inp), _torch_ref64(inp)
    err = float(np.abs(ref - want).max())
    print(f"ref64 vs torch float64, {label}: {err:.3g}")
    assert err <= 1e-12
    nrm = R.normalized(ref)
    assert np.allclose((nrm * nrm).sum(1), 1.0, atol=1e-12)
    if f"T={R.LONG_T}" not in label:
        rows = np.arange(len(inp["lengths"]))[::3]
        assert np.abs(R.bilstm_ref64(inp, rows) - ref[rows]).max() <= 1e-15   # rows are independent (BLAS blocks by shape)


@pytest.mark.parametrize("label", list(ALL_CASES) + ["gates"])
def test_gate_table_is_exact_in_fp32(label):
    inp = R.gate_inputs() if label == "gates" else ALL_CASES[label]
    assert inp["tokens"].min() >= 0 and inp["tokens"].max() < inp["vocab"]
    assert not inp["emb"][0].any()
    if label != "gates":                            # the fma chain over k in both orders
        assert R.table_is_exact(inp)
    else:
        kv = R.kernel_view(inp, inp["d"])
        assert np.array_equal(kv["table"].astype(np.float32).astype(np.float64), kv["table"])


@pytest.mark.parametrize("label", list(CASES))
def test_inputs_cover_the_token_and_length_edges(label):
    inp = CASES[label]
    tok, ln = inp["tokens"], inp["lengths"]
    b, t = tok.shape
    valid = np.arange(t)[None, :] < ln[:, None]
    words = tok[valid]
    assert inp["vocab"] - 1 in words and 0 in words
    if valid.sum() >= inp["vocab"]:
        assert set(words.tolist()) == set(range(inp["vocab"]))
    assert not tok[~valid].any() and ln.min() >= 1 and ln.max() == t
    if "B=37" in label and "T=7" in label:
        assert 1 in ln and sorted(ln[32:].tolist()) == [1] * 4 + [t]     # a group with one row at T and the rest at 1
    if "B=32" in label:
        assert len(set(ln.tolist())) == 1                                # a group of 32 rows of one length


def test_group_loop_lengths_alternate_by_pass():
    for passes in (2, 3):
        inp = R.group_inputs(128, HOST_PER_DIR, passes)
        ln = inp["lengths"]
        assert len(ln) == 32 * HOST_PER_DIR * (passes - 1) + 1
        grid, per_wg = R.schedule(len(ln), "f16x3", HOST_CUS)
        assert grid == HOST_PER_DIR and len(per_wg[0]) == passes
        for groups in per_wg:                    # a workgroup's consecutive groups: short then long, or long then short
            kinds = [int(ln[32 * g: 32 * g + 32].max()) for g in groups]
            assert all((a <= 2) != (b <= 2) for a, b in zip(kinds, kinds[1:])), kinds
            assert all(k <= 2 or k == 5 for k in kinds)


def test_schedule_restates_the_launcher():
    grid, per_wg = R.schedule(4097, "f16x3", 256)
    assert grid == 128 and per_wg[0] == [0, 128] and per_wg[1] == [1] and len(per_wg) == 128
    grid, per_wg = R.schedule(8193, "f16x3", 256)
    assert grid == 128 and per_wg[0] == [0, 128, 256] and per_wg[127] == [127, 255]
    assert R.schedule(4096, "f16x3", 256)[1][0] == [0]
    grid, per_wg = R.schedule(4097, "fp32", 256)
    assert grid == 129 and all(len(g) == 1 for g in per_wg)
    assert R.schedule(33, "f16x3", 1)[0] == 1 and R.schedule(33, "f16x3", 1)[1] == [[0, 1]]


def test_scale_restates_packing_and_takes_three_values():
    import torch
    from text2pos_amd import packing
    for d, _ in R.WIDTHS:
        scales = []
        for m in R.MULTS:
            inp = R.case_inputs(d, 37, 2, 11, "reference", m, live=R.LIVE_UNITS.get(m, 0))
            assert m > 1.0 or R.LIVE_UNITS.get(m, 0) == 0        # up to x 1 every unit of h_1 is alive
            s = R.w_hh_scale(inp)
            assert s == packing.f16x3_scale(torch.from_numpy(np.array(inp["w_hh"])))
            scales.append(s)
        print(f"w_hh_scale d={d}: {scales}")
        assert scales[0] == scales[1] == 2.0 ** 15          # the clip of f16x3_scale: x 2^-6 and x 1 share the largest scale
        assert len(set(scales)) == 3 and scales[1] > scales[2] > scales[3]


@pytest.mark.parametrize("label", list(CASES))
def test_bound_below_cap_and_emulation_within_it(label):
    inp = CASES[label]
    d = inp["d"]
    ref = _ref(label, inp)
    for precision in R.PRECISIONS:
        bound = _bound(label, inp, precision)
        top = float(bound["raw"].max())
        line = f"{label} {precision}: max bound {top:.3g} (normalised {float(bound['out'].max()):.3g})"
        rows = _emulated_rows(label, len(ref), R.kernel_dim(d), precision)
        got = R.bilstm_emul(inp, precision, HOST_CUS, rows=rows)
        want, b_raw, b_out = ref[rows], bound["raw"][rows][:, :d], bound["out"][rows][:, :d]
        ratio = R.worst_ratio(got[:, :d], want, b_raw)
        ratio_n = R.worst_ratio(R.rownorm_emul(got)[:, :d], R.normalized(want), b_out)
        print(line + f", emulation / bound {ratio:.3f} (normalised {ratio_n:.3f})")
        assert top <= R.CAP
        assert R.within(got[:, :d], want, b_raw, 1.0)
        assert R.within(R.rownorm_emul(got)[:, :d], R.normalized(want), b_out, 1.0)
        assert not got[:, d:].any()                      # padded units stay exactly 0


@pytest.mark.parametrize("precision", R.PRECISIONS)
def test_gate_sweep_emulation_within_t1_bound(precision):
    inp = R.gate_inputs()
    ref, bound = _ref("gates", inp), _bound("gates", inp, precision)["raw"]
    got = R.bilstm_emul(inp, precision)
    print(f"gate sweep {precision}: max bound {bound.max():.3g}, emulation / bound {R.worst_ratio(got, ref, bound):.3f}")
    assert len(inp["xs"]) >= 4096 and np.isfinite(got).all()
    assert bound.max() <= R.CAP and R.within(got, ref, bound, 1.0)


# wrong variant -> the cases that must reject it (precision, label, inputs)
def _wrong_cases(wrong):
    widths = dict(R.width_cases())
    edge = [(p, "contractive d=128 B=37 T=7", widths["contractive d=128 B=37 T=7"]) for p in R.PRECISIONS]
    groups = [("f16x3", k, v) for k, v in _group_cases()]
    return {"state_not_reset": groups, "planes_not_cleared": groups, "reverse_from_T": edge, "finished_row_updated": edge,
            "last_word_zero_row": edge, "no_lo_hi": [("f16x3", k, dict(R.scale_cases())[k]) for k in ("permuted d=128 B=37 T=3", "reference x1 (64 live) d=128 B=37 T=2",
                                                                          "reference x64 d=128 B=37 T=2")],
            "table_not_scaled": edge[1:], "drain_no_inv_scale": edge[1:]}[wrong]


@pytest.mark.parametrize("wrong", R.WRONG)
def test_every_emulated_defect_is_rejected(wrong):
    for precision, label, inp in _wrong_cases(wrong):
        d = inp["d"]
        ref, bound = _ref(label, inp), _bound(label, inp, precision)["raw"]
        good = R.bilstm_emul(inp, precision, HOST_CUS)
        bad = R.bilstm_emul(inp, precision, HOST_CUS, wrong=wrong)
        print(f"{wrong} on {label} {precision}: error / bound {R.worst_ratio(bad[:, :d], ref, bound[:, :d]):.3g}")
        assert R.within(good[:, :d], ref, bound[:, :d], R.FACTOR_GPU)
        assert not R.within(bad[:, :d], ref, bound[:, :d], R.FACTOR_GPU), (wrong, label, precision)
