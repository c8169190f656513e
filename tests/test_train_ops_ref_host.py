"""CPU tests of tests/train_ops_ref.py, the references and bounds that tests/test_gpu_train_ops.py holds the kernels of
csrc/train_ops.hip to: for every operation and every shape of the GPU tests the fp32 emulation of the kernel's arithmetic stays
within 1 x the first-order bound of the float64 statement (reference and bound agree without a GPU), and the checker at the GPU
tests' factor (2 x bound, or bit equality) rejects a deliberately wrong emulation of each kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ops_ref as R  # noqa: E402

BN_CASES = list(range(len(R.BN_SHAPES)))
BN_CHUNKS = [2, 3, 2, 3, 1, 2]      # row chunks per segment that the launch picks for R.BN_SHAPES


def _bn(case, relu, wrong=None, inputs=None):
    sizes, _ = R.BN_SHAPES[case]
    x, gamma, beta, dy = inputs or R.bn_inputs(case)
    ref = R.bn_ref64(x, sizes, gamma, beta, relu, dy)
    return ref, R.bn_bounds(x, sizes, gamma, beta, ref, dy), R.bn_emul(x, sizes, gamma, beta, relu, dy, wrong=wrong)


BN_KEYS = ["mean", "invstd", "var_unbiased", "y", "dx", "dgamma_seg", "dbeta_seg"]


def test_bn_shapes_take_the_row_chunk_counts_they_are_chosen_for():
    assert [R.bn_chunks(sum(s), len(s)) for s, _ in R.BN_SHAPES] == BN_CHUNKS
    assert [R.bn_chunks(sum(s), len(s)) for s in ([50], [7, 2, 300, 33], [2, 2, 5], [1000, 3])] == [1, 1, 1, 1]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", BN_CASES)
def test_bn_emulation_within_one_bound_and_relu_margin_holds(case, relu):
    ref, bounds, emu = _bn(case, relu)
    ratios = {k: R.worst_ratio(emu[k], ref[k], bounds[k]) for k in BN_KEYS}
    print(R.BN_SHAPES[case], relu, {k: round(v, 3) for k, v in ratios.items()}, "margin", R.bn_relu_margin(ref, bounds))
    for k in BN_KEYS:
        assert R.within(emu[k], ref[k], bounds[k], 1.0), (k, ratios[k])
    assert R.bn_relu_margin(ref, bounds) >= 8.0
    assert np.array_equal(emu["y"] > 0, ref["pre"] > 0)


@pytest.mark.parametrize("wrong,case,keys", [("unbiased_var", 0, ["invstd", "y", "dx"]), ("unbiased_var", 3, ["invstd", "y", "dx"]),
                                             ("drop_last_chunk", 0, ["mean", "y"]), ("drop_last_chunk", 1, ["mean", "y"]),
                                             ("drop_last_chunk", 5, ["mean", "y"]), ("no_xhat_term", 2, ["dx"]),
                                             ("no_xhat_term", 4, ["dx"])])
def test_bn_checker_rejects_wrong_emulations(wrong, case, keys):
    for relu in (0, 1):
        ref, bounds, emu = _bn(case, relu, wrong)
        for k in keys:
            assert not R.within(emu[k], ref[k], bounds[k], 2.0), (wrong, k)


def test_bn_checker_rejects_a_relu_mask_that_lets_exact_zeros_through():
    """beta = 0 under gamma = 0 makes a whole column of exact zeros: y > 0 is false there, y >= 0 true."""
    case = 4
    sizes, _ = R.BN_SHAPES[case]
    x, gamma, beta, dy = (a.copy() for a in R.bn_inputs(case))
    gamma[5] = beta[5] = 0
    ref, bounds, good = _bn(case, 1, None, (x, gamma, beta, dy))
    assert np.all(ref["pre"][:, 5] == 0) and np.all(ref["dbeta_seg"][:, 5] == 0)
    for k in BN_KEYS:
        assert R.within(good[k], ref[k], bounds[k], 1.0), k
    bad = R.bn_emul(x, sizes, gamma, beta, 1, dy, wrong="mask_ge")
    assert R.within(bad["y"], ref["y"], bounds["y"], 2.0)             # the forward cannot tell
    assert not R.within(bad["dbeta_seg"], ref["dbeta_seg"], bounds["dbeta_seg"], 2.0)


def test_bn_reference_propagates_nan_and_inf_per_segment_and_column():
    sizes, c = R.BN_SHAPES[4]
    x, gamma, beta, _ = (a.copy() for a in R.bn_inputs(4))
    x[3, 2], x[38, 9] = np.nan, np.inf                                # segment 0 column 2, segment 1 column 9
    for relu in (0, 1):
        ref = R.bn_ref64(x, sizes, gamma, beta, relu)
        want = np.zeros(x.shape, bool)
        want[:37, 2] = want[37:39, 9] = True
        assert np.array_equal(np.isnan(ref["y"]), want)
        emu = R.bn_emul(x, sizes, gamma, beta, relu)
        assert R.within(emu["y"], ref["y"], R.bn_bounds(x, sizes, gamma, beta, ref)["y"], 1.0)


def test_bn_running_estimates_recurrence():
    mean, var = np.array([[1.0], [2.0], [4.0]]), np.array([[1.0], [1.0], [2.0]])
    rm, rv, t = R.bn_running_ref64(mean, var, np.array([0.0]), np.array([1.0]), 2, None)
    assert t == 5 and np.allclose(rm, (2 * 0.0 + 7.0) / 5) and np.allclose(rv, (2 * 1.0 + 4.0) / 5)
    rm, _, t = R.bn_running_ref64(mean, var, np.array([0.0]), np.array([1.0]), 2, 0.1)
    assert t == 5 and np.allclose(rm, 0.1 * 0.81 * 1 + 0.1 * 0.9 * 2 + 0.1 * 4)


@pytest.mark.parametrize("c", R.SEG_CHANNELS)
def test_segment_max_reference_has_ties_and_rejects_last_row_ties(c):
    x, dout, ptr = R.seg_inputs(c)
    out, arg = R.segment_max_ref(x, ptr)
    assert out[2].tolist() == [0.0] * c and arg[2].tolist() == [-1] * c              # the empty segment
    big = x[ptr[6]: ptr[7]]
    tied = (big == big.max(0)).sum(0) > 1
    lanes = [len({int(r) % 4 for r in np.nonzero(big[:, j] == big[:, j].max())[0]}) > 1 for j in range(c)]
    assert tied.mean() > 0.5 and np.mean(lanes) > 0.5                                 # most columns tie across different row lanes
    out_l, arg_l = R.segment_max_ref(x, ptr, wrong="last_tie")
    assert np.array_equal(out_l, out) and not np.array_equal(arg_l, arg)
    assert not np.array_equal(R.segment_max_backward_ref(dout, arg_l, len(x)), R.segment_max_backward_ref(dout, arg, len(x)))


def test_segment_max_reference_on_non_finite_columns():
    x = np.array([[1.0, -np.inf], [np.nan, -np.inf], [3.0, -np.inf], [np.nan, -np.inf]], np.float32)
    out, arg = R.segment_max_ref(x, np.array([0, 4], np.int32))
    assert np.isnan(out[0, 0]) and arg[0, 0] == 1 and out[0, 1] == -np.inf and arg[0, 1] == 0


@pytest.mark.parametrize("c", R.SEG_CHANNELS)
@pytest.mark.parametrize("first,tail", [(0, 0), (3, 2)])
def test_segment_mean_emulation_within_one_bound_and_n_minus_1_rejected(c, first, tail):
    x, dout, ptr = R.seg_inputs(c, first, tail)
    ref, dref = R.segment_mean_ref64(x, ptr, dout)
    b, bdx = R.segment_mean_bounds(x, ptr, dout)
    emu, demu = R.segment_mean_emul(x, ptr, dout)
    assert R.within(emu, ref, b, 1.0) and R.within(demu, dref, bdx, 1.0)
    assert np.all(dref[: first] == 0) and np.all(dref[len(x) - tail:] == 0)
    bad, dbad = R.segment_mean_emul(x, ptr, dout, wrong="n_minus_1")
    assert not R.within(bad, ref, b, 2.0) and not R.within(dbad, dref, bdx, 2.0)


@pytest.mark.parametrize("c", R.EDGE_CHANNELS)
def test_edge_features_inputs_emulation_and_wrong_pitch(c):
    x, pos, pos_c, src, dst, d_out, w = R.edge_inputs(c)
    deg = np.bincount(src, minlength=len(x))
    assert w == {3: 8, 64: 72, 128: 136}[c] and len(src) == 5000 and deg.max() >= 3000 and 95 <= (deg == 0).sum() <= 110
    assert dst.min() >= 0 and dst.max() < 150 and np.all(np.isnan(d_out[:, c:])) and w > c
    out = R.edge_features_forward_ref(x, pos, pos_c, src, dst, w)
    assert np.all(out[:, c + 3:] == 0) and out.dtype == np.float32
    ref, bound = R.edge_features_backward_ref64(d_out, src, len(x), c)
    assert np.isfinite(ref).all() and np.all(ref[deg == 0] == 0) and np.all(bound[deg == 0] == 0)
    assert R.within(R.edge_features_backward_emul(d_out, src, len(x), c), ref, bound, 1.0)
    assert not R.within(R.edge_features_backward_emul(d_out, src, len(x), c, wrong="pitch_c"), ref, bound, 2.0)


@pytest.mark.parametrize("d", R.PAIR_DIMS)
def test_pair_features_inputs_emulation_and_wrong_sign(d):
    x, tgt, src, d_out = R.pair_inputs(d)
    assert len(tgt) == len(src) == 4000 and len(x) == 260 and np.all(np.diff(tgt) >= 0)
    assert (src == tgt).sum() >= 500 and (src == 3).sum() >= 500
    ref, bound = R.pair_features_backward_ref64(d_out, tgt, src, len(x))
    assert R.within(R.pair_features_backward_emul(d_out, tgt, src, len(x)), ref, bound, 1.0)
    assert not R.within(R.pair_features_backward_emul(d_out, tgt, src, len(x), wrong="sum_to_target"), ref, bound, 2.0)


@pytest.mark.parametrize("n_rows,dim", R.ROWNORM_SHAPES)
def test_rownorm_backward_emulation_within_one_bound_and_projection_needed(n_rows, dim):
    x, dy, special = R.rownorm_inputs(n_rows, dim)
    ref, bound = R.rownorm_backward_ref64(x, dy)
    emu = R.rownorm_backward_emul(x, dy)
    print(n_rows, dim, R.worst_ratio(emu, ref, bound))
    assert R.within(emu, ref, bound, 1.0)
    nrm = np.linalg.norm(x.astype(np.float64), axis=1)
    if n_rows > 1:
        assert nrm[nrm > 0].min() < 2e-3 and nrm.max() > 0.5e3
    if special:
        z, cz, o = special["zero"], special["cancel"], special["orthogonal"]
        assert np.array_equal(emu[z], dy[z] * (np.float32(1) / np.float32(1e-12))) and np.allclose(ref[z], dy[z].astype(np.float64) * 1e12)
        scale = np.abs(dy[cz].astype(np.float64)) / nrm[cz]
        assert np.all(np.abs(ref[cz]) <= 1e-6 * scale.max())          # pure cancellation: the result is rounding residue
        assert abs(float(x[o].astype(np.float64) @ dy[o].astype(np.float64))) <= 1e-6 * nrm[o] * np.linalg.norm(dy[o])
    assert not R.within(R.rownorm_backward_emul(x, dy, wrong="no_projection"), ref, bound, 2.0)
