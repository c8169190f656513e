"""Every kernel of csrc/train_ops.hip on the cell branch's training path, one at a time, against the float64 references of
tests/train_ops_ref.py: |kernel - ref64| <= 2 x the first-order fp32 bound, element by element, or bit equality where the
operation is exact in fp32 (the maxima, the gathers, the copies).  No element is excluded from a comparison.  Output buffers
that a kernel is said to fill are handed to the C ABI prefilled with NaN.

BatchNorm shapes (segment sizes, C) and what they reach:
  ([1300, 2, 700], 32)   TQ = 8 kernels, 2 row chunks, the unrolled main loops, a 2-row segment split over 2 chunks
  ([1100], 8)            TQ = 8, C < 32 guard, 3 chunks
  ([900, 3, 700], 100)   TQ = 16, 2 chunks, second column block partly filled
  ([2100, 2], 256)       3 chunks, of which the 2-row segment's last is empty
  ([37, 2, 5], 67)       the scalar kernels (C % 4 != 0), one chunk
  ([1200, 2], 6)         the scalar kernels, two chunks
Every test prints its largest |got - ref64| / bound before it asserts (pytest -s shows them; docs/notebook.md records a run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 2.0


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.tensor(np.asarray(a), device=_dev())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=_dev())


def _np(t):
    return t.detach().cpu().numpy()


def _abi():
    from text2pos_amd import _lib as L
    from text2pos_amd.ops import _ptr, _stream
    return L, _ptr, _stream(_dev())


def _check(label, got, ref, bound):
    ratio = R.worst_ratio(got, ref, bound)
    print(f"ratio {label}: {ratio:.3f}")
    assert R.within(got, ref, bound, FACTOR), (label, ratio)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bn_reference(case, relu):
    sizes, _ = R.BN_SHAPES[case]
    x, gamma, beta, dy = R.bn_inputs(case)
    ref = R.bn_ref64(x, sizes, gamma, beta, relu, dy)
    return ref, R.bn_bounds(x, sizes, gamma, beta, ref, dy)


def _bn_forward(x, ptr, gamma, beta, relu):
    L, p, st = _abi()
    (m, c), s = x.shape, ptr.numel() - 1
    y, mean, invstd, var_u = _nan(m, c), _nan(s, c), _nan(s, c), _nan(s, c)
    ws = torch.empty(max(1, L.lib().t2p_bn_train_workspace_bytes(m, s, c)), dtype=torch.uint8, device=_dev())
    L.check(L.lib().t2p_bn_relu_train_forward(p(x), p(ptr), s, m, c, p(gamma), p(beta), R.EPS_BN, relu, p(y), p(mean), p(invstd),
                                              p(var_u), p(ws), ws.numel(), st), "t2p_bn_relu_train_forward")
    return dict(y=y, mean=mean, invstd=invstd, var_unbiased=var_u)


def _bn_backward(dy, x, ptr, gamma, beta, relu, mean, invstd):
    L, p, st = _abi()
    (m, c), s = x.shape, ptr.numel() - 1
    dx, dg, db = _nan(m, c), _nan(s + 1, c), _nan(s + 1, c)
    ws = torch.empty(max(1, L.lib().t2p_bn_train_workspace_bytes(m, s, c)), dtype=torch.uint8, device=_dev())
    L.check(L.lib().t2p_bn_relu_train_backward(p(dy), p(x), p(beta), p(ptr), s, m, c, p(mean), p(invstd), p(gamma), relu, p(dx), p(dg),
                                               p(db), p(ws), ws.numel(), st), "t2p_bn_relu_train_backward")
    return dict(dx=dx, dgamma_seg=dg, dbeta_seg=db)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", range(len(R.BN_SHAPES)))
def test_bn_relu_train_forward_backward_within_float64_bounds(case, relu):
    """y, mean, invstd, var_unbiased, dx, the per-segment dgamma / dbeta rows and their total in row n_seg; two calls give the same
    bits (fixed-order reductions).  With the ReLU the comparison means something only where kernel and reference agree on the
    mask: every float64 pre-activation lies at least 8 bounds of y from zero (asserted on the inputs)."""
    sizes, c = R.BN_SHAPES[case]
    ref, bounds = _bn_reference(case, relu)
    margin = R.bn_relu_margin(ref, bounds)
    print(f"{sizes} C={c} relu={relu} chunks={R.bn_chunks(sum(sizes), len(sizes))} relu margin {margin:.1f} bounds")
    assert margin >= 8.0
    x, gamma, beta, dy = (_t(a) for a in R.bn_inputs(case))
    ptr = _t(R.seg_ptr_of(sizes))
    fwd, again = _bn_forward(x, ptr, gamma, beta, relu), _bn_forward(x, ptr, gamma, beta, relu)
    bwd = _bn_backward(dy, x, ptr, gamma, beta, relu, fwd["mean"], fwd["invstd"])
    bwd_again = _bn_backward(dy, x, ptr, gamma, beta, relu, fwd["mean"], fwd["invstd"])
    torch.cuda.synchronize()
    for k in ("mean", "invstd", "var_unbiased", "y"):
        _check(k, _np(fwd[k]), ref[k], bounds[k])
        assert _bits_equal(_np(fwd[k]), _np(again[k])), k
    for k in ("dbeta_seg", "dgamma_seg", "dx"):
        _check(k, _np(bwd[k]), ref[k], bounds[k])
        assert _bits_equal(_np(bwd[k]), _np(bwd_again[k])), k


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("case", [0, 4])
def test_bn_relu_train_running_estimates(case, momentum):
    """bn_relu_train's closed-form update of running_mean / running_var / num_batches_tracked over three segments, starting from
    num_batches_tracked = 2, against nn.BatchNorm1d's recurrence applied segment by segment in float64 (momentum = None: the
    cumulative average)."""
    from text2pos_amd import train_ops as TO
    sizes, c = R.BN_SHAPES[case]
    assert len(sizes) == 3
    ref, bounds = _bn_reference(case, 1)
    x, gamma, beta, _ = R.bn_inputs(case)
    rng = np.random.default_rng(50 + case)
    rm0, rv0 = rng.standard_normal(c).astype(np.float32), (rng.random(c) + 0.5).astype(np.float32)
    bn = torch.nn.BatchNorm1d(c, momentum=momentum).to(_dev()).train()
    with torch.no_grad():
        bn.weight.copy_(_t(gamma))
        bn.bias.copy_(_t(beta))
        bn.running_mean.copy_(_t(rm0))
        bn.running_var.copy_(_t(rv0))
        bn.num_batches_tracked.fill_(2)
    y = TO.bn_relu_train(_t(x), _t(R.seg_ptr_of(sizes)), bn, relu=True)
    _check("y", _np(y), ref["y"], bounds["y"])
    want_m, want_v, tracked = R.bn_running_ref64(ref["mean"], ref["var_unbiased"], rm0, rv0, 2, momentum)
    _check("running_mean", _np(bn.running_mean), want_m, R.bn_running_bounds(ref["mean"], bounds["mean"], rm0, 2, momentum))
    _check("running_var", _np(bn.running_var), want_v,
           R.bn_running_bounds(ref["var_unbiased"], bounds["var_unbiased"], rv0, 2, momentum))
    assert int(bn.num_batches_tracked) == tracked == 5


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", [0, 2, 4])
def test_bn_relu_train_forward_keeps_nan_and_inf(case, relu):
    """One NaN in x makes that segment's column NaN in y, one +inf likewise (mean = inf, variance = NaN) - as BatchNorm1d (+ relu)
    called once per segment on the CPU does; every other segment and column is untouched."""
    sizes, c = R.BN_SHAPES[case]
    x, gamma, beta, _ = (a.copy() for a in R.bn_inputs(case))
    ptr = R.seg_ptr_of(sizes)
    x[ptr[0] + 5, 1] = np.nan                                   # segment 0, column 1
    x[ptr[2] + 1, c - 1] = np.inf                               # segment 2, last column
    ref = R.bn_ref64(x, sizes, gamma, beta, relu)
    bounds = R.bn_bounds(x, sizes, gamma, beta, ref)
    want_nan = np.zeros(x.shape, bool)
    want_nan[ptr[0]: ptr[1], 1] = want_nan[ptr[2]: ptr[3], c - 1] = True
    assert np.array_equal(np.isnan(ref["y"]), want_nan)
    bn = torch.nn.BatchNorm1d(c).train()
    with torch.no_grad():
        bn.weight.copy_(torch.tensor(gamma))
        bn.bias.copy_(torch.tensor(beta))
        ys = [bn(torch.tensor(x[ptr[i]: ptr[i + 1]])) for i in range(len(sizes))]
        y_torch = torch.cat([torch.relu(y) if relu else y for y in ys]).numpy()
    assert np.array_equal(np.isnan(y_torch), want_nan)
    got = _np(_bn_forward(_t(x), _t(ptr), _t(gamma), _t(beta), relu)["y"])
    print(f"{sizes} C={c} relu={relu}: NaN in y: {int(np.isnan(got).sum())} of {int(want_nan.sum())} expected, "
          f"zeros where NaN is expected: {int((got[want_nan] == 0).sum())}")
    assert np.array_equal(np.isnan(got), want_nan)
    _check("y beside the NaN columns", got, ref["y"], bounds["y"])


# ---- segment max / mean ------------------------------------------------------------------------------------------------------------

def _segment_max_abi(x, ptr):
    L, p, st = _abi()
    s, c = ptr.numel() - 1, x.shape[1]
    out, arg = _nan(s, c), torch.full((s, c), -7, dtype=torch.int32, device=_dev())
    L.check(L.lib().t2p_segment_max_forward(p(x), p(ptr), s, c, p(out), p(arg), st), "t2p_segment_max_forward")
    return out, arg


@pytest.mark.parametrize("c", R.SEG_CHANNELS)
def test_segment_max_forward_backward_bit_exact_with_ties(c):
    """out and arg against NumPy's argmax (the first row wins a tie; x holds 17 distinct values, so the 259-row segment ties in every
    column and across row lanes), the empty segment gives out = 0 / arg = -1, and the backward - a copy - writes every row of a
    tiling seg_ptr: dx is handed over full of NaN, as covers_all_rows=True hands over uninitialised memory."""
    L, p, st = _abi()
    x, dout, ptr = R.seg_inputs(c)
    want, want_arg = R.segment_max_ref(x, ptr)
    xt, pt, dt = _t(x), _t(ptr), _t(dout)
    out, arg = _segment_max_abi(xt, pt)
    assert _bits_equal(_np(out), want) and np.array_equal(_np(arg), want_arg)
    assert np.all(_np(out)[2] == 0) and np.all(_np(arg)[2] == -1)
    dx = _nan(*x.shape)
    L.check(L.lib().t2p_segment_max_backward(p(dt), p(arg), p(pt), len(ptr) - 1, c, p(dx), st), "t2p_segment_max_backward")
    assert not np.isnan(_np(dx)).any()
    assert _bits_equal(_np(dx), R.segment_max_backward_ref(dout, want_arg, len(x)))


@pytest.mark.parametrize("c", R.SEG_CHANNELS)
@pytest.mark.parametrize("covers", [False, True])
def test_segment_max_wrapper_backward(c, covers):
    """Through train_ops.segment_max: with a seg_ptr that starts at row 3 and ends 2 rows early (covers_all_rows=False) the rows
    outside the segments get exactly 0; with a tiling one and covers_all_rows=True the result is the same copy."""
    from text2pos_amd import train_ops as TO
    x, dout, ptr = R.seg_inputs(c) if covers else R.seg_inputs(c, 3, 2)
    want, want_arg = R.segment_max_ref(x, ptr)
    xt = _t(x).requires_grad_(True)
    out = TO.segment_max(xt, _t(ptr), covers_all_rows=covers)
    out.backward(_t(dout))
    assert _bits_equal(_np(out), want)
    got = _np(xt.grad)
    assert _bits_equal(got, R.segment_max_backward_ref(dout, want_arg, len(x)))
    if not covers:
        assert np.all(got[:3] == 0) and np.all(got[-2:] == 0)


def test_segment_max_keeps_nan_and_minus_inf():
    """As torch.max / scatter 'amax': a NaN in a column makes out NaN for that segment (arg: the first NaN row), a column that is all
    -inf gives -inf with arg = the segment's first row."""
    c = 67
    x, _, ptr = R.seg_inputs(c)
    x = x.copy()
    big, mid, one = int(ptr[6]), int(ptr[3]), int(ptr[1])
    x[big + 6, 1] = x[big + 2, 1] = np.nan                      # two NaN in row lane 2: the first one is named
    x[big, 0] = np.nan                                          # the segment's first row
    x[big + 258, 66] = np.nan                                   # its last row, last column
    x[big + 7, 2], x[big + 9, 2] = np.inf, np.nan               # NaN beats +inf
    x[mid: ptr[4], 5] = -np.inf                                 # all -inf over 33 rows
    x[one, 5] = -np.inf                                         # and in the one-row segment
    x[mid + 1, 6] = -np.inf                                     # a row lane's first row is -inf, the others are finite
    want, want_arg = R.segment_max_ref(x, ptr)
    for i in range(len(ptr) - 1):
        if ptr[i + 1] > ptr[i]:
            t = torch.tensor(x[ptr[i]: ptr[i + 1]]).max(0).values.numpy()
            assert np.array_equal(t, want[i], equal_nan=True)
    out, arg = (_np(a) for a in _segment_max_abi(_t(x), _t(ptr)))
    print("out[6, :3] =", out[6, :3], "arg - seg start =", arg[6, :3] - big, "| all -inf column: out =", out[3, 5], out[1, 5],
          "arg =", arg[3, 5] - mid, arg[1, 5] - one)
    assert np.isnan(want[6, [0, 1, 2, 66]]).all() and want[3, 5] == -np.inf and want_arg[3, 5] == mid
    assert np.array_equal(np.isnan(out), np.isnan(want))
    assert np.array_equal(out, want, equal_nan=True) and np.array_equal(arg, want_arg)


@pytest.mark.parametrize("c", R.SEG_CHANNELS)
def test_segment_mean_forward_backward_within_float64_bounds(c):
    """Forward and backward through the C ABI on a tiling seg_ptr, out and dx prefilled with NaN (the empty segment's mean is
    written as 0, every row of dx is written); two calls give identical bits."""
    L, p, st = _abi()
    x, dout, ptr = R.seg_inputs(c)
    ref, dref = R.segment_mean_ref64(x, ptr, dout)
    b, bdx = R.segment_mean_bounds(x, ptr, dout)
    s = len(ptr) - 1
    xt, pt, dt = _t(x), _t(ptr), _t(dout)
    outs, dxs = [], []
    for _ in range(2):
        out, dx = _nan(s, c), _nan(*x.shape)
        L.check(L.lib().t2p_segment_mean_forward(p(xt), p(pt), s, c, p(out), st), "t2p_segment_mean_forward")
        L.check(L.lib().t2p_segment_mean_backward(p(dt), p(pt), s, c, p(dx), st), "t2p_segment_mean_backward")
        outs.append(_np(out))
        dxs.append(_np(dx))
    assert not np.isnan(outs[0]).any() and not np.isnan(dxs[0]).any() and np.all(outs[0][2] == 0)
    _check("segment_mean", outs[0], ref, b)
    _check("segment_mean dx", dxs[0], dref, bdx)
    assert _bits_equal(outs[0], outs[1]) and _bits_equal(dxs[0], dxs[1])


@pytest.mark.parametrize("c", R.SEG_CHANNELS)
def test_segment_mean_wrapper_with_rows_outside_the_segments(c):
    from text2pos_amd import train_ops as TO
    x, dout, ptr = R.seg_inputs(c, 3, 2)
    ref, dref = R.segment_mean_ref64(x, ptr, dout)
    b, bdx = R.segment_mean_bounds(x, ptr, dout)
    xt = _t(x).requires_grad_(True)
    out = TO.segment_mean(xt, _t(ptr))
    out.backward(_t(dout))
    _check("segment_mean", _np(out), ref, b)
    _check("segment_mean dx", _np(xt.grad), dref, bdx)
    assert np.all(_np(xt.grad)[:3] == 0) and np.all(_np(xt.grad)[-2:] == 0)


# ---- the message gathers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.EDGE_CHANNELS)
def test_edge_features_forward_exact_backward_within_bounds(c):
    """Forward through the C ABI into a NaN-filled buffer: columns [0, C + 3) bit-exact (a gather and one fp32 subtraction), the pad
    columns exactly 0.  Backward through the wrapper with NaN in d_out's pad columns (never read): each element within 2 bounds of
    the float64 scatter-add - one row receives 3,000 terms -, rows that no edge names exactly 0."""
    from text2pos_amd import train_ops as TO
    L, p, st = _abi()
    x, pos, pos_c, src, dst, d_out, w = R.edge_inputs(c)
    xt, post, pct, st_, dt = _t(x), _t(pos), _t(pos_c), _t(src), _t(dst)
    out = _nan(len(src), w)
    L.check(L.lib().t2p_edge_features_forward(p(xt), p(post), p(pct), p(st_), p(dt), len(src), c, w, p(out), st),
            "t2p_edge_features_forward")
    assert _bits_equal(_np(out), R.edge_features_forward_ref(x, pos, pos_c, src, dst, w))
    xg = _t(x).requires_grad_(True)
    out2 = TO.edge_features(xg, post, pct, st_, dt)
    assert tuple(out2.shape) == (len(src), w) and torch.equal(out2.detach(), out)
    out2.backward(_t(d_out))
    ref, bound = R.edge_features_backward_ref64(d_out, src, len(x), c)
    got = _np(xg.grad)
    _check(f"edge_features dx C={c}", got, ref, bound)
    silent = np.bincount(src, minlength=len(x)) == 0
    assert silent.sum() >= 95 and np.all(got[silent] == 0)


@pytest.mark.parametrize("d", R.PAIR_DIMS)
def test_pair_features_forward_exact_backward_within_bounds(d):
    """[x[tgt] | x[src] - x[tgt]] bit-exact into a NaN-filled buffer; the atomic scatter backward (self edges, one row that 500
    targets name as their source) within 2 bounds of the float64 sums."""
    from text2pos_amd import train_ops as TO
    L, p, st = _abi()
    x, tgt, src, d_out = R.pair_inputs(d)
    xt, tt, st_ = _t(x), _t(tgt), _t(src)
    out = _nan(len(tgt), 2 * d)
    L.check(L.lib().t2p_pair_features_forward(p(xt), p(tt), p(st_), len(tgt), d, p(out), st), "t2p_pair_features_forward")
    assert _bits_equal(_np(out), R.pair_features_forward_ref(x, tgt, src))
    xg = _t(x).requires_grad_(True)
    out2 = TO.pair_features(xg, tt, st_)
    assert torch.equal(out2.detach(), out)
    out2.backward(_t(d_out))
    ref, bound = R.pair_features_backward_ref64(d_out, tgt, src, len(x))
    _check(f"pair_features dx D={d}", _np(xg.grad), ref, bound)


@pytest.mark.parametrize("n_rows,dim", R.ROWNORM_SHAPES)
def test_rownorm_backward_within_float64_bounds(n_rows, dim):
    """Row norms from 1e-3 to 1e3; an all-zero row (dy / fl32(1e-12), exactly as the clamp defines it), a row with dy = 3 x (pure
    cancellation: the bound is absolute, in |dy| / |x|) and a row with dy orthogonal to x.  dx is handed over full of NaN."""
    L, p, st = _abi()
    x, dy, special = R.rownorm_inputs(n_rows, dim)
    ref, bound = R.rownorm_backward_ref64(x, dy)
    xt, dt, dx = _t(x), _t(dy), _nan(n_rows, dim)
    L.check(L.lib().t2p_rownorm_backward(p(xt), p(dt), n_rows, dim, p(dx), st), "t2p_rownorm_backward")
    got = _np(dx)
    _check(f"rownorm_backward {n_rows}x{dim}", got, ref, bound)
    if special:
        z = special["zero"]
        assert _bits_equal(got[z], dy[z] * (np.float32(1) / np.float32(1e-12)))
        for k in ("cancel", "orthogonal"):
            print(f"  {k} row: ratio {R.worst_ratio(got[special[k]], ref[special[k]], bound[special[k]]):.3f}")
