"""The dense products under every layer - t2p_gemm / t2p_gemm_residual (k_gemm<64> and k_gemm<128>), t2p_gemm_x3, t2p_gemm_skinny,
t2p_gemm_tn, t2p_linear_wgrad_f32 - one call at a time against the float64 statements of tests/gemm_ref.py:
  * |kernel - ref64| <= 2 x bound element by element on N(0,1) inputs (the bounds are derived in gemm_ref.py), no element exempt;
  * bit equality on inputs whose result has no rounding (integers; for f16x3 also the two-plane inputs);
  * outputs prefilled with NaN, pitches larger than the widths, the pitch padding of A / dY / X filled with NaN and 1e30;
  * every element of the output buffer outside the window [c0, c0 + N) x [0, M) bit-unchanged;
  * a second call bit-identical to the first.
t2p_gemm, t2p_gemm_residual and t2p_gemm_x3 run the whole option matrix at every shape: relu x bias x layout x residual (none, a
separate buffer with ldr != ldc, aliased to C) - nothing of it is dropped for f16x3, which runs it at both weight scales.
Every test prints its largest |got - ref64| / bound before it asserts (pytest -s shows them; docs/notebook.md records a run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = R.FACTOR_GPU
F32 = np.float32
LAYOUTS = [(0, lambda n: n, lambda n: 0), (8, lambda n: 2 * n + 8, lambda n: n)]      # (lda - K, ldc(N), c0(N))
OPTIONS = [(layout, relu, use_bias, resid) for layout in (0, 1) for relu in (0, 1) for use_bias in (True, False)
           for resid in (None, "separate", "alias")]


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.tensor(np.asarray(a), device=_dev())


def _np(t):
    return t.detach().cpu().numpy()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _image(m, k, n, scale, kind):
    """pack_gemm_x3 image of the case's weight, on the device."""
    from text2pos_amd import packing
    w = dict(normal=lambda: R.gemm_inputs(m, k, n)[1], exact=lambda: R.gemm_exact_inputs(m, k, n)[1],
             two_plane=lambda: R.two_plane_inputs(m, n)[1])[kind]()
    return packing.pack_gemm_x3(torch.from_numpy(np.array(w)), scale).to(_dev())


def _case(shape, layout, relu, use_bias, resid_mode, kind="normal", bad=None):
    """Host buffers and the float64 reference of one call; bad = (row, column, value) puts a non-finite value into A."""
    m, k, n = shape
    if kind == "two_plane":
        a, w = R.two_plane_inputs(m, n)[:2]
        bias = resid = None
    else:
        a, w, bias, resid = (R.gemm_exact_inputs if kind == "exact" else R.gemm_inputs)(m, k, n)
    if bad is not None:
        a = np.array(a)
        a[bad[0], bad[1]] = bad[2]
    pad, ldc_of, c0_of = LAYOUTS[layout]
    lda, ldc, c0 = k + pad, ldc_of(n), c0_of(n)
    c = dict(m=m, k=k, n=n, relu=relu, a=a, w=w, bias=bias if use_bias else None, resid=None, lda=lda, ldc=ldc, c0=c0,
             a_buf=R.pitched(a, lda), c_buf=R.nan_buffer(m + 2, ldc), r_buf=None, ldr=0, r_first=0, alias=False, kind=kind)
    if resid_mode == "separate":
        c.update(resid=resid, ldr=n + 4, r_buf=R.pitched(resid, n + 4))
    elif resid_mode == "alias":
        c["c_buf"][:m, c0: c0 + n] = resid
        c.update(resid=resid, ldr=ldc, r_first=c0, alias=True)
    c["ref"] = R.two_plane_inputs(m, n)[2] if kind == "two_plane" else R.gemm_ref64(a, w, c["bias"], relu, c["resid"])["out"]
    c["act"] = None if kind == "two_plane" else R.gemm_ref64(a, w, c["bias"], relu, None)["out"]
    return c


def _bound(c, scale=None):
    ref = dict(act=c["act"], out=c["ref"])
    if scale is None:
        return R.gemm_bound(c["a"], c["w"], c["bias"], ref, c["resid"])
    return R.x3_bound(c["a"], c["w"], scale, c["bias"], ref, c["resid"])


def _call(c, scale=None, rows=None, want_amax=False):
    """One call on fresh device buffers; returns (the whole C buffer afterwards, the guard word or None).  scale None: the fp32
    kernel - through t2p_gemm itself when there is no residual, else t2p_gemm_residual."""
    from text2pos_amd import _lib as L
    from text2pos_amd import ops
    m = c["m"] if rows is None else rows
    a, w, bias, out = _t(c["a_buf"]), _t(c["w"]), _t(c["bias"]), _t(c["c_buf"])
    resid = out if c["alias"] else _t(c["r_buf"])
    amax = torch.zeros(1, dtype=torch.int32, device=_dev()) if want_amax else None
    if scale is not None:
        kind = c["kind"]
        ops.gemm_x3(a, c["lda"], _image(c["m"], c["k"], c["n"], scale, kind), scale, bias, out, c["ldc"], c["c0"], m, c["k"], c["n"],
                    bool(c["relu"]), resid, c["ldr"], c["r_first"], amax)
    elif resid is None:
        L.check(L.lib().t2p_gemm(ops._ptr(a), c["lda"], ops._ptr(w), ops._ptr(bias), ops._ptr(out), c["ldc"], c["c0"], m, c["k"], c["n"],
                                 c["relu"], ops._stream(_dev())), "t2p_gemm")
    else:
        ops.gemm_residual(a, c["lda"], w, bias, out, c["ldc"], c["c0"], m, bool(c["relu"]), resid, c["ldr"], c["r_first"])
    torch.cuda.synchronize()
    return _np(out), (int(amax.item()) if want_amax else None)


def _check_case(c, scale=None, label=""):
    """Two calls; the contract of the output buffer; returns error / bound of the worst element (0 for the exact kinds)."""
    want_amax = scale is not None and c["relu"] == 1        # (half of the f16x3 calls hand in a guard word, the others NULL)
    got, amax = _call(c, scale, want_amax=want_amax)
    again, amax2 = _call(c, scale, want_amax=want_amax)
    assert R.bits_equal(got, again) and amax == amax2, (label, "second call differs")
    m, n, c0 = c["m"], c["n"], c["c0"]
    exact = c["kind"] != "normal"
    bound = None if exact else _bound(c, scale)
    ratio = 0.0 if exact else R.worst_ratio(got[:m, c0: c0 + n], c["ref"], bound)
    ok, why = R.check_window(got, c["c_buf"], m, n, c0, c["ref"], bound, FACTOR, exact=exact)
    assert ok, (label, why)
    if want_amax:   # the exact maximum of |A| over [M][K], whatever the padding holds
        assert amax == int(np.abs(c["a"]).max().view(np.int32)), (label, "amax_in")
    return ratio


def _options_sweep(shape, scale=None):
    worst = 0.0
    for opt in OPTIONS:
        for kind in ("normal", "exact"):
            worst = max(worst, _check_case(_case(shape, *opt, kind=kind), scale, label=(shape, scale, opt, kind)))
    return worst


@pytest.mark.parametrize("shape", R.GEMM_SHAPES)
def test_gemm_fp32_option_matrix_within_float64_bound(shape):
    """t2p_gemm (no residual) and t2p_gemm_residual: relu x bias x (lda, ldc, c0) x residual, N(0,1) and integer inputs."""
    assert R.gemm_tile(shape[0], shape[2], _cus()) == 64
    print(f"ratio gemm fp32 {shape}: {_options_sweep(shape):.3f}")


@pytest.mark.parametrize("scale", R.X3_SCALES)
@pytest.mark.parametrize("shape", R.GEMM_SHAPES)
def test_gemm_x3_option_matrix_within_float64_bound(shape, scale):
    """t2p_gemm_x3 with the weights drawn through pack_gemm_x3: the same matrix; the guard word on the relu = 1 half, NULL on the other;
    the two-plane inputs pin hi.hi + hi.lo + lo.hi and the absence of lo.lo bit for bit."""
    print(f"ratio gemm x3 {shape} scale {scale:g}: {_options_sweep(shape, scale):.3f}")
    m, _, n = shape
    for layout in (0, 1):
        _check_case(_case((m, 32, n), layout, 0, False, None, kind="two_plane"), scale, label=(shape, scale, "two-plane"))


@pytest.mark.parametrize("scale", [None] + R.X3_SCALES)
def test_gemm_tile_choice_128_and_64_give_the_same_bits(scale):
    """M = 2,100 x N = 1,024 is 17 x 8 tiles of 128: the 128 x 128 kernel on any chip below 272 CUs; its first 300 rows alone take
    the 64 x 64 kernel.  Both sides of the dispatch are computed from the device's CU count with the launcher's formula and must
    differ, then the rows the two calls share must agree bit for bit; bounds and exact inputs at this shape as everywhere."""
    m, k, n = R.TILE_SHAPE
    big, small = R.gemm_tile(m, n, _cus()), R.gemm_tile(R.TILE_SMALL_ROWS, n, _cus())
    assert (big, small) == (128, 64), f"{_cus()} CUs select {big} / {small}: this shape no longer separates the two kernels"
    worst = 0.0
    for opt in [(1, 1, True, "alias"), (0, 0, False, None), (1, 0, True, "separate"), (0, 1, True, None)]:
        for kind in ("normal", "exact"):
            c = _case(R.TILE_SHAPE, *opt, kind=kind)
            worst = max(worst, _check_case(c, scale, label=("tile", scale, opt, kind)))
            full, _ = _call(c, scale)
            part, _ = _call(c, scale, rows=R.TILE_SMALL_ROWS)
            c0 = c["c0"]
            assert R.bits_equal(full[: R.TILE_SMALL_ROWS, c0: c0 + n], part[: R.TILE_SMALL_ROWS, c0: c0 + n]), (scale, opt, kind)
            keep = np.ones(part.shape, bool)
            keep[: R.TILE_SMALL_ROWS, c0: c0 + n] = False
            assert np.array_equal(R.bits(part)[keep], R.bits(c["c_buf"])[keep])     # rows 300.. of the short call: untouched
    if scale is not None:
        _check_case(_case((m, 32, n), 1, 0, False, None, kind="two_plane"), scale, label=("tile", scale, "two-plane"))
    print(f"ratio gemm tile 128 {'fp32' if scale is None else 'x3 scale %g' % scale}: {worst:.3f}")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("shape", [(65, 20, 40), (129, 64, 256)])
def test_gemm_fp32_nonfinite_input_reaches_its_row_only(shape, value, relu):
    """A NaN or an infinity in A[r][j]: row r of C is what float64 says (NaN, or +-inf by the sign of W[j][n]; under ReLU the
    statement is torch.relu, which keeps NaN and turns -inf into 0), every other row is bit-equal to the clean call."""
    r, j = shape[0] // 2, shape[1] - 3
    for opt in [(1, relu, True, None), (0, relu, False, "separate")]:
        clean = _case(shape, *opt)
        dirty = _case(shape, *opt, bad=(r, j, value))
        got, _ = _call(dirty)
        base, _ = _call(clean)
        ok, why = R.check_window(got, dirty["c_buf"], dirty["m"], dirty["n"], dirty["c0"], dirty["ref"], _bound(dirty), FACTOR)
        assert ok, (shape, value, opt, why)
        row = got[r, dirty["c0"]: dirty["c0"] + dirty["n"]]
        if not relu:
            assert not np.isfinite(row).any()
        if np.isnan(value):
            assert np.isnan(row).all(), "a NaN activation must stay NaN (relu keeps NaN)"
        others = np.arange(shape[0]) != r
        assert R.bits_equal(got[: shape[0]][others], base[: shape[0]][others])


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", [(65, 20, 40), (129, 64, 256)])
def test_gemm_x3_nonfinite_input_reaches_its_row_only(shape, relu):
    """f16x3: a NaN in A[r][j] makes row r NaN (with and without ReLU) and leaves every other row's bits alone.  An infinity is
    past the fp16 range that the guard word watches: hi = inf, lo = fp16(inf - inf) = NaN, so its row is NaN too (include/t2p.h),
    and the guard word reports the infinity."""
    r, j = shape[0] // 2, shape[1] - 3
    inf_bits = int(np.array(np.inf, F32).view(np.int32))
    for value in (float("nan"), float("inf")):
        clean = _case(shape, 1, relu, True, None)
        dirty = _case(shape, 1, relu, True, None, bad=(r, j, value))
        got, amax = _call(dirty, 1024.0, want_amax=True)
        base, _ = _call(clean, 1024.0)
        c0, n = dirty["c0"], dirty["n"]
        want = np.array(clean["ref"])
        want[r] = np.nan
        ok, why = R.check_window(got, dirty["c_buf"], dirty["m"], n, c0, want, _bound(clean, 1024.0), FACTOR)
        assert ok, (shape, value, relu, why)
        assert np.isnan(got[r, c0: c0 + n]).all()
        others = np.arange(shape[0]) != r
        assert R.bits_equal(got[: shape[0]][others], base[: shape[0]][others])
        if np.isinf(value):
            assert amax == inf_bits


@pytest.mark.parametrize("shape", R.SKINNY_SHAPES)
def test_gemm_skinny_within_float64_bound(shape):
    """t2p_gemm_skinny with lda > K and ldc > N: K = 8 i + 4 (the masked lane half; K = 4 included), N = 1 and N % 32 != 0
    (col_ok), M % 32 != 0 and M > 64 (row_ok, two row blocks), the LSTM's own two shapes."""
    from text2pos_amd import ops
    m, k, n = shape
    lda, ldc = k + 4, n + 3
    for kind in ("normal", "exact"):
        a, w, _, _ = (R.gemm_exact_inputs if kind == "exact" else R.gemm_inputs)(m, k, n)
        a_buf, c_buf = R.pitched(a, lda), R.nan_buffer(m + 2, ldc)
        ref = R.gemm_ref64(a, w)
        bound = R.gemm_bound(a, w, None, ref)
        outs = []
        for _ in range(2):
            out = _t(c_buf)
            ops.gemm_skinny(_t(a_buf), lda, _t(w), out, ldc, m)
            torch.cuda.synchronize()
            outs.append(_np(out))
        assert R.bits_equal(outs[0], outs[1])
        if kind == "normal":
            print(f"ratio gemm skinny {shape}: {R.worst_ratio(outs[0][:m, :n], ref['out'], bound):.3f}")
        ok, why = R.check_window(outs[0], c_buf, m, n, 0, ref["out"], bound, FACTOR, exact=kind == "exact")
        assert ok, (shape, kind, why)


def _tn_call(a_buf, b_buf, c_buf, m, k1, n):
    from text2pos_amd import _lib as L
    from text2pos_amd import ops
    a, b, out = _t(a_buf), _t(b_buf), _t(c_buf)
    ws = torch.empty((L.lib().t2p_gemm_tn_workspace_bytes(m, k1, n),), dtype=torch.uint8, device=_dev())
    if m > 0:
        ops.gemm_tn(a[:m], b[:m], k1=k1, n=n, out=out[:k1])
    else:   # the wrapper answers an empty product itself: the kernels' own answer comes from the C ABI
        L.check(L.lib().t2p_gemm_tn(ops._ptr(a), a_buf.shape[1], ops._ptr(b), b_buf.shape[1], ops._ptr(out), c_buf.shape[1], 0, k1, n,
                                    ops._ptr(ws), ws.numel(), ops._stream(_dev())), "t2p_gemm_tn")
    torch.cuda.synchronize()
    return _np(out)


@pytest.mark.parametrize("shape", R.TN_SHAPES)
def test_gemm_tn_within_float64_bound(shape):
    """t2p_gemm_tn with padded lda, ldb, ldc: one row, partly filled 64 x 64 tiles, K1 % 4 != 0, 47 and 16 row splits, no rows."""
    m, k1, n = shape
    lda, ldb, ldc = k1 + 5, n + 3, n + 2
    for kind in ("normal", "exact"):
        a, b = (R.tn_exact_inputs if kind == "exact" else R.tn_inputs)(m, k1, n)
        a_buf, b_buf, c_buf = R.pitched(a, lda, 1), R.pitched(b, ldb, 1), R.nan_buffer(k1 + 1, ldc)
        ref = R.tn_ref64(a, b)
        bound = R.tn_bound(a, b, ref)
        got, again = _tn_call(a_buf, b_buf, c_buf, m, k1, n), _tn_call(a_buf, b_buf, c_buf, m, k1, n)
        assert R.bits_equal(got, again)
        if kind == "normal":
            print(f"ratio gemm_tn {shape} splits {R.tn_splits(m, k1, n, _cus())}: {R.worst_ratio(got[:k1, :n], ref, bound):.4f}")
        ok, why = R.check_window(got, c_buf, k1, n, 0, ref, bound, FACTOR, exact=kind == "exact")
        assert ok, (shape, kind, why)


def _wgrad_rows(widths, m):
    from text2pos_amd import ops
    k1, n = widths
    lda, ldb, ldc = (k1 + 3) // 4 * 4 + 4, (n + 3) // 4 * 4 + 8, n + 3
    worst = (0.0, 0.0)
    for kind in ("normal", "exact"):
        dy, x = (R.tn_exact_inputs if kind == "exact" else R.tn_inputs)(m, k1, n)
        dy_buf, x_buf, c_buf = R.pitched(dy, lda, 1), R.pitched(x, ldb, 1), R.nan_buffer(k1 + 1, ldc)
        ref, cref = R.tn_ref64(dy, x), R.colsum_ref64(dy)
        bound, cbound = R.tn_bound(dy, x, ref), R.colsum_bound(dy, cref)
        runs = []
        for _ in range(2):
            out = _t(c_buf)
            _, cs = ops.linear_wgrad(_t(dy_buf)[:m], _t(x_buf)[:m], True, k1=k1, n=n, out=out[:k1])
            torch.cuda.synchronize()
            runs.append((_np(out), _np(cs)))
        assert R.bits_equal(runs[0][0], runs[1][0]) and R.bits_equal(runs[0][1], runs[1][1])
        got, cs = runs[0]
        ok, why = R.check_window(got, c_buf, k1, n, 0, ref, bound, FACTOR, exact=kind == "exact")
        assert ok, (widths, m, kind, why)
        if kind == "exact":
            assert R.bits_equal(cs, cref.astype(F32)), (widths, m, "colsum")
        else:
            worst = (R.worst_ratio(got[:k1, :n], ref, bound), R.worst_ratio(cs, cref, cbound))
            assert R.within(cs, cref, cbound, FACTOR), (widths, m, "colsum", worst)
            out = _t(c_buf)
            dw, none = ops.linear_wgrad(_t(dy_buf)[:m], _t(x_buf)[:m], False, k1=k1, n=n, out=out[:k1])
            torch.cuda.synchronize()
            assert none is None and R.bits_equal(_np(out), got)
    return worst


def _library_slots(m, k1, n):
    """splits * n_phase of the plan the launcher itself makes on this device: its workspace is slots * (K1 N + 2 K1) floats + 256.
    This ties gemm_ref.wgrad_plan - a restatement that follows csrc/train_gemm.hip::wgrad_plan by hand - to the library at every
    shape; the tile plan itself (tpw, ktp, ntp) is not exported, so tests/test_gemm_ref_host.py pins its rules to the source text."""
    from text2pos_amd import _lib as L
    nbytes = L.lib().t2p_linear_wgrad_workspace_bytes(m, k1, n) - 256
    assert nbytes % (4 * (k1 * n + 2 * k1)) == 0
    return nbytes // (4 * (k1 * n + 2 * k1))


@pytest.mark.parametrize("widths", list(R.WGRAD_WIDTHS))
def test_linear_wgrad_every_tile_plan_within_float64_bound(widths):
    """t2p_linear_wgrad_f32 at widths that select every TPW from 1 to 8, ntp in {1, 2, 4} and n_phase in {1, 2, 4, 8} (the plan is
    restated in gemm_ref.py, pinned to the shape table and the source text by the host test and to the library's slot count here), M in {1, 33, 3001}, padded pitches; dW and the column
    sums against float64, each under its own bound; want_colsum=False returns None and the same dW."""
    for m in R.WGRAD_ROWS:
        p = R.wgrad_plan(m, *widths, _cus())
        assert (p["tpw"], p["ktp"], p["ntp"], p["n_phase"]) == R.WGRAD_WIDTHS[widths] and not p["wave_reduce"], p
        assert p["slots"] == _library_slots(m, *widths), (widths, m, p)
        worst = _wgrad_rows(widths, m)
        print(f"ratio wgrad {widths} M={m} tpw={p['tpw']} ktp={p['ktp']} ntp={p['ntp']} n_phase={p['n_phase']} slots={p['slots']}: "
              f"dW {worst[0]:.4f} colsum {worst[1]:.4f}")


def test_linear_wgrad_wave_reduce_within_float64_bound():
    """(20000, 32, 8): 288 outputs from at least 128 slots, the shape of k_wgrad_reduce_wave."""
    m, k1, n = R.WGRAD_WAVE_SHAPE
    p = R.wgrad_plan(m, k1, n, _cus())
    assert p["wave_reduce"] and p["n_phase"] == 8 and p["slots"] == _library_slots(m, k1, n) >= 128, p
    worst = _wgrad_rows((k1, n), m)
    print(f"ratio wgrad wave reduce {R.WGRAD_WAVE_SHAPE} slots={p['slots']}: dW {worst[0]:.4f} colsum {worst[1]:.4f}")
