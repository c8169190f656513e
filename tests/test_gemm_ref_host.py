"""CPU checks of tests/gemm_ref.py, the yardstick of tests/test_gpu_gemm_family.py: the NumPy emulation of every GEMM kernel stays
within 1 x its bound of the float64 statement at every shape of the GPU test, the exact inputs are exact in any summation order,
`check_window` rejects each deliberately wrong kernel at one or more of those shapes, the restated weight-gradient plan selects
the branches the shape table intends, and the new C-ABI entry points refuse bad arguments before anything is launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

F32 = np.float32
# (lda - K, ldc as a function of N, c0 as a function of N): the two layouts of the GPU test
LAYOUTS = [(0, lambda n: n, lambda n: 0), (8, lambda n: 2 * n + 8, lambda n: n)]


def _gemm_case(shape, layout, relu, use_bias, resid_mode, exact=False, inputs=None):
    """Buffers and references of one t2p_gemm_residual / t2p_gemm_x3 call, as the GPU test builds them."""
    m, k, n = shape
    a, w, bias, resid = inputs if inputs is not None else (R.gemm_exact_inputs if exact else R.gemm_inputs)(m, k, n)
    pad, ldc_of, c0_of = LAYOUTS[layout]
    lda, ldc, c0 = k + pad, ldc_of(n), c0_of(n)
    a_buf, c_buf = R.pitched(a, lda), R.nan_buffer(m + 2, ldc)
    r_buf, ldr, r_first, res = None, 0, 0, None
    if resid_mode == "separate":
        ldr = n + 4
        r_buf, res = R.pitched(resid, ldr), resid
    elif resid_mode == "alias":
        c_buf[:m, c0: c0 + n] = resid
        r_buf, ldr, r_first, res = c_buf, ldc, c0, resid
    b = bias if use_bias else None
    ref = R.gemm_ref64(a, w, b, relu, res)
    return dict(a=a, w=w, bias=b, resid=res, a_buf=a_buf, lda=lda, c_buf=c_buf, ldc=ldc, c0=c0, r_buf=r_buf, ldr=ldr, r_first=r_first,
                ref=ref, m=m, k=k, n=n, relu=relu)


def _run_gemm(c, tile=64, wrong=None):
    return R.gemm_emul(c["a_buf"], c["lda"], c["w"], c["bias"], c["c_buf"], c["ldc"], c["c0"], c["m"], c["k"], c["n"], c["relu"],
                       c["r_buf"], c["ldr"], c["r_first"], tile=tile, wrong=wrong)


def _run_x3(c, scale, wrong=None):
    return R.x3_emul(c["a_buf"], c["lda"], c["w"], scale, c["bias"], c["c_buf"], c["ldc"], c["c0"], c["m"], c["k"], c["n"], c["relu"],
                     c["r_buf"], c["ldr"], c["r_first"], wrong=wrong)


def _ok(c, after, bound=None, factor=1.0, exact=False):
    return R.check_window(after, c["c_buf"], c["m"], c["n"], c["c0"], c["ref"]["out"], bound, factor, exact=exact)


OPTIONS = [(layout, relu, use_bias, resid) for layout in (0, 1) for relu in (0, 1) for use_bias in (True, False)
           for resid in (None, "separate", "alias")]
# the big shape takes a second per emulation: the host test runs the options that differ in kind there, the GPU test runs all
OPTIONS_BIG = [(1, 1, True, "alias"), (0, 0, False, None), (1, 0, True, "separate")]


@pytest.mark.parametrize("shape", R.GEMM_SHAPES + [R.TILE_SHAPE])
def test_gemm_emulation_within_bound_and_exact_case_exact(shape):
    worst = 0.0
    for layout, relu, use_bias, resid in (OPTIONS if shape[0] * shape[1] * shape[2] < 10 ** 7 else OPTIONS_BIG):
        c = _gemm_case(shape, layout, relu, use_bias, resid)
        bound = R.gemm_bound(c["a"], c["w"], c["bias"], c["ref"], c["resid"])
        after = _run_gemm(c, R.gemm_tile(shape[0], shape[2]))
        ok, why = _ok(c, after, bound)
        assert ok, (shape, layout, relu, use_bias, resid, why)
        worst = max(worst, R.worst_ratio(after[: c["m"], c["c0"]: c["c0"] + c["n"]], c["ref"]["out"], bound))
        e = _gemm_case(shape, layout, relu, use_bias, resid, exact=True)
        assert R.exact_headroom(e["a"], e["w"], e["bias"], e["resid"]) < 2.0 ** 18
        ok, why = _ok(e, _run_gemm(e), exact=True)
        assert ok, (shape, layout, relu, use_bias, resid, why)
    print(f"gemm {shape}: emulation worst ratio {worst:.3f}")
    assert worst > 0.0 or shape == (1, 4, 8)


def test_exact_inputs_are_exact_in_any_order():
    """fp32 sequential sums of the products, forwards, backwards and in three shuffled orders, equal the float64 sum."""
    rng = np.random.default_rng(7)
    for m, k, n in [(65, 20, 40), (9, 256, 16), (5, 1024, 8)]:
        a, w, bias, _ = R.gemm_exact_inputs(m, k, n)
        want = a.astype(np.float64) @ w.astype(np.float64)
        terms = a[:, :, None].astype(np.float64) * w[None, :, :].astype(np.float64)
        assert np.array_equal(terms, (a[:, :, None] * w[None, :, :]).astype(np.float64))       # the fp32 products are exact
        for order in [np.arange(k), np.arange(k)[::-1]] + [rng.permutation(k) for _ in range(3)]:
            acc = np.zeros((m, n), F32)
            for kk in order:
                acc = (acc + terms[:, kk, :].astype(F32)).astype(F32)
            assert np.array_equal(acc.astype(np.float64), want)
    # the reduction over rows of the transposed products, at the longest M of the GPU test
    a, b = R.tn_exact_inputs(20000, 4, 8)
    assert R.exact_headroom(a.T, b) < 2.0 ** 18
    acc = np.zeros((4, 8), F32)
    for r in rng.permutation(20000):
        acc = (acc + a[r][:, None] * b[r][None, :]).astype(F32)
    assert np.array_equal(acc.astype(np.float64), R.tn_ref64(a, b))
    assert np.array_equal(np.add.accumulate(a, 0, dtype=F32)[-1].astype(np.float64), R.colsum_ref64(a))


@pytest.mark.parametrize("scale", R.X3_SCALES)
def test_exact_inputs_have_zero_lo_planes_and_two_plane_split_is_as_stated(scale):
    for m, k, n in R.GEMM_SHAPES[:3]:
        a, w, _, _ = R.gemm_exact_inputs(m, k, n)
        for x in (a.astype(np.float64), w.astype(np.float64) * scale):
            hi, lo = R.split_f16(x)
            assert np.array_equal(hi, x) and not lo.any()
    a, w, want, mag = R.two_plane_inputs(65, 40)
    assert a.shape[1] == 32 and mag.max() < 2048.0               # every partial sum of multiples of 2^-13 below 2^11: exact in fp32
    assert np.array_equal(want.astype(F32).astype(np.float64), want)
    for x, s in ((a.astype(np.float64), 1.0), (w.astype(np.float64), scale)):
        hi, lo = R.split_f16(x * s)
        p = np.rint(x)
        assert np.array_equal(hi, p * s) and np.array_equal(lo, (x - p) * s) and np.abs(lo).max() > 0
        assert np.array_equal(hi + lo, x * s)
    # (the construction needs |p| >= 4: with p = 1, q = 8 the sum is an fp16 number and the split is hi = a, lo = 0)
    hi, lo = R.split_f16(np.array([1.0 + 8 * 2.0 ** -13]))
    assert hi[0] != 1.0 and lo[0] == 0.0


def test_pack_gemm_x3_is_the_split_the_emulation_uses():
    import torch
    import text2pos_amd  # noqa: F401
    from text2pos_amd import packing
    for scale in R.X3_SCALES:
        _, w, _, _ = R.gemm_inputs(65, 20, 40)
        img = packing.pack_gemm_x3(torch.from_numpy(np.array(w)), scale).view(torch.float16).numpy().astype(np.float64)
        hi, lo = R.split_f16(w.astype(np.float64) * scale)
        assert img.shape == (2, 40, 32) and not img[:, :, 20:].any()
        assert np.array_equal(img[0, :, :20], hi.T) and np.array_equal(img[1, :, :20], lo.T)


@pytest.mark.parametrize("scale", R.X3_SCALES)
@pytest.mark.parametrize("shape", R.GEMM_SHAPES + [R.TILE_SHAPE])
def test_x3_emulation_within_bound_and_exact_cases_exact(shape, scale):
    worst = 0.0
    for layout, relu, use_bias, resid in (OPTIONS if shape[0] * shape[1] * shape[2] < 10 ** 7 else OPTIONS_BIG):
        c = _gemm_case(shape, layout, relu, use_bias, resid)
        bound = R.x3_bound(c["a"], c["w"], scale, c["bias"], c["ref"], c["resid"])
        after, amax = _run_x3(c, scale)
        ok, why = _ok(c, after, bound)
        assert ok, (shape, layout, relu, use_bias, resid, why)
        assert amax == int(np.abs(c["a"]).max().view(np.int32))
        worst = max(worst, R.worst_ratio(after[: c["m"], c["c0"]: c["c0"] + c["n"]], c["ref"]["out"], bound))
        e = _gemm_case(shape, layout, relu, use_bias, resid, exact=True)
        ok, why = _ok(e, _run_x3(e, scale)[0], exact=True)
        assert ok, (shape, layout, relu, use_bias, resid, why)
    print(f"x3 {shape} scale {scale}: emulation worst ratio {worst:.3f}")
    m, _, n = shape
    a, w, want, _ = R.two_plane_inputs(m, n)
    c = _gemm_case((m, 32, n), 1, 0, False, None, inputs=(a, w, None, None))
    c["ref"] = dict(out=want)
    ok, why = _ok(c, _run_x3(c, scale)[0], exact=True)
    assert ok, why


def _rejected(case, runs, wrong, bound_of):
    """True when check_window refuses the wrong kernel on the N(0,1) inputs at 2 x bound (what the GPU test asserts)."""
    after = runs(case, wrong)
    after = after[0] if isinstance(after, tuple) else after
    return not _ok(case, after, bound_of(case), R.FACTOR_GPU)[0]


def test_checker_rejects_each_wrong_gemm_kernel():
    gb = lambda c: R.gemm_bound(c["a"], c["w"], c["bias"], c["ref"], c["resid"])  # noqa: E731
    run = lambda c, wrong: _run_gemm(c, 64, wrong)  # noqa: E731
    shapes = R.GEMM_SHAPES[:3]
    caught = {w: [] for w in ("last_k_chunk", "last_row_pair", "bias_no_n0", "c0_ignored", "resid_ldc")}
    for shape in shapes:
        for wrong in caught:
            c = _gemm_case(shape, 1, 1, True, "separate")
            assert _ok(c, run(c, None), gb(c), 1.0)[0]
            if _rejected(c, run, wrong, gb):
                caught[wrong].append(shape)
    print("wrong fp32 kernels rejected at:", caught)
    assert caught["last_k_chunk"] == [(1, 4, 8), (65, 20, 40)]            # K % 16 != 0
    assert caught["last_row_pair"] == shapes                               # every M is odd
    assert caught["bias_no_n0"] == [(129, 64, 256)]                        # more than one column tile
    assert caught["c0_ignored"] == shapes
    assert caught["resid_ldc"] == [(65, 20, 40), (129, 64, 256)]           # more than one row
    # with c0 = 0 and ldr = ldc the last two are no bugs at all: the (K, N, 0) layout alone would not see them
    c = _gemm_case((65, 20, 40), 0, 1, True, "alias")
    assert not _rejected(c, run, "c0_ignored", gb) and not _rejected(c, run, "resid_ldc", gb)


def test_checker_rejects_each_wrong_x3_kernel():
    caught = {w: [] for w in ("no_lo_hi", "no_hi_lo", "lolo", "no_scale")}
    for scale in R.X3_SCALES:
        xb = lambda c: R.x3_bound(c["a"], c["w"], scale, c["bias"], c["ref"], c["resid"])  # noqa: E731
        run = lambda c, wrong: _run_x3(c, scale, wrong)  # noqa: E731
        for shape in R.GEMM_SHAPES[1:3]:
            for wrong in caught:
                c = _gemm_case(shape, 1, 0, True, None)
                if _rejected(c, run, wrong, xb):
                    caught[wrong].append((shape, scale, "bound"))
                m, _, n = shape
                a, w, want, _ = R.two_plane_inputs(m, n)
                t = _gemm_case((m, 32, n), 1, 0, False, None, inputs=(a, w, None, None))
                t["ref"] = dict(out=want)
                if not _ok(t, run(t, wrong)[0], exact=True)[0]:
                    caught[wrong].append((shape, scale, "two-plane"))
    print("wrong x3 kernels rejected at:", caught)
    for wrong in ("no_lo_hi", "no_hi_lo"):
        assert len([c for c in caught[wrong] if c[2] == "bound"]) == 4 and len([c for c in caught[wrong] if c[2] == "two-plane"]) == 4
    # the dropped lo.lo product is inside the bound by construction: only the two-plane case sees a kernel that adds it
    assert [c for c in caught["lolo"] if c[2] == "bound"] == [] and len([c for c in caught["lolo"] if c[2] == "two-plane"]) == 4
    assert ((65, 20, 40), 1024.0, "bound") in caught["no_scale"] and all(c[1] == 1024.0 for c in caught["no_scale"])


@pytest.mark.parametrize("shape", R.SKINNY_SHAPES)
def test_skinny_emulation_within_bound_and_wrong_kernel_rejected(shape):
    m, k, n = shape
    lda, ldc = k + 4, n + 3
    for exact in (True, False):
        a, w, _, _ = (R.gemm_exact_inputs if exact else R.gemm_inputs)(m, k, n)
        a_buf, c_buf = R.pitched(a, lda), R.nan_buffer(m + 2, ldc)
        ref = R.gemm_ref64(a, w)
        bound = R.gemm_bound(a, w, None, ref)
        after = R.skinny_emul(a_buf, lda, w, c_buf, ldc, m, k, n)
        ok, why = R.check_window(after, c_buf, m, n, 0, ref["out"], bound, 1.0, exact=exact)
        assert ok, (shape, exact, why)
    print(f"skinny {shape}: emulation worst ratio {R.worst_ratio(after[:m, :n], ref['out'], bound):.3f}")
    bad = R.skinny_emul(a_buf, lda, w, c_buf, ldc, m, k, n, wrong="upper_half")
    assert R.check_window(bad, c_buf, m, n, 0, ref["out"], bound, R.FACTOR_GPU)[0] == (k % 8 == 0), shape


@pytest.mark.parametrize("shape", R.TN_SHAPES)
def test_tn_emulation_within_bound_and_wrong_kernel_rejected(shape):
    m, k1, n = shape
    lda, ldb, ldc = k1 + 5, n + 3, n + 2
    cols = None if m * k1 * n < 10 ** 8 else np.r_[0:40, n - 40: n]     # the largest shape: 80 of its 1,024 columns
    caught = False
    for exact in (True, False):
        a, b = (R.tn_exact_inputs if exact else R.tn_inputs)(m, k1, n)
        a_buf, b_buf, c_buf = R.pitched(a, lda, 1), R.pitched(b, ldb, 1), R.nan_buffer(k1 + 1, ldc)
        ref = R.tn_ref64(a, b)
        bound = R.tn_bound(a, b, ref)
        rest = np.arange(0) if cols is None else np.setdiff1d(np.arange(n), cols)
        for wrong in (None, "split_missing"):
            after = R.tn_emul(a_buf, lda, b_buf, ldb, c_buf, ldc, m, k1, n, cols=cols, wrong=wrong)
            after[:k1, rest] = ref[:, rest].astype(F32)                  # columns that were not emulated: taken from the reference
            ok, why = R.check_window(after, c_buf, k1, n, 0, ref, bound, R.FACTOR_GPU if wrong else 1.0, exact=exact)
            if wrong:
                caught |= not ok
            else:
                assert ok, (shape, exact, why)
                ratio = R.worst_ratio(after[:k1, :n], ref, bound)
    print(f"tn {shape}: splits {R.tn_splits(m, k1, n)}, emulation worst ratio {ratio:.4f}")
    assert caught == (R.tn_splits(m, k1, n) > 1), shape


def _library_slots(m, k1, n):
    """splits * n_phase as the library's own wgrad_plan has it: t2p_linear_wgrad_workspace_bytes is slots * (K1 N + 2 K1) floats + 256."""
    import text2pos_amd  # noqa: F401
    from text2pos_amd import _lib
    nbytes = _lib.lib().t2p_linear_wgrad_workspace_bytes(m, k1, n) - 256
    assert nbytes % (4 * (k1 * n + 2 * k1)) == 0
    return nbytes // (4 * (k1 * n + 2 * k1))


def _library_cus():
    """The CU count the library plans with: the device's, or 256 where there is none (csrc/api.hip::num_cus)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def test_wgrad_plan_selects_the_intended_branches():
    """The restatement gemm_ref.wgrad_plan against the shape table, against the library's own plan (through the workspace size, which
    is slots * (K1 N + 2 K1) floats) and against the source text of the branch rules."""
    seen = dict(tpw=set(), ntp=set(), n_phase=set(), ktp=set())
    for (k1, n), want in R.WGRAD_WIDTHS.items():
        for m in R.WGRAD_ROWS:
            p = R.wgrad_plan(m, k1, n)
            assert (p["tpw"], p["ktp"], p["ntp"], p["n_phase"]) == want, ((k1, n), p)
            assert not p["wave_reduce"], ((k1, n), m, p)
            assert R.wgrad_plan(m, k1, n, _library_cus())["slots"] == _library_slots(m, k1, n), ((k1, n), m)
            for key in seen:
                seen[key].add(p[key])
    assert seen["tpw"] == set(range(1, 9)) and seen["ntp"] == {1, 2, 4} and seen["n_phase"] == {1, 2, 4, 8} and seen["ktp"] == {1, 2, 4, 8}
    m, k1, n = R.WGRAD_WAVE_SHAPE
    for cus in (64, 256, 304):
        p = R.wgrad_plan(m, k1, n, cus)
        assert p["wave_reduce"] and p["slots"] >= 128 and p["n_phase"] == 8, p
    assert R.wgrad_plan(m, k1, n, _library_cus())["slots"] == _library_slots(m, k1, n)
    src = open(os.path.join(os.path.dirname(__file__), "..", "text2pos-cvpr2022_amd", "csrc", "train_gemm.hip")).read()
    for piece in ("p.ktp = kt_n <= 1 ? 1 : (kt_n <= 2 ? 2 : (kt_n <= 4 ? 4 : 8));", "p.tpw = (nt_n + G - 1) / G;",
                  "p.ntp = nt_n <= 1 ? 1 : (nt_n <= 2 ? 2 : 4);", "p.n_phase = G / p.ntp;", "p.rows_chunk = (16384 / ldl) / 32 * 32;",
                  "const int64_t max_by_rows = (M + 2 * p.rows_chunk - 1) / (2 * p.rows_chunk);",
                  "if (total <= 16384 && n_slots >= 128)"):
        assert piece in src, piece


def test_two_plane_terms_are_exact_in_any_order():
    """fp32 sequential sums of the three kinds of product the f16x3 kernel forms on the two-plane inputs - hi.hi, hi.lo, lo.hi, 96
    terms per output - forwards, backwards and in three shuffled orders equal the stated result; with lo.lo they do not."""
    rng = np.random.default_rng(11)
    a, w, want, _ = R.two_plane_inputs(65, 40)
    (ah, al), (wh, wl) = R.split_f16(a.astype(np.float64)), R.split_f16(w.astype(np.float64))
    terms = np.concatenate([x[:, :, None] * y[None, :, :] for x, y in ((ah, wh), (ah, wl), (al, wh))], 1)       # [65][96][40]
    assert np.array_equal(terms.astype(F32).astype(np.float64), terms)
    n_terms = terms.shape[1]
    for order in [np.arange(n_terms), np.arange(n_terms)[::-1]] + [rng.permutation(n_terms) for _ in range(3)]:
        acc = np.zeros((65, 40), F32)
        for t in order:
            acc = (acc + terms[:, t, :].astype(F32)).astype(F32)
        assert np.array_equal(acc.astype(np.float64), want)
    assert not np.array_equal((want + al @ wl).astype(F32).astype(np.float64), want)


@pytest.mark.parametrize("widths", list(R.WGRAD_WIDTHS) + [R.WGRAD_WAVE_SHAPE[1:]])
def test_wgrad_emulation_within_bound_and_wrong_kernels_rejected(widths):
    k1, n = widths
    rows = [R.WGRAD_WAVE_SHAPE[0]] if widths == R.WGRAD_WAVE_SHAPE[1:] else R.WGRAD_ROWS
    lda, ldb, ldc = (k1 + 3) // 4 * 4 + 4, (n + 3) // 4 * 4 + 8, n + 3
    for m in rows:
        p = R.wgrad_plan(m, k1, n)
        last_rows = m - (p["splits"] - 1) * p["rows_per_split"]           # the last slot holds rows once its split has more than
        harmless = p["slots"] == 1 or last_rows <= 2 * (p["n_phase"] - 1)  # 2 (n_phase - 1): else leaving it out changes nothing
        caught = False
        for exact in (True, False):
            if exact and m == 3001 and k1 * n > 30000:
                continue                                                 # (seconds each; the exact inputs run at the smaller M there)
            dy, x = (R.tn_exact_inputs if exact else R.tn_inputs)(m, k1, n)
            dy_buf, x_buf, c_buf = R.pitched(dy, lda, 1), R.pitched(x, ldb, 1), R.nan_buffer(k1 + 1, ldc)
            ref, cref = R.tn_ref64(dy, x), R.colsum_ref64(dy)
            bound, cbound = R.tn_bound(dy, x, ref), R.colsum_bound(dy, cref)
            after, cs = R.wgrad_emul(dy_buf, lda, x_buf, ldb, c_buf, ldc, m, k1, n)
            ok, why = R.check_window(after, c_buf, k1, n, 0, ref, bound, 1.0, exact=exact)
            assert ok, (widths, m, exact, why)
            assert np.array_equal(cs.astype(np.float64), cref) if exact else R.within(cs, cref, cbound, 1.0), (widths, m, exact)
            bad, cs_bad = R.wgrad_emul(dy_buf, lda, x_buf, ldb, c_buf, ldc, m, k1, n, wrong="split_missing colsum_lda")
            caught |= not R.check_window(bad, c_buf, k1, n, 0, ref, bound, R.FACTOR_GPU, exact=exact)[0]
            assert not R.within(cs_bad, cref, cbound, R.FACTOR_GPU), (widths, m)      # the padding is NaN and 1e30
        # (at M = 20,000 a missing slot of ~90 rows is INSIDE twice the worst-case bound of N(0,1) data: the exact inputs see it)
        assert caught == (not harmless), (widths, m)
    assert R.wgrad_emul(dy_buf[:1], lda, x_buf[:1], ldb, c_buf, ldc, 1, k1, n, want_colsum=False)[1] is None
    print(f"wgrad {widths} M={m}: plan {p}, emulation worst ratio {R.worst_ratio(after[:k1, :n], ref, bound):.3f}")


def test_tile_choice_sides_differ_on_every_chip_below_272_cus():
    m, _, n = R.TILE_SHAPE
    for cus in (64, 104, 228, 256, 271):
        assert R.gemm_tile(m, n, cus) == 128 and R.gemm_tile(R.TILE_SMALL_ROWS, n, cus) == 64
    assert R.gemm_tile(m, n, 256) == 128 and R.gemm_tile(R.TILE_SMALL_ROWS, n, 256) == 64
    assert R.gemm_tile(m, n, 272) == 64                                  # 17 x 8 x 2 = 272: from there on both sides are the 64 tile
    assert all(R.gemm_tile(mm, nn, 256) == 64 for mm, _, nn in R.GEMM_SHAPES)


# ---- the new C-ABI entry points refuse bad arguments (nothing is launched: no GPU needed) -------------------------------------------------

def test_new_gemm_exports_refuse_bad_arguments():
    import text2pos_amd  # noqa: F401
    from text2pos_amd import _lib
    assert _lib.ABI_VERSION == _lib.lib().t2p_abi_version()
    assert all(name in _lib.SYMBOLS for name in ("t2p_gemm_residual", "t2p_gemm_x3", "t2p_gemm_skinny"))
    lib = _lib.lib()
    buf = (C.c_float * 80)()                 # host memory: every call below must return before it touches an operand
    p = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)
    null = C.c_void_p(0)

    def residual(a=p, lda=4, w=p, c=p, ldc=8, c0=0, m=1, k=4, n=8, resid=null, ldr=0):
        return lib.t2p_gemm_residual(a, lda, w, null, c, ldc, c0, m, k, n, 0, resid, ldr, null)

    def x3(a=p, lda=4, wx=p, scale=1.0, c=p, ldc=8, c0=0, m=1, k=4, n=8, resid=null, ldr=0):
        return lib.t2p_gemm_x3(a, lda, wx, scale, null, c, ldc, c0, m, k, n, 0, resid, ldr, null, null)

    def skinny(a=p, lda=4, w=p, c=p, ldc=8, m=1, k=4, n=8):
        return lib.t2p_gemm_skinny(a, lda, w, c, ldc, m, k, n, null)

    for f in (residual, x3, skinny):
        for bad in (dict(a=null), dict(c=null), dict(m=-1), dict(k=0), dict(n=0), dict(lda=3), dict(ldc=7)):
            assert f(**bad) == -1, (f.__name__, bad)
            assert lib.t2p_last_error()
        assert f(**({"wx": null} if f is x3 else {"w": null})) == -1
        assert f(m=0) == 0                                               # an empty product is no error and launches nothing
    for f in (residual, x3):
        assert f(c0=1) == -1 and f(c0=-1, ldc=16) == -1                  # window past the pitch / before the row
        assert f(resid=p, ldr=7) == -1                                   # residual pitch below the width
    assert x3(scale=0.0) == -1 and x3(scale=3.0) == -1 and x3(scale=-1.0) == -1
    assert skinny(k=6, lda=8) == -1                                      # K no multiple of 4
    assert residual(k=6, lda=8) == -1 and residual(n=4, ldc=4) == -1     # the launcher's own granules (K % 4, N % 8)
