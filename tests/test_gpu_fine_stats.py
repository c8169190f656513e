"""t2p_fine_step_stats alone (-m gpu): crafted int64 / fp32 inputs, no model.  The yardstick is losses.calc_recall_precision and
losses.calc_pose_error (the reference's training/losses.py:33-62, :81-123 in NumPy) on the equivalent host lists, with stand-in objects
that only have get_center().
Bars: recall and precision are bit-equal (both sides compute count / n in float64).  Pose errors and the five means stay within
64 * 2^-53 * (1 + max|centre| + max|offset| + |pose|): an estimate is the sum of at most 63 terms, a division, two subtractions, two
squares, a sum and a root, then for a mean one more sum and division - fewer than 64 float64 roundings on quantities of that size
in any summation order, NumPy's pairwise one included.  The bar is not a measurement."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 5, 7), (8, 16, 6), (65, 16, 6), (2, 63, 63)]
SHIFT = {(1, 1, 1): 5, (3, 5, 7): 2, (2, 63, 63): 4}     # which of the forced kinds the small batches get
EPS = 2.0 ** -53


def _dev():
    return torch.device("cuda:0")


class _Centre:
    def __init__(self, c):
        self.c = c

    def get_center(self):
        return self.c


def _case(b, m, n, seed=0):
    """Tables of b + 3 poses and a batch of b samples over a permutation of them.  Sample s is forced, by (s + SHIFT) % 6, into: 0 no
    ground-truth pair (every other row has at least one); 1 no predicted match; 2 every pair found through matches1 only; 3 every
    predicted pair wrong; 4 every slot matched (so padding slots are predicted as matched); 5 as drawn."""
    rng = np.random.default_rng([seed, b, m, n])
    rows = b + 3
    pose_idx = rng.permutation(rows)[:b].astype(np.int32)
    gt = np.full((rows, m), -1, dtype=np.int32)
    for r in range(rows):
        k = int(rng.integers(1, min(m, n) + 1))
        gt[r, rng.permutation(m)[:k]] = rng.permutation(n)[:k]
    pose_xy = rng.random((rows, 2))
    centre = rng.uniform(-0.3, 1.4, (rows, m, 3))
    m0 = np.full((b, m), -1, dtype=np.int64)
    m1 = rng.integers(-1, m, (b, n)).astype(np.int64)
    off = rng.uniform(-0.6, 0.6, (b, n, 2)).astype(np.float32)
    for s in range(b):
        g = gt[pose_idx[s]]
        draw = rng.random(m)
        wrong = rng.integers(0, n, m)
        m0[s] = np.where(draw < 0.3, -1, np.where(draw < 0.7, np.where(g >= 0, g, wrong), wrong))
        kind = (s + SHIFT.get((b, m, n), 0)) % 6
        if kind == 0:
            gt[pose_idx[s]] = -1
        elif kind == 1:
            m0[s] = -1
        elif kind == 2:
            m0[s] = np.where(g >= 0, -1, m0[s])
            m1[s] = -1
            for i in np.nonzero(g >= 0)[0]:
                m1[s, g[i]] = i
        elif kind == 3 and n > 1:
            m0[s] = np.where(g >= 0, (g + 1) % n, wrong)
            m1[s] = -1
        elif kind == 4:
            m0[s] = np.where(g >= 0, g, wrong)
    return dict(b=b, m=m, n=n, rows=rows, pose_idx=pose_idx, gt=gt, pose_xy=pose_xy, centre=centre, m0=m0, m1=m1, off=off)


def _reference(c):
    """Per-sample [b, 5] and the five means by the host functions, on lists."""
    from text2pos_amd import losses as L
    b, m = c["b"], c["m"]
    objects = [[_Centre(c["centre"][c["pose_idx"][s], i]) for i in range(m)] for s in range(b)]
    poses = [np.array([*c["pose_xy"][c["pose_idx"][s]], 0.0]) for s in range(b)]
    matches = [np.array([(i, j) for i, j in enumerate(c["gt"][c["pose_idx"][s]]) if j >= 0]).reshape(-1, 2) for s in range(b)]
    sample = np.zeros((b, 5))
    for s in range(b):
        sample[s, 0:2] = L.calc_recall_precision(matches[s: s + 1], c["m0"][s: s + 1], c["m1"][s: s + 1])
    sample[:, 2] = L.calc_pose_error(objects, c["m0"], poses, offsets=c["off"], use_mid_pred=True, return_samples=True)
    sample[:, 3] = L.calc_pose_error(objects, c["m0"], poses, offsets=None, return_samples=True)
    sample[:, 4] = L.calc_pose_error(objects, c["m0"], poses, offsets=c["off"], return_samples=True)
    recall, precision = L.calc_recall_precision(matches, c["m0"], c["m1"])
    means = np.array([recall, precision, L.calc_pose_error(objects, c["m0"], poses, offsets=c["off"], use_mid_pred=True),
                      L.calc_pose_error(objects, c["m0"], poses, offsets=None), L.calc_pose_error(objects, c["m0"], poses, offsets=c["off"])])
    return sample, means


def _bar(c):
    return 64 * EPS * (1.0 + np.abs(c["centre"][..., 0:2]).max() + float(np.abs(c["off"]).max()) + np.abs(c["pose_xy"]).max())


def _upload(c):
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return dict(m0=to(c["m0"]), m1=to(c["m1"]), off=to(c["off"]), pose_idx=to(c["pose_idx"]), gt=to(c["gt"]), pose_xy=to(c["pose_xy"]),
                centre=to(c["centre"][..., 0:2]))


def _run(t, loss=None, loss_offsets=None, check=True):
    from text2pos_amd import ops
    s, r = ops.fine_step_stats(t["m0"], t["m1"], t["off"], t["pose_idx"], t["gt"], t["pose_xy"], t["centre"], loss, loss_offsets, check=check)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for shape in SHAPES:
        c = _case(*shape)
        out[shape] = (c, _reference(c), _upload(c))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_stats_against_the_host_functions(cases, shape):
    c, (want, want_means), t = cases[shape]
    loss = torch.tensor([1.2345678], device=_dev())
    loss_offsets = torch.tensor(0.0123456789, device=_dev())          # (a 0-dim scalar, as the loop has it)
    sample, row = _run(t, loss, loss_offsets)
    assert sample.shape == (c["b"], 5) and row.shape == (7,) and sample.dtype == row.dtype == np.float64
    assert np.array_equal(sample[:, 0:2], want[:, 0:2])                                       # count / n: bit-equal
    bar = _bar(c)
    err = np.abs(sample[:, 2:] - want[:, 2:]).max()
    mean_err = np.abs(row[2:] - want_means).max()
    print(f"{shape}: pose error {err:.3e}, means {mean_err:.3e} (bar {bar:.3e})")
    assert err <= bar and mean_err <= bar
    assert row[0] == float(loss.cpu()[0]) and row[1] == float(loss_offsets.cpu())             # the exact float64 of the fp32 scalars
    # the means are the ascending sums of the kernel's own rows, exactly
    acc = np.zeros(5)
    for s in range(c["b"]):
        acc = acc + sample[s]
    assert np.array_equal(row[2:], acc / c["b"])
    again = _run(t, loss, loss_offsets)
    assert np.array_equal(again[0], sample) and np.array_equal(again[1], row)                  # call to call: the same bits
    none = _run(t)[1]
    assert np.isnan(none[0:2]).all() and np.array_equal(none[2:], row[2:])                     # no losses given: NaN, nothing else moves


def test_the_forced_cases_are_what_they_claim(cases):
    c, (want, _), t = cases[(8, 16, 6)]
    sample, _ = _run(t)
    g = c["gt"][c["pose_idx"]]
    assert (g[0] < 0).all() and sample[0, 0] == 0.0                                            # no ground-truth pair: recall 0
    assert (c["m0"][1] < 0).all() and sample[1, 1] == 0.0 and sample[1, 3] == sample[1, 2] == sample[1, 4]   # nothing predicted: (0.5, 0.5)
    assert (g[2] >= 0).any() and (c["m0"][2][g[2] >= 0] < 0).all() and sample[2, 0] == 1.0      # through matches1 only
    assert (g[3] >= 0).any() and sample[3, 0] == 0.0 and sample[3, 1] == 0.0                   # every predicted pair wrong
    assert (c["m0"][4] >= 0).all() and (g[4] < 0).any() and 0.0 < sample[4, 1] < 1.0 and sample[4, 0] == 1.0   # padding predicted as matched
    assert np.array_equal(sample[:, 0:2], want[:, 0:2])


def test_outputs_are_overwritten_and_nothing_behind_them(cases):
    from text2pos_amd import _lib
    c, _, t = cases[(3, 5, 7)]
    b = c["b"]
    sample = torch.full((b * 5 + 16,), float("nan"), dtype=torch.float64, device=_dev())
    row = torch.full((7 + 16,), float("nan"), dtype=torch.float64, device=_dev())
    sample[b * 5:] = -7.0
    row[7:] = -7.0
    p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())
    rc = _lib.lib().t2p_fine_step_stats(p(t["m0"]), p(t["m1"]), p(t["off"]), p(t["pose_idx"]), b, c["m"], c["n"], p(t["gt"]), p(t["pose_xy"]),
                                        p(t["centre"]), c["rows"], p(None), p(None), p(sample), p(row),
                                        C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream))
    _lib.check(rc, "t2p_fine_step_stats")
    torch.cuda.synchronize()
    want_s, want_r = _run(t)
    assert np.array_equal(sample[: b * 5].cpu().numpy().reshape(b, 5), want_s) and not torch.isnan(sample[: b * 5]).any()
    assert np.isnan(row[:2].cpu().numpy()).all() and np.array_equal(row[2:7].cpu().numpy(), want_r[2:])
    assert bool((sample[b * 5:] == -7.0).all()) and bool((row[7:] == -7.0).all())


@pytest.mark.parametrize("what", ["pose_idx_high", "pose_idx_negative", "matches0_high", "matches0_low", "matches1_high", "gt_hint_high"])
def test_a_bad_index_marks_the_sample_and_raises(cases, what):
    c, _, t = cases[(8, 16, 6)]
    good, _ = _run(t)
    t = {k: v.clone() for k, v in t.items()}
    victim = 5
    if what == "pose_idx_high":
        t["pose_idx"][victim] = c["rows"]
    elif what == "pose_idx_negative":
        t["pose_idx"][victim] = -1
    elif what == "matches0_high":
        t["m0"][victim, 3] = c["n"]
    elif what == "matches0_low":
        t["m0"][victim, 3] = -2
    elif what == "matches1_high":
        t["m1"][victim, 2] = c["m"]
    else:
        t["gt"][int(c["pose_idx"][victim]), 1] = c["n"]
    sample, row = _run(t, check=False)
    assert np.isnan(sample[victim]).all() and np.isnan(row[2:]).all()
    keep = [s for s in range(c["b"]) if s != victim]
    assert np.array_equal(sample[keep], good[keep])                                            # the other samples are untouched
    with pytest.raises(IndexError, match="fine_step_stats"):
        _run(t)


def test_wrapper_refusals():
    from text2pos_amd import ops
    c = _case(3, 5, 7)
    t = _upload(c)
    with pytest.raises(RuntimeError, match="one batch"):
        ops.fine_step_stats(t["m0"], t["m1"][:2].contiguous(), t["off"], t["pose_idx"], t["gt"], t["pose_xy"], t["centre"])
    with pytest.raises(RuntimeError, match="tables"):
        ops.fine_step_stats(t["m0"], t["m1"], t["off"], t["pose_idx"], t["gt"][:, :4].contiguous(), t["pose_xy"], t["centre"])
    with pytest.raises(RuntimeError, match="dtype"):
        ops.fine_step_stats(t["m0"].int(), t["m1"], t["off"], t["pose_idx"], t["gt"], t["pose_xy"], t["centre"])
    with pytest.raises(RuntimeError, match="one value"):
        ops.fine_step_stats(t["m0"], t["m1"], t["off"], t["pose_idx"], t["gt"], t["pose_xy"], t["centre"], loss=torch.zeros(2, device=_dev()))
