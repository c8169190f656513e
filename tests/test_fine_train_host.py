"""CPU tests of the fine stage's train-mode surface: the host-side validation figures (training/losses.py:33-62, :81-123 restated in
losses.py), synthetic.make_fine_batch's invariants (dataloading/kitti360pose/poses.py:114-137), the refusals of the two loss modules
that need no GPU, the ABI number, and the decision-margin rule the GPU tests rely on."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import text2pos_amd as t2p  # noqa: E402
from text2pos_amd import _lib, losses as Lo, synthetic as S, training as T  # noqa: E402
from text2pos_amd.data import Object3d, Pose  # noqa: E402

import fine_train_ref as R  # noqa: E402


def _obj(x, y):
    return Object3d(0, 0, np.array([[x, y, 0.0], [x, y, 0.2]]), np.zeros((2, 3)), "box")


def _pose(x, y):
    return Pose(np.array([x, y, 0.0]), np.zeros(3), "c", "s")


# ---- calc_recall_precision --------------------------------------------------------------------------------------------------
def test_recall_precision_without_any_match():
    gt = [np.array([[0, 1], [2, 0]])]
    assert Lo.calc_recall_precision(gt, np.full((1, 3), -1), np.full((1, 2), -1)) == (0.0, 0.0)


def test_recall_precision_all_matched():
    gt = [np.array([[0, 1], [2, 0]])]
    m0, m1 = np.array([[1, -1, 0]]), np.array([[2, 0]])
    assert Lo.calc_recall_precision(gt, m0, m1) == (1.0, 1.0)


def test_recall_precision_with_a_wrong_match():
    # sample 0: ground truth (0, 1), (2, 0); matches0 finds (0, 1), assigns object 1 to hint 0 (wrong) and misses (2, 0);
    #           matches1 does not report (2, 0) either -> recall 1/2, precision 1/2
    # sample 1: no ground-truth pair, one assigned object -> recall 0 (no pairs), precision 0 / 1
    gt = [np.array([[0, 1], [2, 0]]), np.zeros((0, 2), dtype=np.int64)]
    m0 = np.array([[1, 0, -1], [-1, 1, -1]])
    m1 = np.array([[1, 0], [-1, 1]])
    recall, precision = Lo.calc_recall_precision(gt, m0, m1)
    assert recall == pytest.approx((0.5 + 0.0) / 2) and precision == pytest.approx((0.5 + 0.0) / 2)


def test_recall_counts_a_pair_that_only_matches1_reports():
    gt = [np.array([[2, 0]])]
    recall, precision = Lo.calc_recall_precision(gt, np.array([[-1, -1, -1]]), np.array([[2, -1]]))
    assert recall == 1.0 and precision == 0.0          # (precision looks at matches0 alone)


def test_recall_precision_refuses_lists_of_different_length():
    with pytest.raises(RuntimeError, match="differ in length"):
        Lo.calc_recall_precision([np.zeros((0, 2))], np.zeros((2, 3)), np.zeros((2, 2)))


# ---- calc_pose_error --------------------------------------------------------------------------------------------------------
def _pose_case():
    objects = [[_obj(0.2, 0.2), _obj(0.8, 0.4), _obj(0.5, 0.9)], [_obj(0.1, 0.1), _obj(0.3, 0.3), _obj(0.6, 0.6)]]
    matches0 = np.array([[1, -1, 0], [-1, -1, -1]])
    offsets = np.array([[[0.1, 0.0], [0.0, -0.2]], [[0.3, 0.3], [0.3, 0.3]]])
    poses = [_pose(0.4, 0.5), _pose(0.9, 0.5)]
    return objects, matches0, offsets, poses


def test_pose_error_with_offsets():
    objects, matches0, offsets, poses = _pose_case()
    # sample 0: object 0 + offset of hint 1 = (0.2, 0.0), object 2 + offset of hint 0 = (0.6, 0.9) -> mean (0.4, 0.45): error 0.05
    # sample 1: nothing matched -> the cell's middle (0.5, 0.5): error 0.4
    assert Lo.calc_pose_error(objects, matches0, poses, offsets=offsets) == pytest.approx((0.05 + 0.4) / 2)
    assert Lo.calc_pose_error(objects, matches0, poses, offsets=offsets, return_samples=True) == pytest.approx([0.05, 0.4])


def test_pose_error_without_offsets_is_the_mean_of_the_matched_centres():
    objects, matches0, _, poses = _pose_case()
    # sample 0: mean of (0.2, 0.2) and (0.5, 0.9) = (0.35, 0.55): error hypot(0.05, 0.05)
    assert Lo.calc_pose_error(objects, matches0, poses, offsets=None) == pytest.approx((np.hypot(0.05, 0.05) + 0.4) / 2)


def test_pose_error_use_mid_pred_ignores_matches_and_offsets():
    objects, matches0, offsets, poses = _pose_case()
    want = (np.hypot(0.1, 0.0) + 0.4) / 2
    assert Lo.calc_pose_error(objects, matches0, poses, offsets=offsets, use_mid_pred=True) == pytest.approx(want)
    assert Lo.calc_pose_error(objects, np.full_like(matches0, -1), poses, use_mid_pred=True) == pytest.approx(want)


def test_pose_error_all_objects_matched():
    objects = [[_obj(0.0, 0.0), _obj(1.0, 1.0)]]
    got = Lo.calc_pose_error(objects, np.array([[0, 1]]), [_pose(0.5, 0.5)], offsets=np.zeros((1, 2, 2)))
    assert got == pytest.approx(0.0)


def test_pose_error_refuses_lists_of_different_length():
    objects, matches0, offsets, poses = _pose_case()
    with pytest.raises(RuntimeError, match="differ in length"):
        Lo.calc_pose_error(objects, matches0, poses[:1])
    with pytest.raises(RuntimeError, match="offsets differ"):
        Lo.calc_pose_error(objects, matches0, poses, offsets=offsets[:1])


# ---- make_fine_batch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,n_obj,n_hints,n_pts", [(3, 16, 6, 64), (2, 5, 7, 8), (4, 4, 2, 16)])
def test_make_fine_batch_invariants(batch, n_obj, n_hints, n_pts):
    b = S.make_fine_batch(5, batch, n_obj, n_hints, n_pts)
    for key in ("objects", "object_points", "hint_descriptions", "matches", "all_matches", "offsets", "poses"):
        assert len(b[key]) == batch, key
    for i in range(batch):
        matches, all_matches = b["matches"][i], b["all_matches"][i]
        k = len(matches)
        assert 1 <= k <= min(n_obj, n_hints)
        assert len(b["objects"][i]) == n_obj and len(b["hint_descriptions"][i]) == n_hints
        assert b["object_points"][i].pos.shape == (n_obj * n_pts, 3) and b["object_points"][i].x.shape == (n_obj * n_pts, 3)
        assert matches.shape == (k, 2) and all_matches.shape == (n_obj + n_hints - k, 2)
        assert all_matches.dtype.kind == "i"
        assert np.array_equal(all_matches[:k], matches)
        assert np.array_equal(matches[:, 0], np.arange(k))                      # the matched objects come first
        assert len(set(matches[:, 1].tolist())) == k and matches[:, 1].max() < n_hints
        assert np.sum(all_matches[:, 1] == n_hints) == n_obj - k                # unmatched objects: the hints' dustbin column
        assert np.sum(all_matches[:, 0] == n_obj) == n_hints - k                # unmatched hints: the objects' dustbin row
        assert sorted(all_matches[all_matches[:, 0] < n_obj][:, 0].tolist()) == list(range(n_obj))     # every object once
        assert sorted(all_matches[all_matches[:, 1] < n_hints][:, 1].tolist()) == list(range(n_hints))  # every hint once
        assert b["offsets"][i].shape == (n_hints, 2) and np.isfinite(b["offsets"][i]).all()
        pose = b["poses"][i].pose
        assert pose.shape == (3,) and (0 <= pose[:2]).all() and (pose[:2] <= 1).all()
        for o, h in matches:                                                    # offset = pose - centre of the matched object
            assert np.allclose(b["offsets"][i][h], pose[:2] - b["objects"][i][o].get_center()[:2])
    xyz, rgb, center, mean_rgb, cell_ptr = b["packed"]
    assert xyz.shape == (batch * n_obj, n_pts, 3) and np.array_equal(cell_ptr, np.arange(batch + 1) * n_obj)
    flat = [o for objs in b["objects"] for o in objs]
    assert np.array_equal(np.stack([o.get_center() for o in flat]).astype(np.float32), center)
    assert np.array_equal(np.stack([o.get_color_rgb() for o in flat]).astype(np.float32), mean_rgb)
    assert np.array_equal(torch.cat([p.pos for p in b["object_points"]]).numpy().reshape(xyz.shape), xyz)
    again = S.make_fine_batch(5, batch, n_obj, n_hints, n_pts)
    assert again["hint_descriptions"] == b["hint_descriptions"] and np.array_equal(again["packed"][0], xyz)


def test_make_fine_batch_feeds_the_host_figures():
    b = S.make_fine_batch(9, 3, 16, 6, 8)
    m0 = np.full((3, 16), -1)
    m1 = np.full((3, 6), -1)
    for i, matches in enumerate(b["matches"]):
        m0[i, matches[:, 0]] = matches[:, 1]
        m1[i, matches[:, 1]] = matches[:, 0]
    out = t2p.superglue_matcher.MatchOutputs(matches0=torch.from_numpy(m0), matches1=torch.from_numpy(m1),
                                             offsets=torch.from_numpy(np.stack(b["offsets"])))
    stats = T.fine_batch_stats(b, out)
    assert set(stats) == set(T.FINE_VAL_KEYS)
    assert stats["recall"] == 1.0 and stats["precision"] == 1.0
    assert stats["pose_offsets"] == pytest.approx(0.0, abs=1e-6)               # ground-truth matches + ground-truth offsets
    assert np.isfinite(stats["pose_mid"]) and np.isfinite(stats["pose_mean"])


# ---- loss modules: refusals that need no GPU -------------------------------------------------------------------------------------
def test_matching_loss_has_no_cpu_path_and_checks_shapes():
    crit = t2p.MatchingLoss()
    p = torch.full((2, 4, 3), 0.1)
    good = [np.array([[0, 1]]), np.array([[3, 2]])]
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(p, good)
    with pytest.raises(RuntimeError, match=r"\[B, n_obj \+ 1, n_hints \+ 1\]"):
        crit(p[0], good)


def test_mse_loss_has_no_cpu_path_and_checks_shapes():
    crit = t2p.MSELoss()
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(torch.zeros(2, 6, 2), torch.zeros(2, 6, 2))
    with pytest.raises(RuntimeError, match="same shape"):
        crit(torch.zeros(2, 6, 2), torch.zeros(2, 6))
    with pytest.raises(RuntimeError, match="tensors"):
        crit(torch.zeros(2), [0.0, 0.0])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_train_mode_entry_points():
    assert _lib.ABI_VERSION == _lib.lib().t2p_abi_version()
    for name in ("t2p_match_attention", "t2p_match_head", "t2p_matching_loss", "t2p_mse_loss"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name


def test_new_entry_points_refuse_bad_sizes_without_a_gpu():
    """Sizes are checked before anything touches the device: the refusals can be had on any machine (dummy non-NULL pointers)."""
    import ctypes as C
    lib = _lib.lib()
    p = C.c_void_p(64)
    assert lib.t2p_match_attention(p, 2, 16, 6, 96, 0, p, None) == -3                  # T2P_E_UNSUPPORTED
    assert b"embed_dim=96 not built" in lib.t2p_last_error()
    assert lib.t2p_match_attention(p, 2, 64, 6, 128, 0, p, None) == -1                 # T2P_E_ARG
    assert b"1 <= n_obj, n_hints <= 63" in lib.t2p_last_error()
    assert lib.t2p_match_attention(p, 2, 16, 6, 128, 2, p, None) == -1
    assert lib.t2p_match_head(p, 2, 16, 0, 128, 1.0, 50, 0.2, p, p, p, p, p, None) == -1
    assert b"1 <= n_obj, n_hints <= 63" in lib.t2p_last_error()
    assert lib.t2p_match_head(p, 2, 16, 6, 512, 1.0, 50, 0.2, p, p, p, p, p, None) == -3
    assert lib.t2p_match_head(p, 2, 16, 6, 128, 1.0, -1, 0.2, p, p, p, p, p, None) == -1
    assert lib.t2p_matching_loss(p, 0, 16, 6, p, p, 5, p, p, None) == -1
    assert lib.t2p_matching_loss(p, 2, 16, 6, p, p, 0, p, p, None) == -1
    assert lib.t2p_mse_loss(p, p, 0, p, None) == -1
    assert lib.t2p_mse_loss(None, p, 4, p, None) == -1


# ---- the margin rule of the GPU tests ------------------------------------------------------------------------------------------------
def test_decision_margins_on_a_hand_worked_matrix():
    # inner block (2 objects x 2 hints), log values chosen directly; dustbin row / column are ignored by the rule
    lp = np.array([[[0.0, -3.0, -9.0], [-2.0, -0.5, -9.0], [-9.0, -9.0, -9.0]]])
    m0, m1 = R.decision_margins(np.exp(lp))
    log02 = np.log(0.2)
    # object 0: row gap 3, winner hint 0 whose column gap is 2, distance from log 0.2 = 1.609 -> 1.609
    # object 1: row gap 1.5, winner hint 1 whose column gap is 2.5, distance |-0.5 - log 0.2| = 1.109 -> 1.109
    assert m0[0] == pytest.approx([abs(0.0 - log02), abs(-0.5 - log02)])
    # hint 0: column gap 2, winner object 0 whose row gap is 3, distance 1.609; hint 1: column gap 2.5, row gap 1.5, 1.109
    assert m1[0] == pytest.approx([abs(0.0 - log02), abs(-0.5 - log02)])
    tie = np.array([[[-1.0, -1.0 - 4e-4, -9.0], [-5.0, -6.0, -9.0], [-9.0, -9.0, -9.0]]])
    m0, m1 = R.decision_margins(np.exp(tie))
    assert m0[0, 0] == pytest.approx(4e-4) and m0[0, 1] == pytest.approx(1.0)      # a near-tie in row 0; object 1: its own row gap
    assert m1[0, 1] == pytest.approx(4e-4)                                          # hint 1's winner is object 0, whose row is the tie
    empty = np.zeros((1, 3, 3))                                                     # P = 0 everywhere: clamped, every gap 0
    m0, _ = R.decision_margins(empty)
    assert (m0 == 0).all()
