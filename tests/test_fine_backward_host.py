"""CPU tests of the fine stage's backward (csrc/match_train.hip's t2p_*_backward, train_match.py, losses.py, training.py): the
ABI, the refusals that need no GPU, the opt-in switch, and the references the GPU tests rely on (tests/fine_backward_ref.py): each
fp32 emulation stays within 1 x its bound of the float64 statement, `within` rejects deliberately wrong formulae, and the head's
unrolled backward loop equals torch autograd through oracle.fine.log_optimal_transport."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import text2pos_amd as t2p  # noqa: E402
from text2pos_amd import _lib, training as T  # noqa: E402

import fine_backward_ref as FB  # noqa: E402
import fine_train_ref as R  # noqa: E402
from train_ops_ref import F32, within, worst_ratio  # noqa: E402

NEW = ("t2p_match_attention_backward", "t2p_match_head_backward_workspace_bytes", "t2p_match_head_backward",
       "t2p_matching_loss_backward", "t2p_mse_loss_backward", "t2p_colsum")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_backward_entry_points():
    assert _lib.ABI_VERSION == _lib.lib().t2p_abi_version()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name


def test_backward_entry_points_refuse_bad_sizes_without_a_gpu():
    """The forward's codes and wording, before anything touches the device (dummy non-NULL pointers)."""
    lib = _lib.lib()
    p = C.c_void_p(64)
    assert lib.t2p_match_attention_backward(p, p, 2, 16, 6, 96, 0, p, None) == -3                 # T2P_E_UNSUPPORTED
    assert b"embed_dim=96 not built" in lib.t2p_last_error()
    assert lib.t2p_match_attention_backward(p, p, 2, 64, 6, 128, 0, p, None) == -1                # T2P_E_ARG
    assert b"1 <= n_obj, n_hints <= 63 (got 64, 6)" in lib.t2p_last_error()
    assert lib.t2p_match_attention_backward(p, p, 2, 16, 64, 128, 1, p, None) == -1
    assert lib.t2p_match_attention_backward(p, p, 2, 16, 6, 128, 2, p, None) == -1
    assert b"cross must be 0 (self) or 1 (got 2)" in lib.t2p_last_error()
    assert lib.t2p_match_attention_backward(p, None, 2, 16, 6, 128, 0, p, None) == -1
    assert b"NULL argument" in lib.t2p_last_error()
    big = 1 << 30
    assert lib.t2p_match_head_backward(p, p, 2, 16, 6, 96, 1.0, 50, p, p, p, big, None) == -3
    assert b"embed_dim=96 not built" in lib.t2p_last_error()
    assert lib.t2p_match_head_backward(p, p, 2, 64, 6, 128, 1.0, 50, p, p, p, big, None) == -1
    assert b"1 <= n_obj, n_hints <= 63 (got 64, 6)" in lib.t2p_last_error()
    assert lib.t2p_match_head_backward(p, p, 2, 16, 0, 128, 1.0, 50, p, p, p, big, None) == -1
    assert lib.t2p_match_head_backward(p, p, 2, 16, 6, 128, 1.0, -1, p, p, p, big, None) == -1
    assert b"sinkhorn_iters < 0" in lib.t2p_last_error()
    assert lib.t2p_match_head_backward(p, None, 2, 16, 6, 128, 1.0, 50, p, p, p, big, None) == -1
    assert lib.t2p_matching_loss_backward(p, 0, 16, 6, p, p, 5, p, p, None) == -1
    assert lib.t2p_matching_loss_backward(p, 2, 16, 6, p, p, 0, p, p, None) == -1                 # n = 0
    assert b"n_entries" in lib.t2p_last_error()
    assert lib.t2p_matching_loss_backward(p, 2, 16, 6, p, p, 5, None, p, None) == -1
    assert lib.t2p_mse_loss_backward(p, p, 0, p, p, None) == -1
    assert b"no elements" in lib.t2p_last_error()
    assert lib.t2p_mse_loss_backward(None, p, 4, p, p, None) == -1
    assert lib.t2p_colsum(p, 0, 8, p, None) == -1
    assert b"rows, cols >= 1" in lib.t2p_last_error()
    assert lib.t2p_colsum(p, 8, 0, p, None) == -1
    assert lib.t2p_colsum(None, 8, 8, p, None) == -1


def test_head_backward_refuses_a_workspace_that_is_too_small():
    lib = _lib.lib()
    p = C.c_void_p(64)
    need = lib.t2p_match_head_backward_workspace_bytes(2, 16, 6, 50)
    assert need == 2 * 50 * (16 + 6 + 2) * 8                                                      # every iterate u_t, v_t in float64
    assert lib.t2p_match_head_backward_workspace_bytes(2, 16, 6, 0) == 0
    assert lib.t2p_match_head_backward_workspace_bytes(2, 64, 6, 50) == 0                         # sizes the call refuses
    assert lib.t2p_match_head_backward(p, p, 2, 16, 6, 128, 1.0, 50, p, p, p, need - 1, None) == -2   # T2P_E_WORKSPACE
    assert b"workspace" in lib.t2p_last_error()
    assert lib.t2p_match_head_backward(p, p, 2, 16, 6, 128, 1.0, 50, p, p, None, need, None) == -2


# ---- attention backward: the helpers ----------------------------------------------------------------------------------------------
HOST_ATTN = [(1, 1, 1, 64), (2, 4, 2, 128), (3, 5, 7, 64), (2, 63, 1, 64), (1, 20, 31, 256)]


@pytest.mark.parametrize("shape", HOST_ATTN)
@pytest.mark.parametrize("cross", [0, 1])
def test_attention_backward_emulation_within_one_bound(shape, cross):
    qkv, dmsg = FB.attn_inputs(*shape)
    ref, bound = FB.attn_bwd_ref64(qkv, dmsg, *shape, cross), FB.attn_bwd_bounds(qkv, dmsg, *shape, cross)
    assert np.isfinite(ref).all() and np.isfinite(bound).all()            # every element of d_qkv is covered by a workgroup
    emul = FB.attn_bwd_emul(qkv, dmsg, *shape, cross)
    print(f"attention backward {shape} cross={cross}: emulation at {worst_ratio(emul, ref, bound):.3f} x bound")
    assert within(emul, ref, bound, 1.0)


def test_attention_backward_bounds_reject_wrong_formulae():
    shape = (2, 5, 7, 64)
    qkv, dmsg = FB.attn_inputs(*shape)
    for cross in (0, 1):
        ref, bound = FB.attn_bwd_ref64(qkv, dmsg, *shape, cross), FB.attn_bwd_bounds(qkv, dmsg, *shape, cross)
        assert within(FB.attn_bwd_emul(qkv, dmsg, *shape, cross), ref, bound, 1.0)
        for wrong in ("no_rowsum", "no_scale"):
            assert not within(FB.attn_bwd_emul(qkv, dmsg, *shape, cross, wrong=wrong), ref, bound, 2.0), (cross, wrong)
    # dk on the target rows: the same rows for cross = 0, the other set's for cross = 1
    ref, bound = FB.attn_bwd_ref64(qkv, dmsg, *shape, 1), FB.attn_bwd_bounds(qkv, dmsg, *shape, 1)
    assert not within(FB.attn_bwd_emul(qkv, dmsg, *shape, 1, wrong="dk_to_target"), ref, bound, 2.0)
    same = (2, 6, 6, 64)                                                  # equal set sizes: every element written, to the wrong rows
    qkv, dmsg = FB.attn_inputs(*same)
    ref, bound = FB.attn_bwd_ref64(qkv, dmsg, *same, 1), FB.attn_bwd_bounds(qkv, dmsg, *same, 1)
    wrong = FB.attn_bwd_emul(qkv, dmsg, *same, 1, wrong="dk_to_target")
    assert np.isfinite(wrong).all() and not within(wrong, ref, bound, 2.0)


def test_attention_backward_reference_is_the_gradient_of_the_oracle_attention():
    """attn_bwd_ref64 against torch autograd through the attention lines of oracle.fine.Propagation.forward, in float64."""
    B, M, N, D = 2, 5, 7, 64
    qkv, dmsg = FB.attn_inputs(B, M, N, D)
    for cross in (0, 1):
        x = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
        msg = torch.zeros(B * (M + N), D, dtype=torch.float64)
        rows = []
        for b in range(B):
            for ts in (0, 1):
                ss = 1 - ts if cross else ts
                nt, ns = (M, N)[ts], (M, N)[ss]
                t0, s0 = FB.set_row(ts, b, B, M, N), FB.set_row(ss, b, B, M, N)
                dh = D // 4
                q = x[t0:t0 + nt, :D].view(1, nt, dh, 4)
                k = x[s0:s0 + ns, D:2 * D].view(1, ns, dh, 4)
                v = x[s0:s0 + ns, 2 * D:].view(1, ns, dh, 4)
                prob = torch.softmax(torch.einsum("bndh,bmdh->bhnm", q, k) / dh ** 0.5, dim=-1)
                rows.append((t0, torch.einsum("bhnm,bmdh->bndh", prob, v).reshape(nt, D)))
        for t0, r in rows:
            msg = msg + torch.nn.functional.pad(r, (0, 0, t0, B * (M + N) - t0 - r.shape[0]))
        (msg * torch.from_numpy(dmsg.astype(np.float64))).sum().backward()
        ref = FB.attn_bwd_ref64(qkv, dmsg, B, M, N, D, cross)
        assert np.abs(ref - x.grad.numpy()).max() < 1e-12 * np.abs(ref).max()


# ---- loss backwards: the helpers --------------------------------------------------------------------------------------------------
def _loss_case(shape, seed, duplicate):
    rng = np.random.default_rng(seed)
    b, m1, n1 = shape
    P = np.exp(rng.uniform(-40, 2, shape)).astype(F32)
    lists = [np.stack([rng.integers(0, m1, k), rng.integers(0, n1, k)], 1) for k in rng.integers(1, 2 * m1, b)]
    if duplicate:
        lists[0] = np.concatenate([lists[0], lists[0][:1], lists[0][:1]])
    return P, lists


@pytest.mark.parametrize("shape,dup", [((3, 5, 4), True), ((1, 2, 2), False), ((2, 64, 64), False)])
def test_matching_loss_backward_emulation_and_wrong_formulae(shape, dup):
    P, lists = _loss_case(shape, 7, dup)
    g = F32(0.7)
    ref = FB.matching_loss_bwd_ref64(P, lists, g)
    bound = FB.matching_loss_bwd_bounds(ref)
    emul = FB.matching_loss_bwd_emul(P, lists, g)
    assert within(emul, ref, bound, 1.0)
    listed = sum(len(set(map(tuple, a.tolist()))) for a in lists)
    assert np.count_nonzero(ref) == listed and (ref <= 0).all()
    if shape[0] > 1:
        assert not within(FB.matching_loss_bwd_emul(P, lists, g, wrong="no_batch"), ref, bound, 2.0)
    if dup:
        assert not within(FB.matching_loss_bwd_emul(P, lists, g, wrong="no_count"), ref, bound, 2.0)
    # a listed coupling that is 0: what the formula gives
    P0 = P.copy()
    i, j = lists[0][0]
    P0[0, i, j] = 0.0
    ref0 = FB.matching_loss_bwd_ref64(P0, lists, g)
    assert ref0[0, i, j] == -np.inf and within(FB.matching_loss_bwd_emul(P0, lists, g), ref0, FB.matching_loss_bwd_bounds(ref0), 1.0)
    # and it is the gradient of the reference's loss (training/losses.py:20-30) in float64
    x = torch.from_numpy(P.astype(np.float64)).requires_grad_(True)
    loss = torch.stack([(-torch.log(x[b, torch.as_tensor(a[:, 0]), torch.as_tensor(a[:, 1])])).mean() for b, a in enumerate(lists)]).mean()
    (float(g) * loss).backward()
    assert np.allclose(x.grad.numpy(), ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", [(4, 6, 2), (1,), (3, 1000, 7)])
def test_mse_backward_emulation_and_wrong_formula(shape):
    rng = np.random.default_rng(11)
    a, b = rng.standard_normal(shape).astype(F32), rng.standard_normal(shape).astype(F32)
    g = F32(5.0)
    ref = FB.mse_bwd_ref64(a, b, g)
    assert within(FB.mse_bwd_emul(a, b, g), ref, FB.mse_bwd_bounds(ref), 1.0)
    assert not within(FB.mse_bwd_emul(a, b, g, wrong="no_two"), ref, FB.mse_bwd_bounds(ref), 2.0)
    x = torch.from_numpy(a.astype(np.float64)).requires_grad_(True)
    (float(g) * ((x - torch.from_numpy(b.astype(np.float64))) ** 2).mean()).backward()
    assert np.allclose(x.grad.numpy(), ref, rtol=1e-12, atol=1e-300)


# ---- head backward: the loop is the right formula ------------------------------------------------------------------------------------
def _head_case(B, M, N, D, seed=9):
    rng = np.random.default_rng(seed)
    md = rng.standard_normal((B * (M + N), D)).astype(F32)
    dP = rng.standard_normal((B, M + 1, N + 1)).astype(F32)
    return md, dP


@pytest.mark.parametrize("shape", [(1, 1, 1, 64), (2, 4, 2, 128), (3, 5, 7, 64), (2, 63, 1, 64)])
@pytest.mark.parametrize("iters", [0, 1, 50])
def test_head_backward_loop_equals_autograd_through_the_oracle(shape, iters):
    from oracle import fine as OF
    B, M, N, D = shape
    md, dP = _head_case(*shape)
    alpha = 1.0
    ref_md, ref_bin = FB.head_bwd(md, dP, B, M, N, D, alpha, iters, np.longdouble)
    em_md, em_bin = FB.head_bwd(md, dP, B, M, N, D, alpha, iters, np.float64)
    x = torch.from_numpy(md.astype(np.float64)).requires_grad_(True)
    a = torch.tensor(alpha, dtype=torch.float64, requires_grad=True)
    m0, m1 = x[:B * M].view(B, M, D), x[B * M:].view(B, N, D)
    z = OF.log_optimal_transport(torch.einsum("bnd,bmd->bnm", m0, m1) / D ** 0.5, a, iters)
    (torch.exp(z) * torch.from_numpy(dP.astype(np.float64))).sum().backward()
    scale = float(np.abs(ref_md).max())
    e_md = float(np.abs(ref_md.astype(np.float64) - x.grad.numpy()).max()) / scale
    e_bin = abs(float(ref_bin.sum()) - float(a.grad)) / max(abs(float(a.grad)), scale)
    d64 = float(np.abs(em_md - ref_md).max())
    print(f"head backward {shape} iters={iters}: loop vs autograd {e_md:.1e} (d_mdesc), {e_bin:.1e} (bin_score); delta64 {d64:.2e} "
          f"at scale {scale:.2e}")
    assert e_md < 1e-10 and e_bin < 1e-10
    assert d64 < 1e-10 * scale                                            # the float64 emulation is a float64 evaluation of the same loop


def test_head_forward_helper_reproduces_the_oracle_couplings():
    from oracle import fine as OF
    B, M, N, D = 2, 5, 7, 64
    md, _ = _head_case(B, M, N, D)
    p = FB.head_couplings(md, B, M, N, D, 1.0, 50)
    x = torch.from_numpy(md.astype(np.float64))
    z = OF.log_optimal_transport(torch.einsum("bnd,bmd->bnm", x[:B * M].view(B, M, D), x[B * M:].view(B, N, D)) / D ** 0.5,
                                 torch.tensor(1.0, dtype=torch.float64), 50)
    assert np.abs(p - z.exp().numpy()).max() < 1e-12


def test_entry_lists_have_the_layout_of_all_matches():
    for case in FB.MATCHER_CASES:
        M, N = case["M"], case["N"]
        for a in FB.entry_lists(case["B"], M, N, case["seed"]):
            k = int(((a[:, 0] < M) & (a[:, 1] < N)).sum())
            assert 1 <= k <= min(M, N) and len(a) == M + N - k
            assert sorted(a[a[:, 0] < M][:, 0].tolist()) == list(range(M))      # every object once
            assert sorted(a[a[:, 1] < N][:, 1].tolist()) == list(range(N))      # every hint once


# ---- the switch -------------------------------------------------------------------------------------------------------------------
def test_fine_backward_switch_is_off_by_default_and_restored():
    assert T.fine_backward_enabled() is False
    with T.fine_backward():
        assert T.fine_backward_enabled() is True
        with T.fine_backward(False):
            assert T.fine_backward_enabled() is False
        assert T.fine_backward_enabled() is True
    assert T.fine_backward_enabled() is False
    with pytest.raises(KeyError):
        with T.fine_backward():
            raise KeyError("body")
    assert T.fine_backward_enabled() is False
    assert T.enable_fine_backward(True) is False and T.fine_backward_enabled() is True
    assert T.enable_fine_backward(False) is True and T.fine_backward_enabled() is False


def test_the_model_refusals_follow_the_switch_without_a_gpu():
    """_check_forward_only is the first line of forward_packed: with the switch off both modes raise today's messages on the CPU;
    with it on the train() branch passes and eval() stays refused."""
    prod = R.make_product(64, 1)
    prod.train()
    with pytest.raises(NotImplementedError, match="backward of the matcher is not built"):
        prod._check_forward_only()
    with pytest.raises(NotImplementedError, match="backward of the matcher is not built"):
        prod.forward_packed(None, None, None, None, None, None)
    prod.eval()
    with pytest.raises(NotImplementedError, match="forward-only"):
        prod._check_forward_only()
    with T.fine_backward():
        with pytest.raises(NotImplementedError, match="forward-only"):
            prod._check_forward_only()
        prod.train()
        prod._check_forward_only()
        with torch.no_grad():
            prod._check_forward_only()
    with pytest.raises(NotImplementedError, match="backward of the matcher is not built"):
        prod._check_forward_only()


def test_train_fine_epoch_is_exported_with_the_reference_statistics():
    assert T.FINE_TRAIN_KEYS == ("loss", "loss_offsets", "recall", "precision", "pose_mid", "pose_mean", "pose_offsets")
    assert callable(T.train_fine_epoch) and isinstance(t2p.MatchingLoss(), torch.nn.Module)
