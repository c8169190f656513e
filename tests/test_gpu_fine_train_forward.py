"""The fine matcher in train() mode on the MI355X (train_match.py, csrc/match_train.hip) against oracle/fine.py in .train(), evaluated
in float64 (tests/fine_train_ref.py holds the shapes, the references and the log-domain margin rule): forward outputs, BatchNorm
running statistics, the two loss values, the validation epoch of training/fine.py:119-170 and the refusals.

In train() mode the matcher saturates with the golden weights (couplings from 8 down to 1e-47 at two layers), so
  * matches are compared where the float64 oracle's decision has a margin of at least 1e-3 in log P, and the share of entries below
    that margin is asserted per shape (0 for a-d, at most 15 % for e and f);
  * loss entries are chosen where the float64 coupling is at least 1e-30: below fp32's range -log P is inf, in the reference as here.

Every test prints the distances it measures before it asserts (pytest -s); docs/notebook.md, "Fine matcher in train() mode", is where
they are recorded."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fine_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4        # unit rows and P: the project's bar
TOL_OFFSETS = 1e-5


def _dev():
    return torch.device("cuda:0")


def _to_dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) for a in arrays]


def _cpu(out):
    return {k: v.detach().cpu() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def hip_forward(name):
    """One train-mode forward_packed of a fresh product model on a shape: (outputs on the CPU, the model's state_dict afterwards)."""
    r = R.reference(name)
    s = r["shape"]
    prod = R.make_product(s["D"], s["layers"], _dev()).train()
    xyz, rgb, center, mean_rgb, cell_ptr, hints = r["inputs"]
    with torch.no_grad():
        got = prod.forward_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, hints)
    return _cpu(got), {k: v.detach().cpu().clone() for k, v in prod.state_dict().items()}


def _check_matches(got, want, margin0, margin1, cap, what):
    """matches0 / matches1 equal the float64 oracle's wherever its decision margin is at least R.MARGIN; the share of entries below
    the margin is itself bounded by `cap`."""
    for key, margin in (("matches0", margin0), ("matches1", margin1)):
        decided = margin >= R.MARGIN
        share = 1.0 - decided.mean()
        print(f"{what} {key}: {int((~decided).sum())} of {decided.size} entries below the margin, smallest margin {margin.min():.2e}")
        assert share <= cap, (what, key, share, cap)
        g, w = got[key].numpy(), want[key].numpy()
        assert g.shape == w.shape and g.dtype == np.int64
        assert np.array_equal(g[decided], w[decided]), (what, key, np.argwhere((g != w) & decided).tolist())


# ---- 1. the whole forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_train_mode_forward_matches_the_float64_oracle(name):
    r = R.reference(name)
    got, _ = hip_forward(name)
    want, s = r["out64"], r["shape"]
    assert got["P"].shape == (s["B"], s["M"] + 1, s["N"] + 1) and got["offsets"].shape == (s["B"], s["N"], 2)
    e_obj = (got["object_encodings"].double() - want["object_encodings"]).abs().max().item()
    e_hint = (got["hint_encodings"].double() - want["hint_encodings"]).abs().max().item()
    e_off = (got["offsets"].double() - want["offsets"]).abs().max().item()
    e_p = (got["P"].double() - want["P"]).abs().max().item()
    bar_p = max(TOL, 1.5 * r["e32"])
    print(f"shape {name}: object rows {e_obj:.2e}, hint rows {e_hint:.2e}, offsets {e_off:.2e}, P {e_p:.2e} "
          f"(fp32 oracle {r['e32']:.2e}, bar {bar_p:.2e})")
    assert e_obj < TOL and e_hint < TOL, (e_obj, e_hint)
    assert e_off < TOL_OFFSETS, e_off
    assert e_p < bar_p, (e_p, r["e32"])
    _check_matches(got, want, r["margin0"], r["margin1"], s["cap"], f"shape {name}")
    # the scores belong to the matches: exp of the winning log coupling where the match is mutual, else 0
    m0 = got["matches0"]
    inner = got["P"][:, :-1, :-1]
    assert torch.equal(got["matching_scores0"] > 0.2, m0 >= 0)
    picked = inner.gather(2, m0.clamp(min=0)[:, :, None])[:, :, 0]
    assert ((got["matching_scores0"] - picked).abs()[m0 >= 0] < 1e-6 * picked[m0 >= 0].clamp(min=1)).all()


# ---- 2. the matcher alone ---------------------------------------------------------------------------------------------------------
def _unit_descriptors(s, seed=4242):
    g = torch.Generator().manual_seed(seed)
    d0 = torch.nn.functional.normalize(torch.randn(s["B"], s["M"], s["D"], generator=g), dim=-1)
    d1 = torch.nn.functional.normalize(torch.randn(s["B"], s["N"], s["D"], generator=g), dim=-1)
    return d0, d1


@functools.lru_cache(maxsize=None)
def _matcher_reference(name):
    s = R.SHAPES[name]
    d0, d1 = _unit_descriptors(s)
    orc = R.oracle_from(R.make_product(s["D"], s["layers"]).state_dict(), s["D"], s["layers"])
    sg64, off64 = copy.deepcopy(orc.superglue).train().double(), copy.deepcopy(orc.mlp_offsets).double()
    sg32 = copy.deepcopy(orc.superglue).train()
    with torch.no_grad():
        w64, w32 = sg64(d0.double(), d1.double()), sg32(d0, d1)
        w64["offsets"] = off64(d1.double())
    e32 = (w32["P"].double() - w64["P"]).abs().max().item()
    m0, m1 = R.decision_margins(w64["P"].numpy())
    return d0, d1, w64, e32, m0, m1


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_matcher_alone_on_random_unit_descriptors(name):
    from text2pos_amd import train_match as TM
    s = R.SHAPES[name]
    d0, d1, want, e32, margin0, margin1 = _matcher_reference(name)
    prod = R.make_product(s["D"], s["layers"], _dev()).train()
    saved = copy.deepcopy(prod.state_dict())
    with torch.no_grad():
        got = _cpu(TM.match_train_forward(prod, d0.to(_dev()), d1.to(_dev())))
        prod.load_state_dict(saved)                         # the running estimates back where they were
        again = _cpu(TM.match_train_forward(prod, d0.to(_dev()), d1.to(_dev())))
    e_p = (got["P"].double() - want["P"]).abs().max().item()
    e_off = (got["offsets"].double() - want["offsets"]).abs().max().item()
    print(f"matcher alone, shape {name}: P {e_p:.2e} (fp32 oracle {e32:.2e}), offsets {e_off:.2e}")
    assert e_p < max(TOL, 1.5 * e32), (e_p, e32)
    assert e_off < TOL_OFFSETS
    _check_matches(got, want, margin0, margin1, 0.0, f"matcher alone {name}")
    for key in ("P", "matching_scores0", "matching_scores1", "offsets", "matches0", "matches1"):
        assert torch.equal(got[key], again[key]), key        # bit for bit


# ---- 3. running statistics, then eval() ------------------------------------------------------------------------------------------------
def test_running_statistics_and_train_then_eval():
    r = R.reference("a")
    s = r["shape"]
    _, state = hip_forward("a")
    before = R.make_product(s["D"], s["layers"]).state_dict()
    checked, counters = 0, {}
    for name, b in state.items():
        if name.startswith("superglue.kenc."):               # constructed, never used (models/superglue.py:234): the oracle has none
            assert torch.equal(b, before[name]), name
            continue
        if name.endswith("running_mean") or name.endswith("running_var"):
            ref = r["buffers64"][R.oracle_buffer_name(name)]
            err = (b.double() - ref).abs().max().item()
            assert err < 1e-4 * max(1.0, ref.abs().max().item()), (name, err)
            checked += 1
        elif name.endswith("num_batches_tracked"):
            assert int(b) == int(r["buffers64"][R.oracle_buffer_name(name)]), name
            counters[name] = int(b) - int(before[name])
    assert checked == 2 * len(counters) == 2 * (14 + 2 * s["layers"])
    for name, moved in counters.items():
        if name.startswith("superglue.gnn.layers."):
            assert moved == 2, (name, moved)                 # the object tokens, then the hint tokens
        elif name.startswith("object_encoder.pointnet."):
            assert moved == s["B"], (name, moved)            # the PointNet++ runs once per sample
        else:
            assert moved == 1, (name, moved)                 # mlp_pointnet, colour / position encoders, mlp_merge: once per batch
    # train, then evaluate: eval() with the moved buffers against the oracle loaded with them
    prod = R.make_product(s["D"], s["layers"])
    prod.load_state_dict(state, strict=True)
    prod = prod.to(_dev()).eval()
    orc = R.oracle_from(state, s["D"], s["layers"]).eval()
    xyz, rgb, center, mean_rgb, cell_ptr, hints = r["inputs"]
    want = orc.forward_packed(xyz, rgb, center, mean_rgb, cell_ptr, hints)
    with torch.no_grad():
        got = prod.forward_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, hints)
    assert (got.P.cpu() - want["P"]).abs().max().item() < TOL
    assert torch.equal(got.matches0.cpu(), want["matches0"]) and torch.equal(got.matches1.cpu(), want["matches1"])
    assert (got.offsets.cpu() - want["offsets"]).abs().max().item() < TOL


# ---- 4. losses ---------------------------------------------------------------------------------------------------------------------
def _reference_matching_loss(p64, all_matches):
    """training/losses.py:20-30 in float64."""
    per_sample = [(-torch.log(p64[i, torch.as_tensor(m[:, 0]), torch.as_tensor(m[:, 1])])).mean() for i, m in enumerate(all_matches)]
    return torch.stack(per_sample).mean().item(), [float(v) for v in per_sample]


def test_matching_loss_on_a_given_coupling_tensor():
    """Every (object, hint) pair of shape (a) - dustbins included - whose float64 coupling is at least 1e-30: 70-119 entries per
    sample (more than one pass of a wavefront's lanes), a different number in every sample."""
    import text2pos_amd as t2p
    r = R.reference("a")
    got, _ = hip_forward("a")
    p64 = r["out64"]["P"]
    entries = [np.argwhere(p64[i].numpy() >= 1e-30) for i in range(p64.shape[0])]
    assert all(len(e) > 64 for e in entries) and len({len(e) for e in entries}) > 1
    p = got["P"].to(_dev())
    assert min(float(got["P"][i, e[:, 0], e[:, 1]].min()) for i, e in enumerate(entries)) > 0
    crit = t2p.MatchingLoss()
    loss = crit(p, entries)
    want, want_samples = _reference_matching_loss(got["P"].double(), entries)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    print(f"MatchingLoss on the product's P: {loss.item():.7f} against {want:.7f}")
    assert abs(loss.item() - want) < 2e-6 * abs(want)
    assert np.allclose(crit.last_sample_losses.cpu().numpy(), want_samples, rtol=2e-6, atol=0)
    # tensors instead of arrays, int32 instead of int64: the same bits
    again = t2p.MatchingLoss()(p, [torch.from_numpy(e.astype(np.int32)) for e in entries])
    assert torch.equal(loss, again)


@functools.lru_cache(maxsize=None)
def _end_to_end_case():
    from text2pos_amd import synthetic as S
    batch = S.make_fine_batch(901, 4, 16, 6, 64)
    orc = R.oracle_from(R.make_product(128, 2).state_dict(), 128, 2)
    inputs = batch["packed"] + (batch["hint_descriptions"],)
    out64, _ = R.run_oracle(orc, inputs, double=True)
    out32, _ = R.run_oracle(orc, inputs, double=False)
    return batch, out64, out32


def test_matching_loss_end_to_end():
    """The product's train-mode P of a make_fine_batch batch and the batch's all_matches (the entries whose float64 coupling is at
    least 1e-30: the matcher is untrained, a few ground-truth couplings lie below fp32's range) against the float64 oracle's loss."""
    import text2pos_amd as t2p
    batch, out64, out32 = _end_to_end_case()
    p64 = out64["P"]
    entries = [m[p64[i, m[:, 0], m[:, 1]].numpy() >= 1e-30] for i, m in enumerate(batch["all_matches"])]
    kept, listed = sum(len(e) for e in entries), sum(len(m) for m in batch["all_matches"])
    assert all(len(e) >= 1 for e in entries) and kept >= 0.75 * listed, (kept, listed)
    assert min(float(p64[i, e[:, 0], e[:, 1]].min()) for i, e in enumerate(entries)) >= 1e-30
    want, _ = _reference_matching_loss(p64, entries)
    want32, _ = _reference_matching_loss(out32["P"].double(), entries)
    e32 = abs(want32 - want) / abs(want)
    prod = R.make_product(128, 2, _dev()).train()
    xyz, rgb, center, mean_rgb, cell_ptr = batch["packed"]
    with torch.no_grad():
        got = prod.forward_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, batch["hint_descriptions"])
    loss = t2p.MatchingLoss()(got.P, entries).item()
    err = abs(loss - want) / abs(want)
    print(f"MatchingLoss end to end: {loss:.7f} against {want:.7f}: relative {err:.2e} (fp32 oracle {e32:.2e}); {kept} of {listed} entries")
    assert err < max(2e-6, 1.5 * e32), (loss, want, err, e32)


def test_matching_loss_failure_cases():
    import text2pos_amd as t2p
    p = torch.full((3, 5, 4), 0.25, device=_dev())
    good = [np.array([[0, 0], [4, 3]]), np.array([[1, 2]]), np.array([[2, 1], [3, 3], [4, 0]])]
    crit = t2p.MatchingLoss()
    assert abs(crit(p, good).item() - float(-np.log(0.25))) < 2e-6 * float(-np.log(0.25))
    for bad_entry in ([5, 0], [0, 4], [-1, 1], [2 ** 31 + 1, 0]):
        bad = [good[0], np.array([[1, 2], bad_entry], dtype=np.int64), good[2]]
        with pytest.raises(IndexError, match=r"entry 1 of sample 1, \(%d, %d\)" % tuple(bad_entry)):
            crit(p, bad)
    with pytest.raises(RuntimeError, match="sample 1 has no match entries"):
        crit(p, [good[0], np.zeros((0, 2), dtype=np.int64), good[2]])
    with pytest.raises(RuntimeError, match="3 samples in P but 2 match lists"):
        crit(p, good[:2])
    with pytest.raises(RuntimeError, match="integer indices"):
        crit(p, [good[0], np.array([[1.0, 2.0]]), good[2]])
    with pytest.raises(NotImplementedError, match="backward is not built"):
        crit(p.clone().requires_grad_(True), good)
    with pytest.raises(FloatingPointError, match="NaN among the listed couplings"):
        q = p.clone()
        q[1, 1, 2] = float("nan")
        crit(q, good)
    zero = p.clone()
    zero[2, 3, 3] = 0.0                                      # an underflowed coupling: inf, as in the reference
    assert torch.isinf(crit(zero, good)).item()


def test_mse_loss():
    import text2pos_amd as t2p
    crit = t2p.MSELoss()
    g = torch.Generator().manual_seed(11)
    for shape in [(4, 6, 2), (1,), (3, 1000, 7)]:            # offsets-shaped, a single element, more elements than threads
        a, b = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
        want = ((a.double() - b.double()) ** 2).mean().item()
        got = crit(a.to(_dev()), b.to(_dev()))
        assert got.shape == () and got.is_cuda
        assert abs(got.item() - want) < 2e-6 * want, (shape, got.item(), want)
        assert torch.equal(got, crit(a.to(_dev()), b.to(_dev())))
    with pytest.raises(NotImplementedError, match="backward is not built"):
        crit(torch.zeros(2, 2, device=_dev(), requires_grad=True), torch.zeros(2, 2, device=_dev()))
    with pytest.raises(RuntimeError, match="same shape"):
        crit(torch.zeros(2, 2, device=_dev()), torch.zeros(4, device=_dev()))


def test_losses_are_bit_identical_across_calls():
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    got, _ = hip_forward("a")
    batch = S.make_fine_batch(902, 4, 16, 6, 8)
    p = got["P"].to(_dev())
    first = [t2p.MatchingLoss()(p, batch["all_matches"]) for _ in range(3)]
    assert all(torch.equal(first[0], x) for x in first[1:])
    a = got["offsets"].to(_dev())
    b = torch.from_numpy(np.stack(batch["offsets"])).float().to(_dev())
    mse = [t2p.MSELoss()(a, b) for _ in range(3)]
    assert all(torch.equal(mse[0], x) for x in mse[1:]) and np.isfinite(mse[0].item())


# ---- 5. the validation epoch -------------------------------------------------------------------------------------------------------
def test_val_fine_epoch():
    import weights as W
    import text2pos_amd as t2p
    from text2pos_amd import losses as Lo, synthetic as S, training as T
    v = R.vocab()
    args = R.fine_args(128, 2)
    args.pointnet_numpoints = 64
    model = t2p.SuperGlueMatch(v["classes"], v["colors"], v["words"], args)
    W.fill_state_dict(model, R.WEIGHT_SEED)
    model = model.to(_dev()).train()
    twin = copy.deepcopy(model)
    loader = [S.make_fine_batch(31, 3, 16, 6, 64), S.make_fine_batch(32, 3, 16, 6, 64)]
    stats = T.val_fine_epoch(model, loader)
    assert model.training                                    # the reference does not call model.eval() either
    assert set(stats) == {"recall", "precision", "pose_mid", "pose_mean", "pose_offsets"}
    assert all(np.isfinite(x) for x in stats.values()), stats
    want = {k: [] for k in stats}
    with torch.no_grad():
        for batch in loader:
            out = twin(batch["objects"], batch["hint_descriptions"], batch["object_points"])
            m0, m1, off = out.matches0.cpu().numpy(), out.matches1.cpu().numpy(), out.offsets.cpu().numpy()
            recall, precision = Lo.calc_recall_precision(batch["matches"], m0, m1)
            want["recall"].append(recall)
            want["precision"].append(precision)
            want["pose_mid"].append(Lo.calc_pose_error(batch["objects"], m0, batch["poses"], offsets=off, use_mid_pred=True))
            want["pose_mean"].append(Lo.calc_pose_error(batch["objects"], m0, batch["poses"], offsets=None))
            want["pose_offsets"].append(Lo.calc_pose_error(batch["objects"], m0, batch["poses"], offsets=off))
    for k in stats:
        assert stats[k] == pytest.approx(float(np.mean(want[k])), rel=1e-6, abs=1e-9), k
    for (name, a), (_, b) in zip(model.named_buffers(), twin.named_buffers()):
        assert torch.equal(a, b), name                       # both copies moved their running estimates alike
    assert int(model.superglue.gnn.layers[0].mlp[1].num_batches_tracked) == 2 * len(loader)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_train_mode_with_autograd_names_the_missing_backward():
    r = R.reference("d")
    s = r["shape"]
    prod = R.make_product(s["D"], s["layers"], _dev()).train()
    xyz, rgb, center, mean_rgb, cell_ptr, hints = r["inputs"]
    with pytest.raises(NotImplementedError, match="backward of the matcher is not built"):
        prod.forward_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, hints)
    prod.eval()
    with pytest.raises(NotImplementedError, match="forward-only"):
        prod.forward_packed(*_to_dev(xyz, rgb, center, mean_rgb), cell_ptr, hints)


def _launches_nothing(call, exc, match):
    from text2pos_amd import ops
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        with pytest.raises(exc, match=match), torch.no_grad():
            call()
    finally:
        ops.profile_enable(False)
    assert ops.profile_report() == {}


def test_a_single_row_token_set_is_refused_before_any_launch():
    from text2pos_amd import synthetic as S
    prod = R.make_product(128, 1, _dev()).train()
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(707, 1, fixed_n=4, n_pts=8)
    args = _to_dev(xyz, rgb, center, mean_rgb)
    hints = [S.make_texts(808, 0, 1, n_hints=1)]
    _launches_nothing(lambda: prod.forward_packed(*args, cell_ptr, hints), ValueError, "Expected more than 1 value per channel")


def test_unsupported_sizes_are_refused_by_the_new_entry_points():
    from text2pos_amd import _lib as L, ops
    z = lambda *shape: torch.zeros(shape, device=_dev())
    _launches_nothing(lambda: ops.match_attention(z(2 * 22, 3 * 96), 2, 16, 6, False), L.T2PError, "embed_dim=96 not built")
    _launches_nothing(lambda: ops.match_attention(z(2 * 70, 3 * 64), 2, 64, 6, True), L.T2PError, r"1 <= n_obj, n_hints <= 63 \(got 64, 6\)")
    _launches_nothing(lambda: ops.match_head(z(2 * 22, 512), 2, 16, 6, 1.0, 50), L.T2PError, "embed_dim=512 not built")
    _launches_nothing(lambda: ops.match_head(z(2 * 80, 64), 2, 16, 64, 1.0, 50), L.T2PError, r"1 <= n_obj, n_hints <= 63 \(got 16, 64\)")
    _launches_nothing(lambda: ops.match_head(z(2 * 22, 64), 2, 16, 6, 1.0, -1), L.T2PError, "sinkhorn_iters < 0")
    _launches_nothing(lambda: ops.match_attention(z(7, 3 * 64), 2, 16, 6, False), RuntimeError, r"expected \[44, 3 D\]")


def test_the_largest_token_sets_run():
    """63 + 63 tokens at D = 256 and D = 64 with one layer: every output finite, P's column sums those of the optimal-transport
    problem, both sides of every match agree."""
    from text2pos_amd import train_match as TM
    for d in (256, 64):
        prod = R.make_product(d, 1, _dev()).train()
        s = dict(B=2, M=63, N=63, D=d)
        d0, d1 = _unit_descriptors(s, seed=7)
        with torch.no_grad():
            got = _cpu(TM.match_train_forward(prod, d0.to(_dev()), d1.to(_dev())))
        p = got["P"].double()
        assert torch.isfinite(p).all() and torch.isfinite(got["offsets"]).all()
        # the last half step of the iteration normalises the columns: hints sum to 1, the hints' dustbin to the number of objects
        assert (p[:, :, :-1].sum(1) - 1).abs().max().item() < 1e-4 and (p[:, :, -1].sum(1) - 63).abs().max().item() < 1e-2
        m0, m1 = got["matches0"], got["matches1"]
        for b in range(2):
            for o in range(63):
                if m0[b, o] >= 0:
                    assert m1[b, m0[b, o]] == o
            assert int((m0[b] >= 0).sum()) == int((m1[b] >= 0).sum())
