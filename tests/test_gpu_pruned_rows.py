"""SA levels 2 and 3 in the default plan: no FPS of their own (they pick the prefix of level 1's picks; k_build_rows runs their ball
queries one lane per centroid) and no edge rows of repeated dense points (GroupTables::prune_dup, include/t2p.h:
t2p_group_rows_pruned).  tests/test_pruned_rows_host.py states the rule and the restatement used here; every comparison is bit
equality, no tolerance.

The lists are checked against ops.sample_group's tables (the generic kernel: a real FPS at every level) put through the NumPy
restatement, in calls of 1, 67 and 16,500 objects, with and without self-loop rows; the unpruned form of the same kernels against
ops.group_rows; the encoder's and PointNet2's outputs at tuning 0 against the full lists (tuning 4) and the list-mode scans
(tuning 8).  The objects: 96 of the benchmark's stream, k distinct points repeated to 256 for k on both sides of 32 / 64 / 128, a
ball of radius 0.1 (every centroid of every level over the cap), and balls of 100 and of 50 distinct points repeated to 256 (capped
centroids of level 2 / level 3 with more than 32 distinct in-range points AND repeats behind them).
"""
import numpy as np
import pytest
import torch

import test_pruned_rows_host as H

pytestmark = pytest.mark.gpu

N_CENT = H.N_CENT


def _dev():
    return torch.device("cuda:0")


def _ball(rng, k):
    v = rng.normal(size=(k, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True) * (0.095 * rng.uniform(0, 1, (k, 1)) ** (1 / 3))).astype(np.float32)
    assert len(np.unique(v, axis=0)) == k
    return v[np.arange(256) % k]


@pytest.fixture(scope="module")
def objects():
    """xyz, rgb [112, 256, 3]: the hand-made objects first, so that the 67-object call holds all of them."""
    rng = np.random.default_rng(77)
    rx, rc = H.repeated_objects()
    bx = np.stack([_ball(rng, 256), _ball(rng, 100), _ball(rng, 50)])
    bc = rng.uniform(0, 1, (3, 256, 3)).astype(np.float32)
    bc[1], bc[2] = bc[1, np.arange(256) % 100], bc[2, np.arange(256) % 50]      # colours repeat with the positions: true repeats
    sx, sc = H.stream_objects()
    return np.concatenate([rx, bx, sx]), np.concatenate([rc, bc, sc])


@pytest.fixture(scope="module")
def tables(objects):
    """ops.sample_group's tables of the objects, on the host: fps_idx / nbr / cnt [3 levels]."""
    from text2pos_amd import ops
    tab = ops.sample_group(torch.from_numpy(objects[0]).to(_dev()))
    torch.cuda.synchronize()
    return {k: [t.cpu().numpy() for t in tab[k]] for k in ("fps_idx", "nbr", "cnt")}


@pytest.fixture(scope="module")
def expected(objects, tables):
    """(self_loops, share) -> per level (rows int16 [n, n_c * 33] padded with the terminator, n_rows int64 [n]) of the pruned lists."""
    xyz, rgb = objects
    out = {}
    for self_loops in (True, False):
        for share in (True, False):
            rows = [np.full((len(xyz), nc * 33 + 4), 0xFFFF, dtype=np.uint16) for nc in N_CENT]
            n_rows = [np.zeros(len(xyz), dtype=np.int64) for _ in N_CENT]
            for o in range(len(xyz)):
                lists = H.expected_lists([t[o] for t in tables["fps_idx"]], [t[o] for t in tables["nbr"]], [t[o] for t in tables["cnt"]],
                                         xyz[o], rgb[o], self_loops, share, True)
                for l in range(3):
                    assert len(lists[l]) <= N_CENT[l] * 33
                    rows[l][o, :len(lists[l])] = lists[l]
                    n_rows[l][o] = len(lists[l])
            out[(self_loops, share)] = ([r[:, :nc * 33].view(np.int16) for r, nc in zip(rows, N_CENT)], n_rows)
    return out


def _tiled(a, n):
    reps = -(-n // len(a))
    return torch.from_numpy(a).to(_dev()).repeat(reps, *([1] * (a.ndim - 1)))[:n].contiguous()


def _assert_lists(got, want_rows, want_n, n, tag):
    for l in range(3):
        n_got = got["n_rows"][l].view(torch.int16).to(torch.int64) & 0xFFFF
        n_want = _tiled(want_n[l], n)
        assert torch.equal(n_got, n_want), f"{tag}: n_rows of level {l + 1}"
        live = torch.arange(N_CENT[l] * 33, device=_dev())[None, :] < (n_want[:, None] + 4)      # rows + the 4-row terminator
        assert torch.equal(got["rows"][l][live], _tiled(want_rows[l], n)[live]), f"{tag}: rows of level {l + 1}"


def test_the_objects_cover_the_branches(objects, tables, expected):
    """Tails on both sides of every boundary, capped centroids with more than 32 distinct in-range points and repeats behind them at
    levels 2 and 3, every centroid over the cap, and lists that are shorter than the full ones."""
    k1 = np.array([H.first_tail(f) for f in tables["fps_idx"][0]])
    n_rep = len(H.K_DISTINCT)
    assert [int(k) for k in k1[:n_rep]] == [min(k, 128) for k in H.K_DISTINCT]
    assert (tables["cnt"][0][n_rep] == 32).all() and (tables["cnt"][1][n_rep] == 32).all() and (tables["cnt"][2][n_rep] == 32).all()
    assert k1[n_rep] == 128 and k1[n_rep + 1] == 100 and k1[n_rep + 2] == 50
    # the 100-point ball at level 2 and the 50-point ball at level 3: every centroid has all k1 distinct points in range (> 32) and the
    # repeats behind them, so the cap alone keeps dense points 0 .. 31 and nothing is left to drop; the objects of 31 / 63 distinct
    # points have centroids whose repeats sit inside the cap
    for o, l in ((n_rep + 1, 1), (n_rep + 2, 2)):
        assert (tables["nbr"][l][o][:, :32] == np.arange(32)).all() and (tables["cnt"][l][o] == 32).all()
    stream = k1[n_rep + 3:]
    assert (stream < 128).sum() >= 20 and (stream < 64).sum() >= 10 and (stream < 32).sum() >= 2
    from text2pos_amd import ops
    full = ops.group_rows(torch.from_numpy(objects[0]).to(_dev()), share_mask=2)
    for l in (1, 2):
        n_full = (full["n_rows"][l].cpu().numpy().view(np.uint16)).astype(np.int64)
        n_cut = expected[(True, True)][1][l]
        assert (n_cut <= n_full).all() and (n_cut[k1 < (128, 64)[l - 1]] < n_full[k1 < (128, 64)[l - 1]]).any()
    # every stream object with a level-1 tail loses rows (the balls do not: their caps are full of distinct points)
    both = (expected[(True, True)][1][1] + expected[(True, True)][1][2])[n_rep + 3:]
    both_full = sum((full["n_rows"][l].cpu().numpy().view(np.uint16)).astype(np.int64) for l in (1, 2))[n_rep + 3:]
    assert (both[stream < 128] < both_full[stream < 128]).all(), "a stream object with a level-1 tail keeps all its rows"
    assert (both[stream == 128] == both_full[stream == 128]).all()


@pytest.mark.parametrize("self_loops", [True, False], ids=["loops", "no_loops"])
@pytest.mark.parametrize("n_obj", [1, 67, 16500], ids=["one", "67", "16500"])
def test_pruned_lists_equal_the_restatement(objects, tables, expected, n_obj, self_loops):
    """(a) lists and n_rows of all three levels, (b) fps_idx, against the generic kernel's tables."""
    from text2pos_amd import ops
    xyz, rgb = (_tiled(a, n_obj) for a in objects)
    for share in (True, False) if n_obj == 67 else (True,):
        got = ops.group_rows_built(xyz, rgb, self_loops=self_loops, share_mask=2 if share else 0, prune_dup=True)
        torch.cuda.synchronize()
        tag = f"{n_obj} objects, self_loops={self_loops}, share={share}"
        for l in range(3):
            assert torch.equal(got["fps_idx"][l], _tiled(tables["fps_idx"][l], n_obj)), f"{tag}: fps_idx of level {l + 1}"
        _assert_lists(got, *expected[(self_loops, share)], n_obj, tag)


def test_every_handmade_object_alone(objects, tables, expected):
    from text2pos_amd import ops
    for o in range(len(H.K_DISTINCT) + 3):
        xyz, rgb = (torch.from_numpy(a[o:o + 1]).to(_dev()) for a in objects)
        got = ops.group_rows_built(xyz, rgb, share_mask=2, prune_dup=True)
        torch.cuda.synchronize()
        rows, n = expected[(True, True)]
        _assert_lists(got, [r[o:o + 1] for r in rows], [v[o:o + 1] for v in n], 1, f"object {o} alone")


@pytest.mark.parametrize("self_loops", [True, False], ids=["loops", "no_loops"])
@pytest.mark.parametrize("share_mask", [0, 2])
def test_unpruned_form_equals_the_scan_kernels_lists(objects, share_mask, self_loops):
    """(c) with prune_dup = 0 the lane-per-centroid queries write the lists the list-mode scan writes."""
    from text2pos_amd import ops
    xyz, rgb = (torch.from_numpy(a).to(_dev()) for a in objects)
    old = ops.group_rows(xyz, self_loops=self_loops, share_mask=share_mask)
    new = ops.group_rows_built(xyz, rgb, self_loops=self_loops, share_mask=share_mask)
    torch.cuda.synchronize()
    for l in range(3):
        assert torch.equal(old["fps_idx"][l], new["fps_idx"][l]), f"fps_idx of level {l + 1}"
    for l in (1, 2):
        assert torch.equal(old["n_rows"][l], new["n_rows"][l]), f"n_rows of level {l + 1}"
        n = old["n_rows"][l].view(torch.int16).to(torch.int64) & 0xFFFF
        live = torch.arange(N_CENT[l] * 33, device=_dev())[None, :] < (n[:, None] + 4)
        assert torch.equal(old["rows"][l][live], new["rows"][l][live]), f"rows of level {l + 1}"


def _cells(objects, n_pts=256):
    from text2pos_amd import synthetic as S
    xyz, rgb, center, mean_rgb, cell_ptr = (np.ascontiguousarray(a).copy() for a in S.make_cells(SEED_CELLS, 40, n_pts=n_pts))
    if n_pts == 256:
        n_hand = len(H.K_DISTINCT) + 3
        pos = np.linspace(0, len(xyz) - 1, n_hand).astype(np.int64)       # spread over the cells: first, last and in between
        xyz[pos], rgb[pos] = objects[0][:n_hand], objects[1][:n_hand]
    return [torch.from_numpy(a).to(_dev()) for a in (xyz, rgb, center, mean_rgb)], cell_ptr


SEED_CELLS = 20220002


def _model(vocab, oracle_model, precision, **kw):
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    hm = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(**kw), precision=precision)
    hm.load_state_dict(oracle_model.state_dict(), strict=True)      # (the weights do not depend on the points per object)
    return hm.to(_dev()).eval()


@pytest.mark.parametrize("self_loops", [True, False], ids=["loops", "no_loops"])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_outputs_are_bit_identical(vocab, oracle_model, objects, precision, self_loops):
    """(d) encoder and PointNet2 outputs at tuning 0 against the full lists (4) and the list-mode scans (8); the guard word stays 0.
    The encoder prunes the lists only without self-loop rows: a self-loop row takes its source from another object's rows (row
    sbase + c of the cell's flattened batch), so with them a tail centroid's output row is not centroid 0's and the dense point it
    becomes one level up repeats nothing (measured: 13,427 of 13,657 such SA1 rows differ; docs/notebook.md).  With self loops the
    test therefore covers the lane-per-centroid queries, without them the pruned lists as well."""
    args, cell_ptr = _cells(objects)
    hm = _model(vocab, oracle_model, precision)
    hm.add_self_loops = self_loops
    outs, trunk = {}, {}
    pn = hm.object_encoder.pointnet.eval()
    pn.precision, pn.add_self_loops = precision, self_loops
    with torch.no_grad():
        for tuning in (0, 4, 8):
            hm.tuning = tuning
            outs[tuning] = hm.encode_objects_packed(*args, cell_ptr, want_trace=("sa_out", "obj_emb"), check_overflow=False)
            assert hm.overflow_detected() == 0, f"tuning {tuning}: the fp16-range guard fired"
            pn.tuning = tuning
            trunk[tuning] = pn.forward_packed(args[0][:300], args[1][:300])
    pn.tuning = 0
    for t in (4, 8):
        (out_a, tr_a), (out_b, tr_b) = outs[0], outs[t]
        for l in range(3):
            assert torch.equal(tr_a["sa_out"][l], tr_b["sa_out"][l]), f"SA{l + 1} output, tuning 0 against {t}"
        assert torch.equal(tr_a["obj_emb"], tr_b["obj_emb"]), f"obj_emb, tuning 0 against {t}"
        assert torch.equal(out_a, out_b), f"cell embeddings, tuning 0 against {t}"
        for k in ("features0", "features1", "features2"):
            assert torch.equal(getattr(trunk[0], k), getattr(trunk[t], k)), f"PointNet2 {k}, tuning 0 against {t}"


def test_100_points_are_untouched(vocab, oracle_model, objects):
    """(e) the generic path (n_pts != 256) has no pruned form: tuning 0 and 4 give the same bits."""
    args, cell_ptr = _cells(objects, n_pts=100)
    hm = _model(vocab, oracle_model, "f16x3", pointnet_numpoints=100)
    outs = {}
    with torch.no_grad():
        for tuning in (0, 4):
            hm.tuning = tuning
            outs[tuning] = hm.encode_objects_packed(*args, cell_ptr, want_trace=("sa_out", "obj_emb"))
    for l in range(3):
        assert torch.equal(outs[0][1]["sa_out"][l], outs[4][1]["sa_out"][l])
    assert torch.equal(outs[0][1]["obj_emb"], outs[4][1]["obj_emb"]) and torch.equal(outs[0][0], outs[4][0])
