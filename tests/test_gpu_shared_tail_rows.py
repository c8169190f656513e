"""SA level 2 lists the edge rows of repeated FPS centroids once (GroupTables::share_tail, include/t2p.h: t2p_group_rows_shared).

T.FixedPoints(256) draws with replacement, so an object with d < 256 base points has d distinct positions.  FPS takes each once and
then picks point 0 for the rest of the level: those TAIL centroids (c > 0, fps_idx[c] == 0) repeat centroid 0's ball-query hits, and
the row list k_sa_rows consumes carries them once, under a pseudo-centroid code, plus one self-loop row per tail centroid.
A tail exists at level 3 / 2 / 1 iff d < 32 / 64 / 128; the 13 objects below sit on both sides of each boundary.
Levels 1 and 3 keep full lists (level 3's kernel lost more to the extra slot than the 1 % of rows gave: docs/notebook.md), which
the test checks as well.

The row-list contract is checked against ops.sample_group's tables, the outputs bit for bit against the full lists (tuning bit 2),
and the cells against the CPU oracle through the gate every cell test uses (tests/knn_graph.py, no tolerance of its own).

One figure differs from the issue that asked for this test: it expected "exactly 1 + NC rows" at a shared level for the object whose
256 points are one point.  By the contract it states itself (and by this test's multiset comparison) that object has centroid 0's
32 hits (the neighbour cap) + its loop, the 32 hits once more under the shared code, and NC - 1 loops of the tail: 64 + NC rows
(against 33 NC in the full list).  The test asserts 64 + NC.
"""
import numpy as np
import pytest
import torch

import knn_graph as KG

pytestmark = pytest.mark.gpu

CELL_PTR = np.array([0, 1, 4, 13], dtype=np.int32)
# distinct points per object (None: untouched; "xyz": 10 distinct positions under 256 untouched colours).  The 1-object cell holds a
# tail object; in the other cells tail objects stand first, in the middle and last (the aliased self-loop rows cross objects).
DISTINCT = [20, 31, None, 64, 1, 100, 128, 32, "xyz", 33, 65, 2, 63]
TAIL_CODE = {1: 64}            # pseudo-centroid code per shared level index
SHARE_MASK = 0b010


def _dev():
    return torch.device("cuda:0")


def _to_dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) for a in arrays]


@pytest.fixture(scope="module")
def cells():
    from text2pos_amd import synthetic as S
    xyz, rgb, center, mean_rgb = (a.copy() for a in S.make_objects(4242, 0, 13))
    rng = np.random.default_rng(7)
    for o, d in enumerate(DISTINCT):
        if d is None:
            continue
        k = 10 if d == "xyz" else d
        # the object's first k DISTINCT positions (the synthetic stream itself draws with replacement), every one of them present
        _, first = np.unique(xyz[o], axis=0, return_index=True)
        base = np.sort(first)[:k]
        assert len(base) == k, f"object {o} has {len(first)} distinct positions, {k} wanted"
        idx = rng.permutation(np.concatenate([base, base[rng.integers(0, k, 256 - k)]]))
        xyz[o] = xyz[o][idx]
        if d != "xyz":
            rgb[o] = rgb[o][idx]
    return xyz, rgb, center, mean_rgb, CELL_PTR


@pytest.fixture(scope="module")
def oracle_run(oracle_model, cells):
    """The oracle's cell embeddings and trace, computed once for the f16x3 and fp32 gates."""
    tr = []
    want = oracle_model.encode_objects_packed(*cells, trace=tr).numpy()
    return want, tr


def _gate(om, got, gtr, want, wtr, cell_ptr, tag):
    """tests/knn_graph.py: 1e-4 on the kNN graph the kernel chose, flips proven near-ties (the gate of tests/test_gpu_numpoints.py)."""
    got_knn = KG.global_knn(gtr["knn_idx"].cpu().numpy(), cell_ptr)
    viol = KG.knn_violation(got_knn, KG.normalized64(gtr["obj_emb"]), cell_ptr)
    assert viol <= 0, f"{tag}: a chosen neighbour is farther than an unchosen one by {viol:.2e} beyond fp32 rounding"
    emb = [d for d in wtr if "object_embeddings" in d][0]["object_embeddings"].numpy()
    flips, resolved, gap = KG.check_cells(np.asarray(got), got_knn, np.asarray(want), KG.oracle_knn(emb, cell_ptr), emb, cell_ptr,
                                          KG.float64_oracle(om), tag)
    assert len(flips) <= 1, f"{tag}: {len(flips)} cells with a kNN near-tie flip"


def _expected_rows(fps, nbr, cnt, level, shared, self_loops):
    """Sorted u16 rows of one object from its FPS indices / neighbour table / counts."""
    nc = fps.shape[0]
    rows, tail_open = [], False
    for c in range(nc):
        tail = shared and c > 0 and fps[c] == 0
        loop = [((c | 0x80) << 8) | c] if self_loops else []
        if tail and tail_open:
            rows += loop
            continue
        code = TAIL_CODE[level] if tail else c
        rows += [(code << 8) | int(j) for j in nbr[c, :cnt[c]]] + loop
        tail_open = tail_open or tail
    return np.sort(np.array(rows, dtype=np.int64))


@pytest.mark.parametrize("self_loops", [True, False], ids=["loops", "no_loops"])
def test_row_list_contract(cells, self_loops):
    from text2pos_amd import ops
    xyz = _to_dev(cells[0])[0]
    tab = ops.sample_group(xyz)
    full = ops.group_rows(xyz, self_loops=self_loops, share_mask=0)
    got = ops.group_rows(xyz, self_loops=self_loops, share_mask=SHARE_MASK)
    torch.cuda.synchronize()
    for l in range(3):
        fps, nbr, cnt = (tab[k][l].cpu().numpy() for k in ("fps_idx", "nbr", "cnt"))
        assert np.array_equal(got["fps_idx"][l].cpu().numpy(), fps), f"level {l + 1}: fps_idx changed"
        rows = got["rows"][l].cpu().numpy().view(np.uint16)
        n_rows = got["n_rows"][l].cpu().numpy().view(np.uint16)
        shared = bool(SHARE_MASK >> l & 1)
        nc = fps.shape[1]
        for o in range(len(DISTINCT)):
            want = _expected_rows(fps[o], nbr[o], cnt[o], l, shared, self_loops)
            assert n_rows[o] == len(want), f"object {o} level {l + 1}: n_rows {n_rows[o]}, expected {len(want)}"
            assert np.array_equal(np.sort(rows[o, :n_rows[o]].astype(np.int64)), want), f"object {o} level {l + 1}: rows differ"
            term = rows[o, n_rows[o]:min(n_rows[o] + 4, nc * 33)]
            assert (term == 0xFFFF).all(), f"object {o} level {l + 1}: terminator"
            has_tail = bool((fps[o, 1:] == 0).any())
            d = 10 if DISTINCT[o] == "xyz" else (256 if DISTINCT[o] is None else DISTINCT[o])
            assert has_tail == (d < (128, 64, 32)[l]), f"object {o} level {l + 1}: tail {has_tail} with {d} distinct points"
        full_n = full["n_rows"][l].cpu().numpy().view(np.uint16).astype(np.int64)
        if shared:
            assert n_rows.astype(np.int64).sum() < full_n.sum(), f"level {l + 1}: no row was dropped"
            if self_loops:
                assert n_rows[DISTINCT.index(1)] == 64 + nc     # one point: 32 hits + loop, 32 shared hits, nc - 1 loops (docstring)
        else:
            assert np.array_equal(n_rows, full_n.astype(np.uint16))
            full_rows = full["rows"][l].cpu().numpy().view(np.uint16)
            for o in range(len(DISTINCT)):       # (the slots behind a list's terminator are never written: compared up to n_rows)
                assert np.array_equal(rows[o, :n_rows[o]], full_rows[o, :n_rows[o]]), f"object {o}: level {l + 1} is not shared"


def _pair_model(vocab, oracle_model, precision, self_loops=True):
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    hm = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(), precision=precision)
    hm.load_state_dict(oracle_model.state_dict(), strict=True)
    hm.add_self_loops = self_loops
    return hm.to(_dev()).eval()


@pytest.mark.parametrize("self_loops", [True, False], ids=["loops", "no_loops"])
def test_same_bits_as_full_lists(vocab, oracle_model, cells, self_loops):
    hm = _pair_model(vocab, oracle_model, "f16x3", self_loops)
    args, cell_ptr = _to_dev(*cells[:4]), cells[4]
    outs = {}
    with torch.no_grad():
        for tuning in (0, 4):
            hm.tuning = tuning
            outs[tuning] = hm.encode_objects_packed(*args, cell_ptr, want_trace=("sa_out", "obj_emb"))
        hm.tuning = 0
        two = hm.encode_objects_packed(*args, cell_ptr, streams=2)
    (out0, tr0), (out4, tr4) = outs[0], outs[4]
    for l in range(3):
        assert torch.equal(tr0["sa_out"][l], tr4["sa_out"][l]), f"SA{l + 1} output depends on the shared tail rows"
    assert torch.equal(tr0["obj_emb"], tr4["obj_emb"]) and torch.equal(out0, out4)
    assert torch.equal(two, out0), "two streams"


def test_cells_vs_oracle_f16x3(vocab, oracle_model, oracle_run, cells):
    hm = _pair_model(vocab, oracle_model, "f16x3")
    want, wtr = oracle_run
    with torch.no_grad():
        got, gtr = hm.encode_objects_packed(*_to_dev(*cells[:4]), cells[4], want_trace=("obj_emb", "knn_idx"))
    _gate(oracle_model, got.cpu().numpy(), gtr, want, wtr, cells[4], "shared tail rows f16x3")


def test_cells_vs_oracle_fp32_full_lists(vocab, oracle_model, oracle_run, cells):
    hm = _pair_model(vocab, oracle_model, "fp32")
    want, wtr = oracle_run
    with torch.no_grad():
        got, gtr = hm.encode_objects_packed(*_to_dev(*cells[:4]), cells[4], want_trace=("obj_emb", "knn_idx"))
    _gate(oracle_model, got.cpu().numpy(), gtr, want, wtr, cells[4], "fp32, full lists")
