"""CPU tests of the oracle's explicit-graph cell head (OracleCellRetrieval.cell_head, DynamicEdgeConv(knn=...)) and of the kNN
gate in tests/knn_graph.py: the gate accepts a genuine near-tie flip and catches what the earlier count-bar rules let through."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import knn_graph as KG
from oracle import model as OM, pyg_restated as gnn

SIZES = [1, 2, 7, 8, 9, 30]          # below, at and above k = 8: lists padded with -1, full, and chosen from more


@pytest.fixture(scope="module")
def small_cells():
    from text2pos_amd import synthetic as S
    xyz, rgb, center, mean_rgb = S.make_objects(5, 0, sum(SIZES))
    ptr = np.zeros(len(SIZES) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(SIZES)
    return xyz, rgb, center, mean_rgb, ptr


@pytest.mark.parametrize("variation", [0, 1])
def test_cell_head_is_the_tail_of_encode_objects_packed(vocab, small_cells, variation):
    """cell_head(emb) and cell_head(emb, knn=<the oracle's own list>) give encode_objects_packed's bits (variation 0: max
    aggregation, 1: mean, whose sums keep knn()'s edge order); on a float64 copy the same two agree bit for bit, and slices of
    whole cells give the same cells."""
    import weights as W
    om = OM.OracleCellRetrieval(vocab["classes"], vocab["colors"], vocab["words"], OM.default_args(variation=variation)).eval()
    W.fill_state_dict(om, 11)
    xyz, rgb, center, mean_rgb, ptr = small_cells
    tr = []
    want = om.encode_objects_packed(xyz, rgb, center, mean_rgb, ptr, trace=tr)
    emb = [d for d in tr if "object_embeddings" in d][0]["object_embeddings"]
    own = KG.oracle_knn(emb, ptr)
    assert (own[: ptr[3]] == -1).any() and (own >= 0).sum(1).tolist() == sum(([min(8, n)] * n for n in SIZES), [])
    with torch.no_grad():
        assert torch.equal(om.cell_head(emb, ptr), want)
        assert torch.equal(om.cell_head(emb, ptr, knn=own), want)
        assert torch.equal(om.cell_head(emb, ptr, knn=torch.from_numpy(own)), want)
        assert (om.cell_head(emb, ptr, chunk_objects=10) - want).abs().max().item() < 1e-6
        om64 = KG.float64_oracle(om)
        h64 = om64.cell_head(emb, ptr)
        batch = torch.arange(len(SIZES)).repeat_interleave(torch.tensor(SIZES))
        own64 = gnn.knn_table(F.normalize(emb.double(), dim=-1), 8, batch)     # the float64 head's own graph
        assert h64.dtype == torch.float64 and torch.equal(om64.cell_head(emb, ptr, knn=own64), h64)
        assert (om64.cell_head(emb, ptr, chunk_objects=10) - h64).abs().max().item() < 1e-12
    assert (h64 - want.double()).abs().max().item() < 1e-5
    assert np.array_equal(KG.cell_head64(om64, emb, ptr, knn=own64), h64.numpy())


def test_global_knn_takes_the_chunk_of_the_call():
    g = KG.global_knn(np.array([[0, 1], [1, -1], [0, 1], [1, 0]]), np.array([0, 2, 4]), chunk_objects=2)
    assert g.tolist() == [[0, 1], [1, -1], [2, 3], [3, 2]]
    # cells of 3, 4, 5 objects in chunks of 7: [cell 0, cell 1], [cell 2]
    knn = np.zeros((12, 1), dtype=np.int64)
    assert KG.global_knn(knn, np.array([0, 3, 7, 12]), 7)[:, 0].tolist() == [0] * 7 + [7] * 5


def _tie_case(seed=3):
    """Object embeddings [n, 256] of 100 cells.  Cell 0 holds 12 objects: object 0 = e0, object j = c_j e0 + s_j e_j, so that
    object 0's squared distance to object j is d2[j - 1]; its 8th and 9th neighbours (self included: objects 7 and 8) tie to
    3e-6, and object 11 lies far off (1.1).  The other 99 cells are random, of 1 to 20 objects."""
    rng = np.random.default_rng(seed)
    d2 = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.7 + 3e-6, 0.9, 1.0, 1.1])
    c = 1.0 - d2 / 2.0
    cell0 = np.zeros((12, 256))
    cell0[0, 0] = 1.0
    cell0[1:, 0] = c
    cell0[np.arange(1, 12), np.arange(1, 12)] = np.sqrt(1.0 - c * c)
    sizes = [12] + rng.choice([1, 2, 5, 8, 9, 12, 20], 99).tolist()
    emb = np.concatenate([cell0 * rng.uniform(0.5, 2.0, (12, 1)), rng.standard_normal((sum(sizes) - 12, 256))])
    ptr = np.zeros(len(sizes) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(sizes)
    return torch.from_numpy(emb.astype(np.float32)), ptr


def _old_rules_accept(got, want, flips, gap):
    """The acceptance rules the cell gates had before check_cells: (a) the oracle-encoded database / configs[4] gates,
    `flipped = per_cell >= 1e-4` with at most 1 % of the cells; (b) the numpoints / fuzz gates, at most one cell beyond 1e-4
    and below 0.2; (c) the headline sample, every list difference a near-tie and the flipped cells left out."""
    per_cell = np.abs(got - want).max(axis=1)
    bad = np.flatnonzero(per_cell >= KG.TOL)
    ok = np.ones(len(per_cell), dtype=bool)
    ok[flips] = False
    return (len(bad) <= len(per_cell) // 100,
            len(bad) <= 1 and (len(bad) == 0 or per_cell[bad].max() < 0.2),
            gap < KG.TOL and (per_cell[ok] < KG.TOL).all())


def test_checker_resolves_a_near_tie_and_catches_what_the_old_rules_let_through(oracle_model):
    emb, ptr = _tie_case()
    with torch.no_grad():
        want = oracle_model.cell_head(emb, ptr).numpy()
    want_knn = KG.oracle_knn(emb, ptr)
    assert want_knn[0].tolist() == list(range(8))            # object 0: itself and objects 1 .. 7; object 8 is 9th by 3e-6
    embn64 = KG.normalized64(emb)
    assert KG.knn_violation(want_knn, embn64, ptr) <= 0      # the oracle's own graph
    om64 = KG.float64_oracle(oracle_model)

    def kernel_run(knn):                                      # a kernel that evaluates the head correctly on graph `knn`
        return KG.cell_head64(om64, emb, ptr, knn=knn).astype(np.float32)

    # (1) the 8th neighbour swapped at the tie: a legitimate kNN graph, and the cell resolves within 1e-4 on it
    tie = want_knn.copy()
    tie[0, 7] = 8
    assert KG.knn_violation(tie, embn64, ptr) <= 0
    got = kernel_run(tie)
    flips, resolved, gap = KG.check_cells(got, tie, want, want_knn, emb.numpy(), ptr, om64, "near-tie swap")
    assert flips.tolist() == [0] and resolved < 1e-6 and gap < 1e-5
    moved = float(np.abs(got[0] - want[0]).max())
    assert moved > KG.TOL                                    # (the flip matters: excluding the cell would hide it)
    print(f"near-tie swap: cell 0 moves by {moved:.2e} from the oracle's own graph, {resolved:.2e} from the resolved reference")
    # (2) swapped with a far object: not a kNN graph, not a near-tie
    far = want_knn.copy()
    far[0, 7] = 11
    assert KG.knn_violation(far, embn64, ptr) > 0.3
    assert KG.knn_flips(far, want_knn, embn64, ptr)[1] > 0.3
    got_far = kernel_run(far)
    with pytest.raises(AssertionError, match="not a near-tie"):
        KG.check_cells(got_far, far, want, want_knn, emb.numpy(), ptr, om64, "far swap")
    assert all(_old_rules_accept(got_far, want, [0], 0.0)[:2])            # (a) and (b) never looked at the graph
    # (3) the near-tie cell moved by 2e-4 more: check_cells refuses it; every old rule accepted it
    bent = got.copy()
    bent[0, int(np.argmax(np.abs(bent[0])))] += 2e-4
    with pytest.raises(AssertionError, match="kNN graph the kernel chose"):
        KG.check_cells(bent, tie, want, want_knn, emb.numpy(), ptr, om64, "near-tie swap, moved")
    assert all(_old_rules_accept(bent, want, KG.knn_flips(tie, want_knn, embn64, ptr)[0], gap))
    # (4) an unflipped cell moved by 2e-4 is refused as well
    other = got.copy()
    other[5, 0] += 2e-4
    with pytest.raises(AssertionError, match="oracle's kNN graph"):
        KG.check_cells(other, tie, want, want_knn, emb.numpy(), ptr, om64, "other cell moved")


def test_knn_violation_checks_the_list_structure():
    emb, ptr = _tie_case(5)
    embn64 = KG.normalized64(emb)
    knn = KG.oracle_knn(emb, ptr)
    small = int(np.flatnonzero(np.diff(ptr) == 2)[0])        # a 2-object cell: two entries, then -1
    o = int(ptr[small])
    for row, col, val, msg in ((0, 3, 0, "twice"), (0, 3, int(ptr[1]), "outside"), (0, 7, -1, "outside"),
                               (o, 2, o, "past")):
        bad = knn.copy()
        bad[row, col] = val
        with pytest.raises(AssertionError, match=msg):
            KG.knn_violation(bad, embn64, ptr)
    # an object that lists a neighbour of another cell is refused by check_cells too
    bad = knn.copy()
    bad[0, 7] = int(ptr[1])
    with pytest.raises(AssertionError, match="outside its cell"):
        KG.check_cells(np.zeros((len(ptr) - 1, 256)), bad, np.zeros((len(ptr) - 1, 256)), knn, emb.numpy(), ptr, None, "x")
