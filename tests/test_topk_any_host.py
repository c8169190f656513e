"""Host side of "top-k for any k up to 1,024": the workspace arithmetic of t2p_sim_topk (no GPU needed: the size query only
computes) against the formula include/t2p.h documents, and the pipeline's early refusal of a top_k beyond the limit."""
import numpy as np
import pytest
import torch

MIB = 1 << 20
SHAPES = [(1000, 12000), (1250, 100000), (10000, 1000000)]


def _macro(name):
    """An integer limit as the binding read it from include/t2p.h; the tile size is a cast expression there, so it is matched as text."""
    from text2pos_amd import _lib
    if name == "T2P_SIM_TOPK_TILE_BYTES":
        with open(_lib.HEADER) as f:
            assert "#define T2P_SIM_TOPK_TILE_BYTES ((size_t)256 << 20)" in f.read()
        return 256 << 20
    return _lib.DEFINES[name]


def _documented_bytes(nq, nc):
    """include/t2p.h, retrieval block, k > T2P_SIM_TOPK_REG_K: one chunk of queries' float64 scores.
    ld = ceil(nc / 16) * 16;  row = 8 * ld;  cap = floor((TILE - 256) / row), rounded DOWN to a multiple of 128 when >= 128;
    chunk = min(nq, cap);  bytes = chunk * row + 256."""
    tile = _macro("T2P_SIM_TOPK_TILE_BYTES")
    row = 8 * ((nc + 15) // 16 * 16)
    cap = (tile - 256) // row
    if cap >= 128:
        cap = cap // 128 * 128
    return min(nq, cap) * row + 256, cap


def _ws(nq, nc, k):
    import text2pos_amd  # noqa: F401
    from text2pos_amd import _lib as L
    return int(L.lib().t2p_sim_topk_workspace_bytes(nq, nc, k))


def test_header_states_the_range():
    assert _macro("T2P_SIM_TOPK_MAX_K") == 1024 and _macro("T2P_SIM_TOPK_REG_K") == 16
    assert _macro("T2P_SIM_TOPK_TILE_BYTES") == 256 * MIB
    from text2pos_amd import retrieval
    assert retrieval.MAX_TOP_K == _macro("T2P_SIM_TOPK_MAX_K")


@pytest.mark.parametrize("k", [17, 1024])
@pytest.mark.parametrize("nq,nc", SHAPES)
def test_workspace_is_bounded_and_as_documented(nq, nc, k):
    got = _ws(nq, nc, k)
    want, cap = _documented_bytes(nq, nc)
    assert got == want
    assert got <= 256 * MIB                      # the score tile alone: no term in nq * k is needed
    assert got < 256 * MIB + 64 * nq * k         # the stated bound: 256 MiB + a term linear in nq * k
    # monotone in nq, constant from the chunk size on
    sizes = [_ws(n, nc, k) for n in sorted({1, 2, 100, 127, 128, 129, 255, 256, 257, max(cap - 1, 1), cap, cap + 1, 2 * cap, nq})]
    assert sizes == sorted(sizes)
    assert _ws(cap, nc, k) == _ws(cap + 1, nc, k) == _ws(100 * cap, nc, k)
    assert _ws(nq, nc, 17) == _ws(nq, nc, 1024)


def test_small_k_workspace_does_not_depend_on_k():
    for nq, nc in SHAPES[:2] + [(130, 1000), (1, 1)]:
        assert len({_ws(nq, nc, k) for k in (1, 10, 16)}) == 1
    assert _ws(0, 1000, 10) >= 0 and _ws(0, 1000, 100) >= 0      # the size query of an empty call


def test_one_query_too_large_for_the_tile():
    """8 * nc bytes beyond the tile: the size query has nothing to offer (the call itself refuses with T2P_E_ARG)."""
    nc = 256 * MIB // 8 + 1
    assert _documented_bytes(1, nc)[1] == 0 and _ws(1, nc, 100) == 256


# ---- pipeline: the ValueError comes before the model is asked for anything -----------------------------------------------
def _toy_scene(seed=11, n_cells=13, n_poses=21):
    from text2pos_amd import data as D, synthetic as S
    rng = np.random.default_rng(seed)
    cells, poses = [], []
    dirs = ["north", "south", "east", "west", "on-top"]
    for i in range(n_cells):
        objs = []
        for j in range(int(rng.integers(6, 12))):
            c = rng.random(3) * np.array([1.0, 1.0, 0.3])
            n = int(rng.integers(30, 90))
            objs.append(D.Object3d(j, 1000 * i + j, c + 0.05 * rng.standard_normal((n, 3)),
                                   np.repeat(np.clip(rng.random((1, 3)), 0, 1), n, axis=0),
                                   S.LABELS[int(rng.integers(0, len(S.LABELS)))]))
        x, y = 30.0 * (i % 4), 30.0 * (i // 4)
        cells.append(D.Cell(i, "toy1", objs, 30.0, np.array([x, y, 0.0, x + 30.0, y + 30.0, 10.0])))
    for q in range(n_poses):
        c = cells[int(rng.integers(0, n_cells))]
        descs = [D.DescriptionBestCell(dirs[int(rng.integers(0, 5))], o.get_color_text(), o.label, o.id, True)
                 for o in [c.objects[int(k)] for k in rng.integers(0, len(c.objects), 6)]]
        poses.append(D.Pose(rng.random(3), c.bbox_w[0:3] + rng.random(3) * 30.0, c.id, "toy1", descs))
    return cells, poses


class _StubCoarse:
    """CPU stand-in with the CellRetrievalNetwork surface run_coarse uses; counts what it is asked to encode."""
    embed_dim, device = 16, torch.device("cpu")

    def __init__(self):
        self.calls = 0

    def encode_objects(self, objects, object_points):
        self.calls += 1
        rows = [torch.sin(torch.arange(1, 17) * float(len(objs) + pts.pos.double().sum())) for objs, pts in zip(objects, object_points)]
        return torch.nn.functional.normalize(torch.stack(rows).float(), dim=-1)

    def encode_text(self, texts):
        self.calls += 1
        rows = [torch.tensor([(sum(map(ord, t)) * (i + 3)) % 97 / 97.0 - 0.5 for i in range(self.embed_dim)]) for t in texts]
        return torch.nn.functional.normalize(torch.stack(rows).float(), dim=-1)


def _topk(queries, cells, k):
    from oracle.model import retrieve_topk_f64
    idx, sc = retrieve_topk_f64(cells.numpy(), queries.numpy(), k)
    return torch.from_numpy(idx), torch.from_numpy(sc)


def test_pipeline_refuses_top_k_beyond_the_limit_before_encoding():
    import text2pos_amd  # noqa: F401
    from text2pos_amd import io as IO, pipeline as PL
    cells, poses = _toy_scene()
    sc = IO.Scenes(cells, poses)
    model = _StubCoarse()
    for top_k in ((1, 1025), (1, 5, 2000), (0, 5)):
        with pytest.raises(ValueError, match="1024"):
            PL.run_coarse(model, sc, PL.PerCellTransform(64, 3), top_k, (5, 10, 15), topk_fn=_topk)
        with pytest.raises(ValueError, match="1024"):
            PL.evaluate(model, None, sc, PL.PerCellTransform(64, 3), top_k=top_k, topk_fn=_topk)
    assert model.calls == 0
    with pytest.raises(ValueError, match="1024"):                 # the command line: before the dataset is opened
        PL.main(["--base_path", "/nonexistent", "--path_coarse", "/nonexistent", "--top_k", "1", "5", "10", "1025"])
    # inside the limit the same call goes through (13 cells: the 12 of 13 asked for, in one ranking)
    retr, acc = PL.run_coarse(model, sc, PL.PerCellTransform(64, 3), (1, 12), (5, 10, 15), topk_fn=_topk)
    assert model.calls > 0 and all(len(r) == 12 and len(set(r)) == 12 for r in retr) and set(acc["hit"]) == {1, 12}
