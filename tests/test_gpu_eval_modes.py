"""The evaluation's oracle switches end to end on the GPU (pipeline.evaluate(coarse_mode=, fine_mode=)): the street oracle through
the product model and the group-restricted kernel against a NumPy restatement of evaluation/pipeline.py:93-108 on the embeddings
the model itself returned; the coarse + fine oracles' perfect table; the random modes' reproducibility."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_CELLS, N_POSES, TOP_K, THRESHS = 50, 37, (1, 5, 10), (5, 10, 15)


def _scene(seed=23):
    """50 cells of 30 m on a 10 x 5 grid, 37 poses; every third pose lies up to 6 m outside its own cell (the fine oracle clips)."""
    from text2pos_amd import data as D, synthetic as S
    rng = np.random.default_rng(seed)
    cells, poses = [], []
    dirs = ["north", "south", "east", "west", "on-top"]
    for i in range(N_CELLS):
        objs = []
        for j in range(int(rng.integers(6, 12))):
            c = rng.random(3) * np.array([1.0, 1.0, 0.3])
            n = int(rng.integers(30, 120))
            col = np.clip(rng.random(3), 0, 1)
            objs.append(D.Object3d(j, 1000 * i + j, c + 0.05 * rng.standard_normal((n, 3)),
                                   np.clip(col + 0.05 * rng.standard_normal((n, 3)), 0, 1), S.LABELS[int(rng.integers(0, len(S.LABELS)))]))
        x, y = 30.0 * (i % 10), 30.0 * (i // 10)
        cells.append(D.Cell(i, "toy1", objs, 30.0, np.array([x, y, 0.0, x + 30.0, y + 30.0, 10.0])))
    for q in range(N_POSES):
        c = cells[int(rng.integers(0, N_CELLS))]
        descs = [D.DescriptionBestCell(dirs[int(rng.integers(0, 5))], o.get_color_text(), o.label, o.id, True)
                 for o in [c.objects[int(k)] for k in rng.choice(len(c.objects), 6, replace=False)]]
        in_cell = rng.random(3) * np.array([30.0, 30.0, 10.0])
        if q % 3 == 0:
            in_cell[0] = 30.0 + 6.0 * rng.random()
        poses.append(D.Pose(in_cell / 30.0, c.bbox_w[0:3] + in_cell, c.id, "toy1", descs))
    return cells, poses


def test_evaluation_modes_end_to_end(hip_model, tmp_path):
    from threadpoolctl import threadpool_limits
    import text2pos_amd as t2p
    from text2pos_amd import evaluation as E, io as IO, pipeline as PL
    cells, poses = _scene()
    sc = IO.Scenes(cells, poses)
    tf = PL.PerCellTransform(256, 5)
    IO.save_street_centers(str(tmp_path), "toy1", np.array([[45.0, 75.0, 5.0], [150.0, 40.0, 5.0], [255.0, 110.0, 5.0]]))
    streets = IO.load_street_centers(str(tmp_path), "toy1")
    assert streets.shape == (3, 3) and streets.dtype == np.float64
    cg, qg = E.street_groups(cells, poses, streets)
    assert len(set(cg.tolist())) == 3
    kmax = max(TOP_K)

    # ---- street: the grouped kernel on the model's own embeddings ----
    seen = []

    def spy(q, c, k, cell_groups, query_groups):
        seen.append((q.detach().cpu().numpy().copy(), c.detach().cpu().numpy().copy(), np.array(cell_groups), np.array(query_groups)))
        return t2p.retrieve_topk(c, q, k, cell_groups=cell_groups, query_groups=query_groups)

    out = PL.evaluate(hip_model, None, sc, tf, top_k=TOP_K, threshs=THRESHS, coarse_mode="street", street_centers=streets, topk_fn=spy)
    assert len(seen) == 1
    q_emb, c_emb, cg_seen, qg_seen = seen[0]
    assert q_emb.shape[0] == N_POSES and c_emb.shape[0] == N_CELLS                     # no query is left out
    assert np.array_equal(cg_seen, cg) and np.array_equal(qg_seen, qg)
    c64, q64 = c_emb.astype(np.float64), q_emb.astype(np.float64)
    ids = [c.id for c in cells]
    want = []
    with threadpool_limits(limits=1, user_api="blas"):
        for i in range(N_POSES):
            s = c64 @ q64[i]
            s[cg != qg[i]] = -np.inf
            order = np.argsort(-1.0 * s, kind="stable")
            top = s[order[:kmax + 1]]
            gaps = -np.diff(top[np.isfinite(top)])
            assert ((gaps == 0) | (gaps > 1e-10)).all(), "a near-tie inside the top k + 1"
            want.append([ids[j] for j in order[:kmax]])
    assert len(out["retrievals"]) == N_POSES and out["retrievals"] == want
    # without a spy the same call ranks through retrieve_topk's grouped path, with the same result
    retr, acc = PL.run_coarse(hip_model, sc, tf, TOP_K, THRESHS, coarse_mode="street", street_centers=streets)
    assert retr == want and set(acc) == {"hit", "close", "localisation"}
    street_of = dict(zip(ids, cg.tolist()))
    for i, r in enumerate(retr):
        n_own = int((cg == qg[i]).sum())
        assert all(street_of[cid] == qg[i] for cid in r[:min(kmax, n_own)])
    plain, _ = PL.run_coarse(hip_model, sc, tf, TOP_K, THRESHS)
    assert plain != retr                                                               # (the restriction does restrict)

    # ---- coarse oracle + fine oracle: perfect from the largest clip residual on ----
    resid = 0.0
    for p in poses:
        c = sc.cells_dict[p.cell_id]
        pred = c.bbox_w[0:2] + np.clip((p.pose_w[0:2] - c.bbox_w[0:2]) / c.cell_size, 0, 1) * c.cell_size
        resid = max(resid, float(np.linalg.norm(p.pose_w[0:2] - pred)))
    assert 0.0 < resid <= 6.0
    perfect = PL.evaluate(None, None, sc, tf, top_k=(1,), threshs=THRESHS, coarse_mode="oracle", fine_mode="oracle")
    assert perfect["retrievals"] == [[p.cell_id] for p in poses] and perfect["hit"] == {1: 1.0}
    assert set(perfect["fine_oracle"]) == {1} and set(perfect["fine_oracle"][1]) == set(THRESHS)
    assert any(t >= resid for t in THRESHS)
    for t in THRESHS:
        if t >= resid:
            assert perfect["fine_oracle"][1][t] == 1.0
    with pytest.raises(ValueError, match="max\\(top_k\\) must be 1"):
        PL.evaluate(None, None, sc, tf, top_k=TOP_K, threshs=THRESHS, coarse_mode="oracle")

    # ---- random: runs, reproducible, seeded ----
    a = PL.evaluate(None, None, sc, tf, top_k=TOP_K, threshs=THRESHS, coarse_mode="random", fine_mode="random", seed=3)
    b = PL.evaluate(None, None, sc, tf, top_k=TOP_K, threshs=THRESHS, coarse_mode="random", fine_mode="random", seed=3)
    c = PL.evaluate(None, None, sc, tf, top_k=TOP_K, threshs=THRESHS, coarse_mode="random", fine_mode="random", seed=4)
    assert a["retrievals"] == b["retrievals"] and a["fine_oracle"] == b["fine_oracle"] and a["localisation"] == b["localisation"]
    assert a["retrievals"] != c["retrievals"]
    assert all(len(r) == kmax and set(r) <= set(ids) for r in a["retrievals"])
