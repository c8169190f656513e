"""Randomised shapes of the cell branch against the CPU oracle (a tool, not collected by pytest):
    python tests/tools/fuzz_cells.py [trials] [first_seed]        (GPU box, repo root)
Cells of 1 .. 150 objects, objects built from 2 / 3 / 5 distinct points, collinear objects, clouds squeezed into a corner
of the unit cube (every ball-query neighbourhood hits the 32-neighbour cap), tiny clouds around the origin (no neighbour but
the point itself), next to ordinary synthetic objects.  Integer stages must match bit for bit, the SA outputs and object
embeddings within 1e-4, the kernel's kNN lists a kNN graph of its own object embeddings, and every cell embedding within 1e-4:
of the oracle's where the kNN graphs agree, of the float64 oracle head on the kernel's graph where a proven near-tie flipped
(tests/knn_graph.py; at most one such cell per case)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_graph as KG  # noqa: E402
import weights as W  # noqa: E402
import text2pos_amd as t2p  # noqa: E402
from oracle import model as OM  # noqa: E402
from text2pos_amd import synthetic as S  # noqa: E402

TOL = 1e-4


def normalize_scale(p):
    p = p - p.mean(0, keepdims=True)
    return (p * (0.999999 / np.abs(p).max())).astype(np.float32)


def odd_object(rng, kind):
    if kind == "few":            # 2 - 5 distinct points, repeated
        k = int(rng.choice([2, 3, 5]))
        base = rng.uniform(-1, 1, (k, 3))
        return normalize_scale(base[rng.integers(0, k, 256)])
    if kind == "line":
        t = rng.uniform(-1, 1, (256, 1))
        return normalize_scale(t * rng.uniform(-1, 1, (1, 3)))
    if kind == "dense":          # everything within every radius of everything: the 32-neighbour cap bites everywhere
        p = rng.uniform(-0.05, 0.05, (256, 3))
        p[0] = (1.0, 1.0, 1.0)   # one far point keeps the scale
        return normalize_scale(p)
    if kind == "sparse":         # far-apart points: most balls hold their centre only
        p = rng.uniform(-1, 1, (256, 3))
        return normalize_scale(np.sign(p) * np.abs(p) ** 0.2)
    raise ValueError(kind)


def make_case(seed):
    rng = np.random.default_rng(seed)
    n_cells = int(rng.integers(1, 14))
    sizes = [int(rng.choice([1, 2, int(rng.integers(3, 12)), int(rng.integers(12, 40)), int(rng.integers(60, 150))],
                            p=[0.15, 0.1, 0.45, 0.25, 0.05])) for _ in range(n_cells)]
    n = sum(sizes)
    xyz, rgb, center, mean_rgb = (a.copy() for a in S.make_objects(1000 + seed, 0, n))
    for o in range(n):
        r = rng.random()
        if r < 0.25:
            xyz[o] = odd_object(rng, str(rng.choice(["few", "line", "dense", "sparse"])))
            if rng.random() < 0.5:   # repeated points keep their colours too (T.FixedPoints draws whole points)
                _, first = np.unique(xyz[o], axis=0, return_index=True)
                for i in range(256):
                    j = first[np.flatnonzero((xyz[o][first] == xyz[o][i]).all(1))[0]]
                    rgb[o][i] = rgb[o][j]
            mean_rgb[o] = rgb[o].mean(0)
    ptr = np.zeros(n_cells + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(sizes)
    return xyz, rgb, center, mean_rgb, ptr


def main():
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    classes, colors, words = S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words()
    om = OM.OracleCellRetrieval(classes, colors, words, OM.default_args()).eval()
    W.fill_state_dict(om, 11)
    models = {}
    for prec in ("f16x3", "fp32"):
        m = t2p.CellRetrievalNetwork(classes, colors, words, S.default_args(), precision=prec)
        m.load_state_dict(om.state_dict(), strict=True)
        models[prec] = m.to(dev).eval()
    om64 = KG.float64_oracle(om)
    worst, worst_viol, n_flips = 0.0, -np.inf, 0
    for seed in range(seed0, seed0 + trials):
        xyz, rgb, center, mean_rgb, ptr = make_case(seed)
        tr = []
        want = om.encode_objects_packed(xyz, rgb, center, mean_rgb, ptr, trace=tr).numpy()
        pn = [d for d in tr if "sa" in d]
        emb = [d for d in tr if "object_embeddings" in d][0]["object_embeddings"].numpy()
        want_knn = KG.oracle_knn(emb, ptr)
        dargs = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz, rgb, center, mean_rgb)]
        for prec, m in models.items():
            for chunk in (0, max(int(np.diff(ptr).max()), 37)):   # one chunk / many small chunks of whole cells
                with torch.no_grad():
                    got, gtr = m.encode_objects_packed(*dargs, ptr, want_trace=True, chunk_objects=chunk)
                tag = f"seed {seed} {prec} chunk {chunk} sizes {np.diff(ptr).tolist()}"
                for l, (nc, c) in enumerate(((128, 64), (64, 128), (32, 256))):
                    # oracle FPS indices are positions inside the cell's batch of n x (2 nc) dense points
                    w_idx = np.concatenate([(d["sa"][l]["fps"].numpy().reshape(-1, nc)
                                             - 2 * nc * np.arange(d["sa"][l]["fps"].numel() // nc)[:, None]) for d in pn])
                    assert (gtr["fps_idx"][l].cpu().numpy() == w_idx).all(), tag + f" FPS level {l + 1}"
                    w_sa = torch.cat([d["sa"][l]["out"] for d in pn]).numpy()
                    d_sa = np.abs(gtr["sa_out"][l].cpu().numpy()[:, :c] - w_sa).max()
                    assert d_sa < TOL, tag + f" SA{l + 1} {d_sa:.2e}"
                d_emb = np.abs(gtr["obj_emb"].cpu().numpy() - emb).max()
                assert d_emb < TOL, tag + f" object embeddings {d_emb:.2e}"
                got_knn = KG.global_knn(gtr["knn_idx"].cpu().numpy(), ptr, chunk)
                viol = KG.knn_violation(got_knn, KG.normalized64(gtr["obj_emb"]), ptr)
                assert viol <= 0, tag + f" kNN lists: a chosen neighbour farther than an unchosen one by {viol:.2e}"
                flips, resolved, gap = KG.check_cells(got.cpu().numpy(), got_knn, want, want_knn, emb, ptr, om64, tag)
                assert len(flips) <= 1, tag + f" {len(flips)} cells with a kNN near-tie flip"
                if len(flips):
                    print(f"  {tag}: cell {flips.tolist()} with a proven kNN near-tie flip (distance gap {gap:.1e}), "
                          f"{resolved:.2e} from the float64 oracle on the kernel's graph")
                same = np.ones(len(ptr) - 1, dtype=bool)
                same[flips] = False
                d_out = np.abs(got.cpu().numpy() - want).max(axis=1)
                worst = max(worst, float(d_emb), float(d_out[same].max(initial=0.0)), resolved)
                worst_viol, n_flips = max(worst_viol, viol), n_flips + len(flips)
        print(f"seed {seed}: {len(ptr) - 1} cells, {xyz.shape[0]} objects (sizes {np.diff(ptr).tolist()}): ok")
    print(f"fuzz ok: {trials} cases, worst difference {worst:.2e} (proven near-tie flips: {n_flips}, resolved on the kernel's "
          f"graph), worst knn_violation {worst_viol:.2e}")


if __name__ == "__main__":
    main()
