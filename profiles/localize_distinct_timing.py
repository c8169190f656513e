"""What distinct candidates cost (docs/notebook.md, "Distinct candidates"), on the scene of profiles/localize_timing.py - bench.py's
`pipeline` block: 2,048 cells, 1,024 six-hint queries, top-10, pad_size 16, a six-layer fine model at D = 128.

  Localizer.localize(hints, 10)                              the plain call, the comparison of every pair
  Localizer.localize(hints, 10, distinct_radius=cell size)   the default pool min(Nc, 1024, max(64, 32 k)) = 320 ranked cells per query

in interleaved pairs after a warm-up of both (--pairs, at least 15): the median and spread of each, of their difference, the
per-kernel split of one pass of each (t2p_profile_report: `topk_distinct` is the selection, `sim_scores` / `topk_select` the
ranking of the pool), and what the selection did to the answers: n_valid, exhausted, and how many distinct places (by the
conflict relation at the same radius) the plain top-10 of a query holds.

Two layouts of the same cells (same embeddings, same object tokens; only the corners move, so the ranking is the same):
  stride 30   the scene as bench.py lays it out: disjoint 30 m squares, 64 to a row - no two cells conflict at 30 m
  stride 10   the corners on a 10 m stride (the 30-10 layout of the dataset): a cell conflicts with up to 24 neighbours

    python profiles/localize_distinct_timing.py [--pairs 15] [--out profiles/localize_distinct_timing.json]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from text2pos_amd import evaluation as E, localize as LZ, pipeline as PL, retrieval as RT  # noqa: E402
from localize_timing import N_CELLS, N_POSES, PAD, TOP_K, kernels_ms, make_models, make_scene, summary, timed, write  # noqa: E402


def places(rows, centers, sep):
    """Distinct places among each query's candidates: the greedy count by the conflict relation (one scene, so no groups)."""
    out = []
    for r in rows:
        kept = []
        for c in r[r >= 0]:
            if not any(abs(centers[c, 0] - centers[a, 0]) < sep and abs(centers[c, 1] - centers[a, 1]) < sep for a in kept):
                kept.append(c)
        out.append(len(kept))
    return np.array(out)


def pairs(loc, hints, n_pairs, sep):
    plain = lambda: loc.localize(hints, top_k=TOP_K)
    distinct = lambda: loc.localize(hints, top_k=TOP_K, distinct_radius=sep)
    free, held = timed(plain)[0], timed(distinct)[0]                     # warm-up of both: the tables, the kernels' code objects
    walls, events = dict(plain=[], distinct=[]), dict(plain=[], distinct=[])
    for i in range(n_pairs):
        for name, fn in ((("plain", plain), ("distinct", distinct)) if i % 2 == 0 else (("distinct", distinct), ("plain", plain))):
            _, w, e = timed(fn)
            walls[name].append(w)
            events[name].append(e)
    diff = [b - a for a, b in zip(walls["plain"], walls["distinct"])]
    centers = loc.database.cell_centers().cpu().numpy()
    n_plain, n_held = places(free.cell_rows, centers, sep), places(held.cell_rows, centers, sep)
    assert np.array_equal(n_held, held.n_valid)                          # the selected candidates are pairwise distinct
    k_plain, k_held = kernels_ms(plain), kernels_ms(distinct)
    rank = lambda k: round(sum(v["total_ms"] for n, v in k.items() if n in ("sim_scores", "topk_select", "sim_partial", "topk_merge")), 4)
    return dict(distinct_radius_m=sep, pool=RT.default_distinct_pool(len(loc.database), TOP_K), pairs=n_pairs,
                localize_wall_s=summary(walls["plain"]), localize_distinct_wall_s=summary(walls["distinct"]),
                localize_event_s=summary(events["plain"]), localize_distinct_event_s=summary(events["distinct"]),
                distinct_minus_plain_wall_s=summary(diff), plain_spread_s=round(max(walls["plain"]) - min(walls["plain"]), 5),
                distinct_spread_s=round(max(walls["distinct"]) - min(walls["distinct"]), 5),
                ratio_of_medians=round(statistics.median(walls["distinct"]) / statistics.median(walls["plain"]), 4),
                places_in_plain_top_k=dict(mean=float(n_plain.mean()), min=int(n_plain.min()), max=int(n_plain.max())),
                n_valid=dict(mean=float(held.n_valid.mean()), min=int(held.n_valid.min())), exhausted_queries=int(held.exhausted.sum()),
                same_candidates_as_plain=float(np.mean((held.cell_rows == free.cell_rows).all(axis=1))),
                selection_ms=k_held.get("topk_distinct", dict(total_ms=0.0))["total_ms"],
                ranking_ms=dict(plain=rank(k_plain), distinct=rank(k_held)),
                localize_kernels_ms=k_plain, localize_distinct_kernels_ms=k_held)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_distinct_timing.json"))
    a = ap.parse_args()
    n_pairs = max(15, a.pairs)
    dev = torch.device("cuda:0")
    scenes = make_scene()
    tf = PL.PerCellTransform(256, 5)
    coarse, fine = make_models(dev, scenes, tf)
    hints = [E.create_hint_description(p) for p in scenes.all_poses]
    out = dict(cells=N_CELLS, poses=N_POSES, top_k=TOP_K, pad_size=PAD, device=torch.cuda.get_device_name(0),
               fine_model="SuperGlueMatch embed_dim 128, 6 x (self, cross), 50 Sinkhorn iterations, random init")
    db = LZ.CellDatabase.build(coarse, fine, scenes.all_cells, tf, PAD)
    sep = float(db.cell_size[0])
    out["stride_30"] = pairs(LZ.Localizer(coarse, fine, db), hints, n_pairs, sep)
    i = torch.arange(N_CELLS, device=db.device)
    corners = torch.stack([10.0 * (i % 64), 10.0 * (i // 64)], dim=1).to(torch.float64)
    dense = LZ.CellDatabase(db.coarse, db.fine, db.center_xy, corners, db.cell_size, db.cell_ids, db.scene_names, db.meta)
    out["stride_10"] = pairs(LZ.Localizer(coarse, fine, dense), hints, n_pairs, sep)
    write(out, a.out)


if __name__ == "__main__":
    main()
