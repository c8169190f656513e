"""The serving path against the evaluation's coarse + fine stages (docs/notebook.md, "Localizer"), on the synthetic scene of bench.py's
`pipeline` block: 2,048 cells of raw float64 points, 1,024 six-hint poses, top-10, pad_size 16, a six-layer fine model at D = 128.

  (a) localize.CellDatabase.build         paid once: upload, both encoders over the 2,048 cells
  (b) localize.Localizer.localize         the 1,024 queries from the built database
  (c) pipeline.evaluate (--pairs N)       timings["coarse_s"] + timings["fine_s"] of the evaluation with the on-device input side, which
                                          encodes the 2,048 cells and 163,840 objects again; run in interleaved pairs with (b)

  (d) localize with a prior (--prior_pairs N)  (b) beside the same call restricted to the cells within 60 m of each pose's own position
                                          (t2p_sim_topk_prior: the mask is an epilogue of the same product loop), in interleaved pairs;
                                          written to its own file

hipEvent and wall-clock times after a warm-up pass, the median of --repeats (>= 5) passes, the per-kernel breakdown of one localize
pass (t2p_profile_report), written as JSON.

    python profiles/localize_timing.py [--repeats 7] [--pairs 3] [--out profiles/localize_timing.json]
    python profiles/localize_timing.py --prior_pairs 15 [--prior_radius 60] [--prior_out profiles/localize_prior_timing.json]
                                          # (d) alone: one build, no evaluation"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import text2pos_amd as t2p  # noqa: E402
from text2pos_amd import data as D, evaluation as E, io as IO, localize as LZ, ops, pipeline as PL, synthetic as S  # noqa: E402

SEED = 20220002 + 5      # the scene of bench.py::pipeline_rates
N_CELLS, N_POSES, TOP_K, PAD = 2048, 1024, 10, 16


def make_scene():
    rng = np.random.default_rng(SEED)
    dirs = ["north", "south", "east", "west", "on-top"]
    cells, poses = [], []
    for i in range(N_CELLS):
        objs = []
        for j in range(int(rng.integers(6, 20))):
            c = rng.random(3) * np.array([1.0, 1.0, 0.3])
            n = int(rng.integers(30, 400))
            col = np.clip(rng.random(3), 0, 1)
            objs.append(D.Object3d(j, 1000 * i + j, c + 0.05 * rng.standard_normal((n, 3)),
                                   np.clip(col + 0.05 * rng.standard_normal((n, 3)), 0, 1), S.LABELS[int(rng.integers(0, len(S.LABELS)))]))
        x, y = 30.0 * (i % 64), 30.0 * (i // 64)
        cells.append(D.Cell(i, "syn1", objs, 30.0, np.array([x, y, 0.0, x + 30.0, y + 30.0, 10.0])))
    for q in range(N_POSES):
        c = cells[int(rng.integers(0, N_CELLS))]
        descs = [D.DescriptionBestCell(dirs[int(rng.integers(0, 5))], o.get_color_text(), o.label, o.id, True)
                 for o in [c.objects[int(k)] for k in rng.choice(len(c.objects), 6, replace=False)]]
        poses.append(D.Pose(rng.random(3), c.bbox_w[0:3] + rng.random(3) * 30.0, c.id, "syn1", descs))
    return IO.Scenes(cells, poses)


def make_models(dev, scenes, tf):
    """bench.py's models: random-init coarse model whose BatchNorm statistics come from one train-mode pass over 64 cells, random-init
    fine model of six layer pairs."""
    from text2pos_amd.scene import DeviceScene
    torch.manual_seed(1234)
    coarse = t2p.CellRetrievalNetwork(S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words(), S.default_args()).to(dev)
    bns = [m for m in coarse.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    for m in bns:
        m.reset_running_stats()
        m.momentum = None
    coarse.train()
    block = DeviceScene(scenes.all_cells[:64], dev)
    with torch.no_grad():
        packed, cp, _ = block.pack_cells(tf, 0, 64)
        coarse.encode_objects_packed(*packed, cp)
    coarse.eval()
    for m in bns:
        m.momentum = 0.1
    torch.manual_seed(4321)
    fine = t2p.SuperGlueMatch(S.LABELS + ["pad"], S.COLOR_NAMES, S.known_words(), PL._model_args(128, num_layers=6, sinkhorn_iters=50))
    return coarse, fine.to(dev).eval()


def timed(fn):
    """(result, wall seconds, hipEvent seconds) of fn() on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, a.elapsed_time(b) / 1e3


def summary(xs):
    return dict(series=[round(x, 5) for x in xs], median=round(statistics.median(xs), 5), min=round(min(xs), 5), max=round(max(xs), 5))


def kernels_ms(run):
    """Per-kernel split of one pass of run() (t2p_profile_report), largest first."""
    ops.profile_enable(True)
    ops.profile_report()
    run()
    rep = ops.profile_report()
    ops.profile_enable(False)
    return {k: dict(launches=v[0], total_ms=round(v[1], 4)) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1])}


def prior_pairs(loc, scenes, hints, n_pairs, radius, base):
    """(d): interleaved (unrestricted, restricted) pairs of Localizer.localize; the prior of a query is its pose's own position."""
    xy = np.array([np.asarray(p.pose_w, dtype=np.float64)[0:2] for p in scenes.all_poses])
    plain = lambda: loc.localize(hints, top_k=TOP_K)
    prior = lambda: loc.localize(hints, top_k=TOP_K, prior_xy=xy, prior_radius=radius)
    free, held = timed(plain)[0], timed(prior)[0]                        # warm-up of both: the prior's tables, its kernels' code objects
    walls = dict(plain=[], prior=[])
    events = dict(plain=[], prior=[])
    for i in range(n_pairs):
        for name, fn in ((("plain", plain), ("prior", prior)) if i % 2 == 0 else (("prior", prior), ("plain", plain))):
            _, w, e = timed(fn)
            walls[name].append(w)
            events[name].append(e)
    diff = [b - a for a, b in zip(walls["plain"], walls["prior"])]
    # what the restriction did to the answers: candidates that qualified, and how often the true cell is among them
    truth = [p.cell_id for p in scenes.all_poses]
    hit = lambda r: float(np.mean([t in ids for t, ids in zip(truth, r.cell_ids)]))
    return dict(base, prior_radius_m=radius, pairs=n_pairs,
                localize_wall_s=summary(walls["plain"]), localize_prior_wall_s=summary(walls["prior"]),
                localize_event_s=summary(events["plain"]), localize_prior_event_s=summary(events["prior"]),
                prior_minus_plain_wall_s=summary(diff), plain_spread_s=round(max(walls["plain"]) - min(walls["plain"]), 5),
                prior_spread_s=round(max(walls["prior"]) - min(walls["prior"]), 5),
                n_valid_mean=float(held.n_valid.mean()), n_valid_min=int(held.n_valid.min()),
                true_cell_in_top_k=dict(plain=hit(free), prior=hit(held)),
                localize_kernels_ms=kernels_ms(plain), localize_prior_kernels_ms=kernels_ms(prior))


def write(out, path):
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=3, help="interleaved (evaluate, localize) pairs; 0 = skip the evaluation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_timing.json"))
    ap.add_argument("--prior_pairs", type=int, default=0, help="(d) alone: interleaved (localize, localize with a prior) pairs")
    ap.add_argument("--prior_radius", type=float, default=60.0, help="radius of (d)'s prior around each pose's own position, metres")
    ap.add_argument("--prior_out", default=os.path.join(ROOT, "profiles", "localize_prior_timing.json"))
    a = ap.parse_args()
    repeats = max(5, a.repeats)
    dev = torch.device("cuda:0")
    scenes = make_scene()
    tf = PL.PerCellTransform(256, 5)
    coarse, fine = make_models(dev, scenes, tf)
    hints = [E.create_hint_description(p) for p in scenes.all_poses]
    out = dict(cells=N_CELLS, poses=N_POSES, top_k=TOP_K, pad_size=PAD, device=torch.cuda.get_device_name(0),
               objects=int(sum(len(c.objects) for c in scenes.all_cells)),
               fine_model="SuperGlueMatch embed_dim 128, 6 x (self, cross), 50 Sinkhorn iterations, random init")

    build = lambda: LZ.CellDatabase.build(coarse, fine, scenes.all_cells, tf, PAD)
    db, _, _ = timed(build)                                             # warm-up: the allocator's first workspaces
    if a.prior_pairs > 0:
        write(prior_pairs(LZ.Localizer(coarse, fine, db), scenes, hints, max(5, a.prior_pairs), a.prior_radius, out), a.prior_out)
        return
    walls, events = [], []
    for _ in range(repeats):
        db, w, e = timed(build)
        walls.append(w)
        events.append(e)
    out["build"] = dict(wall_s=summary(walls), event_s=summary(events))

    loc = LZ.Localizer(coarse, fine, db)
    run = lambda: loc.localize(hints, top_k=TOP_K)
    res, _, _ = timed(run)
    walls, events = [], []
    for _ in range(repeats):
        res, w, e = timed(run)
        walls.append(w)
        events.append(e)
    out["localize"] = dict(wall_s=summary(walls), event_s=summary(events), queries_per_s=round(N_POSES / statistics.median(walls), 1),
                           matched_mean=float(res.matched.mean()))

    out["localize_kernels_ms"] = kernels_ms(run)

    if a.pairs > 0:
        pairs = max(3, a.pairs)
        ev_s, loc_s, parts = [], [], []
        PL.evaluate(coarse, fine, scenes, tf, (1, 5, TOP_K), (5, 10, 15), PAD, timings={})     # warm-up
        for _ in range(pairs):
            tm = {}
            torch.cuda.synchronize()
            PL.evaluate(coarse, fine, scenes, tf, (1, 5, TOP_K), (5, 10, 15), PAD, timings=tm)
            torch.cuda.synchronize()
            ev_s.append(tm["coarse_s"] + tm["fine_s"])
            parts.append({k: round(v, 5) for k, v in tm.items()})
            loc_s.append(timed(run)[1])
        out["pairs"] = dict(evaluate_coarse_plus_fine_s=summary(ev_s), evaluate_parts=parts, localize_wall_s=summary(loc_s),
                            evaluate_spread_s=round(max(ev_s) - min(ev_s), 5),
                            ratio_of_medians=round(statistics.median(ev_s) / statistics.median(loc_s), 3))
    write(out, a.out)


if __name__ == "__main__":
    main()
