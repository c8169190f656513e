# Time of one retrieval call (text2pos_amd.retrieve_topk = t2p_sim_topk) over k, beside torch's float64 GEMM + topk on the same
# tensors: one JSON line per (shape, k).  Device events around `--calls` back-to-back calls, median over `--steps` such windows
# after `--warmup` of them; the per-kernel split comes from a separate profiled call (ops.profile_report), outside the timed windows.
#   python profiles/topk_sweep.py [--shapes 1000x12000,1250x100000] [--ks 10,16,17,32,100,256,1024] [--steps 9] [--warmup 3]
# --groups G adds the group-restricted call (t2p_sim_topk_grouped; cells and queries uniform over G ids) timed in windows that
# alternate with windows of the unrestricted call: `grouped_ms` and the per-pair ratios grouped / unrestricted.
# --prior RADIUS adds, in the same way, the prior-restricted call (t2p_sim_topk_prior): 30 m boxes at stride 10 on a square grid (the
# geometry of tests/topk_ref.py), seeded prior points uniform over the grid, every query's radius RADIUS: `prior_ms` and its ratios.
# --skip-torch leaves the float64 GEMM + topk yardstick out (A/B runs of two builds of the library: T2P_LIB).
# --shapes route is the grid the k <= 16 routing threshold (csrc/sim_topk.hip: kTileMinPairs) was chosen on: nq in {64, 130, 256, 1000,
# 1250} x nc in {1000, 4000, 12000, 100000}, to be run at --ks 1,10,16 once per forced path - two A/B builds of the library,
#   python text2pos-cvpr2022_amd/build.py --variant lists T2P_SIM_TILE_MIN_PAIRS=4000000000000000000
#   python text2pos-cvpr2022_amd/build.py --variant tile T2P_SIM_TILE_MIN_PAIRS=1
# each selected with T2P_LIB; profiles/t04_topk_route_sweep.md holds the table.
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import text2pos_amd as t2p  # noqa: E402
from text2pos_amd import ops  # noqa: E402


def timed(fn, steps, warmup, calls):
    """median / min / max milliseconds per call over `steps` windows of `calls` calls each"""
    ms = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ms)), min(ms), max(ms)


def timed_pairs(fn_a, fn_b, steps, warmup, calls):
    """Windows of fn_a and fn_b in alternation: (median ms of a, median ms of b, per-pair ratios b / a)."""
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls
    a_ms, b_ms = [], []
    for i in range(warmup + steps):
        ta, tb = window(fn_a), window(fn_b)
        if i >= warmup:
            a_ms.append(ta)
            b_ms.append(tb)
    return float(np.median(a_ms)), float(np.median(b_ms)), [b / a for a, b in zip(a_ms, b_ms)]


ROUTE_SHAPES = ",".join(f"{nq}x{nc}" for nq in (64, 130, 256, 1000, 1250) for nc in (1000, 4000, 12000, 100000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x12000,1250x100000")
    ap.add_argument("--ks", default="10,16,17,32,100,256,1024")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="calls per timed window (0: 20 for the small shape, 3 above 10^8 scores)")
    ap.add_argument("--groups", type=int, default=0, help="also time the group-restricted call with this many group ids")
    ap.add_argument("--prior", type=float, default=None, help="also time the prior-restricted call with this radius in metres")
    ap.add_argument("--skip-torch", action="store_true", help="do not time torch's float64 GEMM + topk")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "topk_sweep needs cuda:0: there is no CPU path to time"
    dev = torch.device("cuda:0")
    for shape in (ROUTE_SHAPES if a.shapes == "route" else a.shapes).split(","):
        nq, nc = (int(x) for x in shape.split("x"))
        g = torch.Generator().manual_seed(nq * 31 + nc)
        c = torch.nn.functional.normalize(torch.randn(nc, a.dim, generator=g), dim=-1).to(dev)
        q = torch.nn.functional.normalize(torch.randn(nq, a.dim, generator=g), dim=-1).to(dev)
        calls = a.calls or (20 if nq * nc <= 10 ** 8 else 3)
        cd, qd = c.double(), q.double()      # (the yardstick's conversion is not in its time)
        variants = {}      # name -> the restriction's arguments of retrieve_topk; each is timed in windows that alternate with the plain call
        if a.groups:
            cg = torch.randint(0, a.groups, (nc,), generator=g).to(torch.int32).to(dev)
            qg = torch.randint(0, a.groups, (nq,), generator=g).to(torch.int32).to(dev)
            variants["grouped"] = dict(cell_groups=cg, query_groups=qg)
        if a.prior is not None:
            w = math.isqrt(nc - 1) + 1
            i = torch.arange(nc, dtype=torch.float64)
            x0, y0 = 10.0 * (i % w), 10.0 * (i // w)
            xy = torch.randint(0, 10 * w + 21, (nq, 2), generator=torch.Generator().manual_seed(7000 + nq + nc)).double()
            variants["prior"] = dict(cell_boxes=torch.stack([x0, y0, x0 + 30.0, y0 + 30.0], dim=1).to(dev), query_xy=xy.to(dev),
                                     query_radius=torch.full((nq,), a.prior, dtype=torch.float64, device=dev),
                                     validate=False)      # (the value check reads three flags back: not the kernels' time)
        for k in (int(x) for x in a.ks.split(",")):
            med, lo, hi = timed(lambda: t2p.retrieve_topk(c, q, k), a.steps, a.warmup, calls)
            t_med, t_lo, t_hi = (0.0, 0.0, 0.0) if a.skip_torch else timed(lambda: (qd @ cd.T).topk(k), a.steps, a.warmup, calls)
            restricted = {}
            for name, kw in variants.items():
                u_ms, r_ms, ratios = timed_pairs(lambda: t2p.retrieve_topk(c, q, k), lambda: t2p.retrieve_topk(c, q, k, **kw),
                                                 a.steps, a.warmup, calls)
                ops.profile_report()
                ops.profile_enable(True)
                try:
                    t2p.retrieve_topk(c, q, k, **kw)
                finally:
                    ops.profile_enable(False)
                pre = "" if name == "grouped" else name + "_"      # (the grouped call's keys are the ones earlier tables were made from)
                restricted.update({"groups": a.groups, "paired_ungrouped_ms": round(u_ms, 4)} if name == "grouped" else
                                  {"prior_radius": a.prior, "paired_unrestricted_ms": round(u_ms, 4)})
                restricted.update({name + "_ms": round(r_ms, 4), pre + "ratio_median": round(float(np.median(ratios)), 4),
                                   pre + "ratio_min": round(min(ratios), 4), pre + "ratio_max": round(max(ratios), 4),
                                   name + "_kernels": {n: dict(launches=cnt, ms=round(ms, 4)) for n, (cnt, ms) in ops.profile_report().items()}})
            idx, score = t2p.retrieve_topk(c, q, k)
            want = (qd @ cd.T).topk(k)
            torch.cuda.synchronize()
            ops.profile_report()
            ops.profile_enable(True)
            try:
                t2p.retrieve_topk(c, q, k)
            finally:
                ops.profile_enable(False)
            kernels = {n: dict(launches=cnt, ms=round(ms, 4)) for n, (cnt, ms) in ops.profile_report().items()}
            print(json.dumps(dict(nq=nq, nc=nc, dim=a.dim, k=k, calls_per_window=calls, steps=a.steps,
                                  ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                                  torch_f64_gemm_topk_ms=round(t_med, 4), torch_min=round(t_lo, 4), torch_max=round(t_hi, 4),
                                  kernels=kernels, workspace_bytes=int(ops.L.lib().t2p_sim_topk_workspace_bytes(nq, nc, k)),
                                  max_score_diff_vs_torch=float((score - want.values).abs().max()), **restricted)), flush=True)
        del c, q, cd, qd


if __name__ == "__main__":
    main()
