"""A fine training step on the host-twin feed and on the device feed of training.SceneFineFeed (docs/notebook.md, "Fine training feed
from a resident scene"): wall time per step of train_fine_epoch at B = 32, 16 objects, 6 hints, 256 points, D = 128, six layer pairs on a
raw scene of 512 cells, interleaved pairs; the share of it spent building the batch; and t2p_fine_step_stats (events around 200
back-to-back launches through the wrapper, the kernel alone by the library's own per-launch events) next to fine_batch_stats on the host.

    python profiles/fine_feed_timing.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else None
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import text2pos_amd as t2p  # noqa: E402
from text2pos_amd import io as IO, ops, synthetic as S, training as T  # noqa: E402
from text2pos_amd.pipeline import _model_args  # noqa: E402
from text2pos_amd.scene import DeviceScene  # noqa: E402
from fine_scene import make_fine_scene  # noqa: E402

dev = torch.device("cuda:0")
B, PAD, HINTS, N_PTS = 32, 16, 6, 256
out = {}
t0 = time.perf_counter()
cells, poses = make_fine_scene(512, 2048, 7, PAD, HINTS, lo_pts=30, hi_pts=1000)
scenes = IO.Scenes(cells, poses)
sc = DeviceScene(cells, dev, n_pad=PAD, pad_seed=0)
out["scene"] = dict(cells=len(cells), poses=len(poses), objects=sc.n_objects, raw_points=int(sc.rows.sum()), build_s=time.perf_counter() - t0)
kw = dict(n_pts=N_PTS, seed=0, batch_size=B, pad_size=PAD, num_mentioned=HINTS, rotate_degrees=120.0, shuffle=True)
t0 = time.perf_counter()
feed_d = T.SceneFineFeed(scenes, sc, **kw)
out["feed_build_s"] = time.perf_counter() - t0
feed_h = T.SceneFineFeed(scenes, sc, host=True, **kw)


def model():
    torch.manual_seed(0)
    m = t2p.SuperGlueMatch(S.LABELS + ["pad"], S.COLOR_NAMES, [str(w) for w in scenes.get_known_words()], _model_args(128, 6, 50))
    return m.to(dev)


runs = {}
for name, feed in (("device", feed_d), ("host", feed_h)):
    m = model()
    runs[name] = dict(feed=feed, model=m, opt=torch.optim.Adam(m.parameters(), lr=1e-5), build=[], step=[], skipped=0)
order = feed_d.epoch_order(0)
WARM, PAIRS = 3, 20
for i in range(WARM + PAIRS):
    idx = order[i * B: (i + 1) * B]
    for name in (("device", "host") if i % 2 == 0 else ("host", "device")):
        r = runs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = r["feed"].batch(idx, 0)
        t1 = time.perf_counter()
        stats = T.train_fine_epoch(r["model"], [batch], r["opt"], scene=sc)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= WARM:
            r["build"].append((t1 - t0) * 1e3)
            r["step"].append((t2 - t0) * 1e3)
            r["skipped"] += stats["skipped_steps"]
for name, r in runs.items():
    out[name] = dict(step_ms_median=float(np.median(r["step"])), step_ms_min=float(np.min(r["step"])), step_ms_max=float(np.max(r["step"])),
                     build_ms_median=float(np.median(r["build"])), build_ms_min=float(np.min(r["build"])), skipped=r["skipped"],
                     steps=[round(v, 3) for v in r["step"]])
out["pair_ratio_median"] = float(np.median(np.array(runs["host"]["step"]) / np.array(runs["device"]["step"])))

# the statistics alone: the kernel's launch (events around 200 launches) and fine_batch_stats on the host for the same batch
m = runs["host"]["model"]
bh, bd = feed_h.batch(order[:B], 0), feed_d.batch(order[:B], 0)
with torch.no_grad():
    o = m(bh["objects"], bh["hint_descriptions"], bh["object_points"])
ft = bd["fine_targets"]


def kernel_us(m0, m1, off, pi, gt, pxy, cxy, reps=200):
    for _ in range(10):
        ops.fine_step_stats(m0, m1, off, pi, gt, pxy, cxy, check=False)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        ops.fine_step_stats(m0, m1, off, pi, gt, pxy, cxy, check=False)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def host_ms(fn, reps=20):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


out["stats_32_16_6"] = dict(kernel_us_back_to_back=kernel_us(o.matches0, o.matches1, o.offsets.contiguous(), ft["pose_idx"], ft["gt_hint"],
                                                             ft["pose_xy"], ft["slot_center_xy"]),
                            host_fine_batch_stats_ms=host_ms(lambda: T.fine_batch_stats(bh, o)))
import test_gpu_fine_stats as K  # noqa: E402
c = K._case(2, 63, 63)
t = K._upload(c)
out["stats_2_63_63"] = dict(kernel_us_back_to_back=kernel_us(t["m0"], t["m1"], t["off"], t["pose_idx"], t["gt"], t["pose_xy"], t["centre"]),
                            host_calc_functions_ms=host_ms(lambda: K._reference(c)))
# one launch + the 56-byte copy, as the loop pays it
t0 = time.perf_counter()
for _ in range(100):
    ops.fine_step_row(ops.fine_step_stats(o.matches0, o.matches1, o.offsets.contiguous(), ft["pose_idx"], ft["gt_hint"], ft["pose_xy"],
                                          ft["slot_center_xy"], check=False)[1])
out["stats_32_16_6"]["launch_plus_copy_us"] = (time.perf_counter() - t0) * 1e4
# the kernel alone: the library's own events around each launch
ops.profile_enable(True)
ops.profile_report()
for _ in range(50):
    ops.fine_step_stats(o.matches0, o.matches1, o.offsets.contiguous(), ft["pose_idx"], ft["gt_hint"], ft["pose_xy"], ft["slot_center_xy"], check=False)
n, ms = ops.profile_report()["fine_step_stats"]
out["stats_32_16_6"]["kernel_us_events"] = ms * 1e3 / n
for _ in range(50):
    ops.fine_step_stats(t["m0"], t["m1"], t["off"], t["pose_idx"], t["gt"], t["pose_xy"], t["centre"], check=False)
n, ms = ops.profile_report()["fine_step_stats"]
out["stats_2_63_63"]["kernel_us_events"] = ms * 1e3 / n
ops.profile_enable(False)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
