#!/usr/bin/env python3
"""Times the KITTI evaluation protocol (mcav_eval_depth: crop, exact per-image median scaling, metrics) on one KITTI-sized batch and prints
one JSON line.  Workload: B = 12 ground-truth maps padded to 375 x 1242 with mixed true sizes, 30 % density, 192 x 640 disparities, Garg
crop, median scaling.
usage: python tools/eval_bench.py [--batch 12] [--iters 200] [--no-median]
  us_per_batch      back-to-back calls of the C entry with prebuilt arguments (events around the loop)
  us_graph          the same call captured once and replayed
  us_per_launch     each launch's own duration (per-dispatch events, csrc/kernel_timer.h), median over 50 calls, in launch order
  bytes / hbm_frac  algorithmic bytes (gt read twice inside the crop boxes, disparity read twice, 8 B of keys written and read three times
                    per masked pixel) and their rate as a fraction of 8 TB/s at us_per_batch
  numpy_us          tests/eval_protocol_ref.py (numpy / torch-CPU) on the same input"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_protocol_ref as R  # noqa: E402
import evaluate as E  # noqa: E402
from mcav import lib as L  # noqa: E402
from mcav import nn as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--no-median", action="store_true")
a = ap.parse_args()
dev = "cuda"
B, Hg, Wg, h, w = a.batch, 375, 1242, 192, 640
sizes = [[(375, 1242), (370, 1226), (374, 1238), (370, 1224)][b % 4] for b in range(B)]
rng = np.random.RandomState(0)
gt = np.zeros((B, Hg, Wg), np.float32)
for b, (H, W) in enumerate(sizes):
    g = (np.round(rng.uniform(1.0, 85.0, (H, W)) * 256) / 256).astype(np.float32)
    g[rng.rand(H, W) > 0.3] = 0
    gt[b, :H, :W] = g
z = torch.nn.functional.interpolate(torch.from_numpy(rng.randn(B, 1, h // 8, w // 8).astype(np.float32)), size=(h, w), mode="bilinear",
                                    align_corners=False)
disp = (0.02 + 0.3 * torch.sigmoid(z))[:, 0].numpy()            # smooth, as a depth network gives them

gt_d, disp_d = torch.from_numpy(gt).to(dev), torch.from_numpy(disp).to(dev)
boxes = [E.crop_box(H, W, "garg") for H, W in sizes]
meta = torch.tensor([v for s in sizes for v in s] + [v for bx in boxes for v in bx], dtype=torch.int32, device=dev)
lib = L.lib()
ws = torch.empty(lib.mcav_eval_depth_workspace_bytes(B, Hg, Wg), dtype=torch.uint8, device=dev)
rows = torch.empty((B, 11), device=dev)
flags = 0 if a.no_median else E.EVAL_MEDIAN_SCALING


def call():
    L.check(lib.mcav_eval_depth(L.ptr(gt_d), L.ptr(disp_d), B, Hg, Wg, h, w, L.ptr(meta), L.c_p(meta.data_ptr() + 8 * B), 1e-3, 80.0, 1.0,
                                flags, L.ptr(rows), L.ptr(ws), ws.numel(), L.stream()), "mcav_eval_depth")


for _ in range(20):
    call()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.iters):
    call()
e1.record()
torch.cuda.synchronize()
us = 1000.0 * e0.elapsed_time(e1) / a.iters

s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    call()
torch.cuda.current_stream().wait_stream(s)
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    call()
for _ in range(10):
    graph.replay()
torch.cuda.synchronize()
e0.record()
for _ in range(a.iters):
    graph.replay()
e1.record()
torch.cuda.synchronize()
us_graph = 1000.0 * e0.elapsed_time(e1) / a.iters

N.kernel_timer_begin()
for _ in range(50):
    call()
torch.cuda.synchronize()
d = N.kernel_timer_end()
nl = len(d) // 50
per_launch = [round(1000.0 * sorted(d[k::nl])[25], 2) for k in range(nl)]
names = (["init", "gather"] + ["hist%d" % p if k == 0 else "select%d" % p for p in range(3) for k in range(2)] if flags else []) + ["metrics",
                                                                                                                                    "finalize"]
r = rows.cpu().numpy()
masked = float(r[:, 9].sum())
box_px = sum((bx[1] - bx[0]) * (bx[3] - bx[2]) for bx in boxes)
nbytes = 2 * 4 * box_px + 2 * 4 * B * h * w + (32 * masked if flags else 0)
t0 = time.perf_counter()
want, want_rows = R.evaluate(gt, disp, sizes, "garg", median_scaling=not a.no_median)
numpy_us = 1e6 * (time.perf_counter() - t0)
assert np.array_equal(r[:, 9], want_rows[:, 9]) and np.allclose(r[:, 10], want_rows[:, 10], rtol=2e-6)
print(json.dumps({"workload": "eval_depth B=%d padded %dx%d disp %dx%d garg%s" % (B, Hg, Wg, h, w, "" if a.no_median else " median"),
                  "us_per_batch": round(us, 2), "us_graph": round(us_graph, 2), "launches": nl,
                  "us_per_launch": dict(zip(names, per_launch)), "masked_pixels": int(masked), "bytes": int(nbytes),
                  "hbm_frac": round(nbytes / (us * 1e-6) / 8e12, 4), "numpy_us": round(numpy_us, 1),
                  "abs_rel": float(E.reduce_rows(rows)["abs_rel"])}))
