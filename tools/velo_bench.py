#!/usr/bin/env python3
"""Times the Velodyne -> sparse depth map projection (mcav_velo_depth_map: KITTI Eigen ground truth) on one KITTI-sized batch and prints one
JSON line.  Workload: B = 12 seeded KITTI-like scans of 120 k points (tests/velo_ref.py scan: uniform azimuth, elevation -0.43..0.035 rad,
range 1-90 m), alternating 375 x 1242 (2011_09_26 P_rect_02) and 370 x 1226 (2011_09_28), padded to 375 x 1242.
usage: python tools/velo_bench.py [--batch 12] [--points 120000] [--iters 100]
  us_per_batch      median over --iters back-to-back calls of the C entry with prebuilt arguments (an event pair around each call, no
                    synchronisation in between), after 20 warm-up calls; us_loop_mean: the whole loop / iters
  us_per_launch     each launch's own duration (per-dispatch events, csrc/kernel_timer.h), median over 50 calls, in launch order
  bytes / byte_bound_frac   algorithmic bytes (16 B per point read; per padded pixel 4 B written by init, 4 B read and 4 B written by
                    finalize; the ~8 B of each landing point's atomic are left out) and that over the 8 TB/s HBM peak at us_per_batch: the
                    fraction of a byte bound
  numpy_restated_ms / monodepth2_ms   tests/velo_ref.py restated() and its monodepth2 transcription, per scan, on one host core"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import velo_ref as V  # noqa: E402
import geometry.velodyne  # noqa: E402,F401  (registers the signature)
from mcav import lib as L  # noqa: E402
from mcav import nn as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--host-scans", type=int, default=2, help="scans timed on the host (numpy)")
a = ap.parse_args()
dev = "cuda"
B, Hg, Wg = a.batch, 375, 1242
dates = [("2011_09_26", "2011_09_28")[b % 2] for b in range(B)]
scans = [V.scan(1000 + b, a.points) for b in range(B)]
Ps = [V.kitti_P(d) for d in dates]
sizes = [V.KITTI_SIZES[d] for d in dates]
offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
pts = torch.from_numpy(np.concatenate(scans)).to(dev)
offs = torch.from_numpy(offsets).to(dev)
P = torch.from_numpy(np.stack(Ps).reshape(B, 12)).to(dev)
sz = torch.tensor(sizes, dtype=torch.int32, device=dev)
out = torch.empty((B, Hg, Wg), device=dev)
lib = L.lib()


def call():
    L.check(lib.mcav_velo_depth_map(L.ptr(pts), L.ptr(offs), L.ptr(P), L.ptr(sz), L.c_p(0), B, Hg, Wg, a.points, 0, L.ptr(out), L.stream()),
            "mcav_velo_depth_map")


for _ in range(20):
    call()
torch.cuda.synchronize()
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
t0 = time.perf_counter()
for e0, e1 in ev:
    e0.record()
    call()
    e1.record()
torch.cuda.synchronize()
loop_us = 1e6 * (time.perf_counter() - t0) / a.iters
per_call = sorted(1000.0 * e0.elapsed_time(e1) for e0, e1 in ev)
us = per_call[len(per_call) // 2]

N.kernel_timer_begin()
for _ in range(50):
    call()
torch.cuda.synchronize()
d = N.kernel_timer_end()
nl = len(d) // 50
per_launch = [round(1000.0 * sorted(d[k::nl])[25], 2) for k in range(nl)]

got = out.cpu().numpy()
want = V.restated_batch(Ps, scans, sizes, Hg, Wg)
assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the map differs from the restatement"
landed = int((got > 0).sum())
nbytes = 16 * B * a.points + 12 * B * Hg * Wg

hs = min(a.host_scans, B)
try:                                                   # one host core: BLAS (monodepth2's np.dot) limited to one thread
    from threadpoolctl import threadpool_limits
    limit = threadpool_limits(1)
except ImportError:
    limit = None
t0 = time.perf_counter()
for b in range(hs):
    V.restated(Ps[b], scans[b], sizes[b])
np_ms = 1e3 * (time.perf_counter() - t0) / hs
t0 = time.perf_counter()
for b in range(hs):
    V.monodepth2(Ps[b], scans[b], sizes[b])
m2_ms = 1e3 * (time.perf_counter() - t0) / hs
print(json.dumps({"workload": "velo_depth_map B=%d x %d points padded %dx%d" % (B, a.points, Hg, Wg),
                  "us_per_batch": round(us, 2), "us_min": round(per_call[0], 2), "us_loop_mean": round(loop_us, 2), "launches": nl,
                  "us_per_launch": dict(zip(["init", "scatter", "finalize"], per_launch)), "nonzero_pixels": landed,
                  "bytes": int(nbytes), "byte_bound_frac": round(nbytes / (us * 1e-6) / 8e12, 4),
                  "numpy_restated_ms_per_scan": round(np_ms, 2), "monodepth2_ms_per_scan": round(m2_ms, 2),
                  "host_one_thread": limit is not None}))
