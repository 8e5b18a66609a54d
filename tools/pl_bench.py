#!/usr/bin/env python3
"""Times a batch of network disparities -> pseudo-LiDAR clouds and prints one JSON line.  Workload: B = 12 maps of 192 x 640 (a seeded
KITTI-like scene: tests/pl_batch_cases.py) -> clouds at 375 x 1242 with KITTI's P_rect_02 and velodyne -> camera transform.
usage: python tools/pl_bench.py [--batch 12] [--iters 50] [--rounds 3]
  a_dense     PseudoLiDAR.project_batch (mcav_pl_batch_project, dense) + CloudBatch.counts(): one read-back per batch
  b_beams     the same with beam_tables() (64 x 512 cells per image)
  c_project_PL   what the tree offered before: depth = 1 / (10 disp + 0.01) and F.interpolate to 375 x 1242 with stock torch, then twelve
              project_PL calls (float64 rows, one read-back each)
Each is the host time of --iters batches ending in a device synchronise, per batch, after 5 warm-up batches; the three are alternated
--rounds times and every round is listed (us), with the median.  a_dense_kernels_us / b_beams_kernels_us: an event pair around the C
entry alone (no read-back), median.
bytes: the algorithmic traffic -- 4 B read per network pixel and 16 B written per point; beams add 8 B per cell (the cell words; the
memset, the atomics and the second read of the cells are left out); c: 4 B read and 4 B written per network pixel by the conversion, 4 B
read per network pixel and 4 B written per output pixel by the resize, 4 B read per output pixel and 32 B written per point by project_PL.
gbytes_per_s = bytes over the kernel time (a, b) or the batch time (c)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pl_batch_cases as C  # noqa: E402
from pseudo_lidar import CloudBatch, PseudoLiDAR, beam_tables  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
dev = "cuda"
B, h, w, H, W = a.batch, 192, 640, 375, 1242
P, T = C.scaled_P(C.DATES[0], H, W), C.velo_T(C.DATES[0])
disp = torch.from_numpy(np.stack([C.network_map(h, w, 300 + b, "disparity") for b in range(B)])).to(dev)
pl = PseudoLiDAR.from_matrices(T, P, 0)
sizes = [(H, W)] * B
tables = beam_tables()
dense_out, beam_out = CloudBatch(B, B * H * W, dev), CloudBatch(B, B * 64 * 512, dev)


def run_a():
    return pl.project_batch(disp, sizes=sizes, out=dense_out).counts()


def run_b():
    return pl.project_batch(disp, sizes=sizes, beams=tables, out=beam_out).counts()


def run_c():
    depth = torch.nn.functional.interpolate((1.0 / (10.0 * disp + 0.01))[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    return [pl.project_PL(depth[b]) for b in range(B)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / a.iters


def kernels(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return sorted(1000.0 * e0.elapsed_time(e1) for e0, e1 in ev)[a.iters // 2]


runs = {"a_dense": run_a, "b_beams": run_b, "c_project_PL": run_c}
for fn in runs.values():
    for _ in range(5):
        fn()
rounds = {k: [] for k in runs}
for _ in range(a.rounds):
    for k, fn in runs.items():
        rounds[k].append(round(timed(fn), 1))
ka = kernels(lambda: pl.project_batch(disp, sizes=sizes, out=dense_out))
kb = kernels(lambda: pl.project_batch(disp, sizes=sizes, beams=tables, out=beam_out))

na, nb = int(run_a()[-1]), int(run_b()[-1])
old = run_c()
nc = sum(int(c.shape[0]) for c in old)
# (nc may differ from na by a few points: the stock resize differs from the protocol's by an ulp here and there, which can move a pixel
# across a cut)
bytes_a = 4 * B * h * w + 16 * na
bytes_b = 4 * B * h * w + 16 * nb + 8 * B * 64 * 512
bytes_c = 8 * B * h * w + 4 * B * h * w + 4 * B * H * W + 4 * B * H * W + 32 * nc
med = lambda v: sorted(v)[len(v) // 2]
print(json.dumps({"workload": "pseudo-LiDAR B=%d %dx%d -> %dx%d" % (B, h, w, H, W), "iters": a.iters,
                  "us_per_batch": {k: {"rounds": v, "median": med(v)} for k, v in rounds.items()},
                  "a_dense_kernels_us": round(ka, 1), "b_beams_kernels_us": round(kb, 1),
                  "points": {"a_dense": na, "b_beams": nb, "c_project_PL": nc},
                  "bytes": {"a_dense": bytes_a, "b_beams": bytes_b, "c_project_PL": bytes_c},
                  "gbytes_per_s": {"a_dense": round(bytes_a / ka / 1e3, 1), "b_beams": round(bytes_b / kb / 1e3, 1),
                                   "c_project_PL": round(bytes_c / med(rounds["c_project_PL"]) / 1e3, 1)},
                  "a_not_slower_than_c": med(rounds["a_dense"]) <= med(rounds["c_project_PL"])}))
