#!/usr/bin/env python3
"""Times the pillar voxeliser and prints one JSON line.  Workload: B = 12 clouds made by PseudoLiDAR.project_batch from 192 x 640
disparities (a seeded scene: tests/pl_batch_cases.py) at 375 x 1242, dense and as 64 x 512 beams, voxelised on PointPillars' KITTI grid
(432 x 496 pillars of 0.16 m) with N = 32 slots, plain (C = 4) and decorated (C = 9).
usage: python tools/pillar_bench.py [--batch 12] [--iters 50] [--rounds 3] [--points 32]
  hip    pseudo_lidar.pillarize(out=...) (mcav_pillarize: memset + 6 kernels), nothing read back
  torch  the same definition composed from stock torch operations on the same GPU: cell ids, torch.unique with the inverse, a stable sort by
         (cell, index), ranks within the cell, index_put (and for C = 9 the float64 means by index_add).  torch.unique sizes its result on
         the host, so this path synchronises once per call; the tree had no such path: this is the baseline.
Each figure is the median of --iters per-dispatch event pairs (us), after 5 warm-up calls; hip and torch are alternated --rounds times in
one session and every round is listed.  equal: whether the torch composition's offsets, coords, num_points and voxels (the x, y, z, i
columns) equal the kernels' bit for bit.  bytes: the algorithmic traffic -- 16 B read per live point, P * N * C * 4 + P * 20 B written -- and the share of
8 TB/s they make at the hip median."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pl_batch_cases as PC  # noqa: E402
from pseudo_lidar import PillarBatch, PillarGrid, PseudoLiDAR, beam_tables, pillarize  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--points", type=int, default=32)
a = ap.parse_args()
dev = "cuda"
B, N, h, w, H, W = a.batch, a.points, 192, 640, 375, 1242
grid = PillarGrid()
x0, y0, z0, z1, vx, vy = (float(np.float32(v)) for v in grid.scalars())
M = B * grid.ny * grid.nx
disp = torch.from_numpy(np.stack([PC.network_map(h, w, 300 + b, "disparity") for b in range(B)])).to(dev)
pl = PseudoLiDAR.from_matrices(PC.velo_T(PC.DATES[0]), PC.scaled_P(PC.DATES[0], H, W), 0)
clouds = {"dense": pl.project_batch(disp, sizes=[(H, W)] * B), "beams": pl.project_batch(disp, sizes=[(H, W)] * B, beams=beam_tables(64, 512))}


vx_t, vy_t = torch.tensor(vx, device=dev), torch.tensor(vy, device=dev)      # torch divides by a Python scalar through its reciprocal


def torch_pillarize(points, offsets, decorate):
    n_max = points.shape[0]
    i = torch.arange(n_max, device=dev)
    live = i < offsets[-1].clamp(max=n_max)
    b = torch.searchsorted(offsets[1:-1].to(torch.int64).contiguous(), i, right=True)
    fx, fy = torch.floor((points[:, 0] - x0) / vx_t), torch.floor((points[:, 1] - y0) / vy_t)      # a tensor divisor: an IEEE division
    keep = live & (fx >= 0) & (fx < grid.nx) & (fy >= 0) & (fy < grid.ny) & (points[:, 2] >= z0) & (points[:, 2] < z1)
    ix, iy = torch.where(keep, fx, 0.0).to(torch.int64), torch.where(keep, fy, 0.0).to(torch.int64)
    cell = torch.where(keep, (b * grid.ny + iy) * grid.nx + ix, M)
    ucell, inv = torch.unique(cell, return_inverse=True)
    sc, order = torch.sort(cell, stable=True)                 # by (cell, index)
    start = torch.searchsorted(sc, ucell)
    grp = inv[order]
    slot = torch.arange(n_max, device=dev) - start[grp]
    take = (slot < N) & (sc < M)
    P = ucell.numel() - int(ucell[-1] == M)                   # the dropped points' cell sorts last
    C = 9 if decorate else 4
    vox = torch.zeros((P, N, C), device=dev)
    g, s, rows = grp[take], slot[take], points[order[take]]
    vox[:, :, :4].index_put_((g, s), rows)
    num = torch.zeros(P, dtype=torch.int32, device=dev).index_add_(0, g, torch.ones_like(g, dtype=torch.int32))
    pc = ucell[:P]
    pb = pc // (grid.ny * grid.nx)
    piy, pix = (pc // grid.nx) % grid.ny, pc % grid.nx
    coords = torch.stack([pb, torch.zeros_like(pb), piy, pix], dim=1).to(torch.int32)
    poff = torch.searchsorted(pb, torch.arange(B + 1, device=dev)).to(torch.int32)
    if decorate:
        mean = (torch.zeros((P, 3), dtype=torch.float64, device=dev).index_add_(0, g, rows[:, :3].double()) / num[:, None]).float()
        used = torch.arange(N, device=dev)[None, :] < num[:, None]
        vox[:, :, 4:7] = torch.where(used[:, :, None], vox[:, :, :3] - mean[:, None, :], 0.0)
        vox[:, :, 7] = torch.where(used, vox[:, :, 0] - (pix.float() * vx + (vx * 0.5 + x0))[:, None], 0.0)
        vox[:, :, 8] = torch.where(used, vox[:, :, 1] - (piy.float() * vy + (vy * 0.5 + y0))[:, None], 0.0)
    return vox, coords, num, poff


def kernels(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return sorted(1000.0 * e0.elapsed_time(e1) for e0, e1 in ev)[a.iters // 2]


med = lambda v: sorted(v)[len(v) // 2]
result = {"workload": "pillars B=%d %dx%d grid N=%d, clouds of %dx%d from %dx%d" % (B, grid.nx, grid.ny, N, H, W, h, w), "iters": a.iters,
          "runs": {}}
for kind, cb in clouds.items():
    for decorate in (False, True):
        C = 9 if decorate else 4
        out = PillarBatch(B, min(cb.points.shape[0], M), N, C, dev)
        runs = {"hip": lambda: pillarize(cb.points, cb.offsets, grid=grid, max_points=N, decorate=decorate, out=out),
                "torch": lambda: torch_pillarize(cb.points, cb.offsets, decorate)}
        for fn in runs.values():
            for _ in range(5):
                fn()
        rounds = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                rounds[k].append(round(kernels(fn), 1))
        pb = runs["hip"]()
        vox, coords, num, poff = runs["torch"]()
        P, n = int(pb.counts()[-1]), int(min(cb.counts()[-1], cb.points.shape[0]))
        equal = P == vox.shape[0] and torch.equal(pb.offsets, poff)
        equal = {"offsets": bool(equal), "coords": bool(equal and torch.equal(pb.coords[:P], coords)),
                 "num_points": bool(equal and torch.equal(pb.num_points[:P], num)),
                 "voxels": bool(equal and torch.equal(pb.voxels[:P, :, :4].view(torch.int32), vox[:, :, :4].view(torch.int32)))}
        nbytes = 16 * n + P * N * C * 4 + P * 20
        us = med(rounds["hip"])
        result["runs"]["%s_c%d" % (kind, C)] = {
            "points": n, "pillars": P, "us_per_dispatch": {k: {"rounds": v, "median": med(v)} for k, v in rounds.items()},
            "torch_over_hip": round(med(rounds["torch"]) / us, 2), "equal": equal, "bytes": nbytes,
            "gbytes_per_s": round(nbytes / us / 1e3, 1), "share_of_8TBps": round(nbytes / us / 1e3 / 8000.0, 4)}
print(json.dumps(result))
