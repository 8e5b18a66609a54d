#!/usr/bin/env python3
"""Times the soft-occupancy grid (pseudo_lidar.occupancy / occupancy_backward) and prints one JSON line.  Workload: B = 12 maps of
192 x 640 (a seeded KITTI-like scene: tests/pl_batch_cases.py, its NaN and infinity replaced) -> clouds at 375 x 1242, dense and as
64 x 512 beams -> PIXOR's 700 x 800 x 35 canvas of 0.1 m cells, sigma2 = 0.01.
usage: python tools/quant_bench.py [--batch 12] [--iters 30] [--stock-iters 5] [--rounds 3]
Per cloud kind (us, the median of --iters event pairs, alternated --rounds times, every round listed):
  forward             occupancy(out=...)                      (mcav_cloud_occupancy: a memset of the column counters and 7 launches)
  forward_counts      occupancy(out=..., provenance=True)     the same with point_count
  forward_empty       the same call on offsets of zeros: the sort's passes over the counters and the canvas write, no point work
  backward            occupancy_backward(out=...)             (mcav_cloud_occupancy_bwd: one launch)
  backward_project    occupancy_backward, then project_batch_backward on its result: canvas gradient -> disparity gradient
  memset              canvas.zero_(): the floor, one write of the canvas
  stock_forward, stock_backward   the stock PyTorch formulation on the same rows, float32: cell indices by floor, bincount for the
                      counts, then per offset of the 3 x 3 x 3 block exp(-d2 / sigma2) * w / n put into a zero canvas with
                      index_put_(accumulate=True); the backward is torch.autograd.grad through that graph (built once, retain_graph).
                      --stock-iters event pairs.
ratios: each of the product's times over the memset floor and over the stock formulation's.  max_diff: the largest difference between
the two formulations over the largest magnitude (float32 atomics in another order, expf, no fixed point)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pl_batch_cases as C  # noqa: E402
from pseudo_lidar import (CloudBatch, OccupancyBatch, PseudoLiDAR, VoxelGrid, beam_tables, occupancy, occupancy_backward,  # noqa: E402
                          project_batch_backward)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--stock-iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--kinds", default="beams,dense")
ap.add_argument("--no-stock", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("quant_bench: needs the GPU; a CPU run says nothing about these times")
dev = "cuda"
B, h, w, H, W = a.batch, 192, 640, 375, 1242
SIGMA2 = 0.01
P, T = C.scaled_P(C.DATES[0], H, W), C.velo_T(C.DATES[0])
maps = np.stack([C.network_map(h, w, 300 + b, "disparity") for b in range(B)])
maps[~np.isfinite(maps)] = np.float32(0.02)
disp = torch.from_numpy(maps).to(dev)
pl = PseudoLiDAR.from_matrices(T, P, 0)
sizes = [(H, W)] * B
grid = VoxelGrid()
med = lambda v: sorted(v)[len(v) // 2]


def kernels(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return round(med([1000.0 * e0.elapsed_time(e1) for e0, e1 in ev]), 1)


def stock_canvas(pts, image):
    """float32 torch, differentiable in pts [n, 3]; image: the image of every row -> [B, nz, ny, nx]"""
    origin = torch.tensor([grid.x[0], grid.y[0], grid.z[0]], device=dev)
    size = torch.tensor(grid.size, device=dev)
    cells = torch.tensor([grid.nx, grid.ny, grid.nz], device=dev)
    idx = torch.floor((pts.detach() - origin) / size)
    keep = ((idx >= 0) & (idx < cells)).all(dim=1)
    p, idx, b = pts[keep], idx[keep].long(), image[keep]
    flat = ((b * grid.nz + idx[:, 2]) * grid.ny + idx[:, 1]) * grid.nx + idx[:, 0]
    total = B * grid.nz * grid.ny * grid.nx
    n = torch.bincount(flat, minlength=total)[flat].float()
    canvas = torch.zeros(total, device=dev)
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                j = idx + torch.tensor([ox, oy, oz], device=dev)
                inside = ((j >= 0) & (j < cells)).all(dim=1)
                centre = j[inside].float() * size + (size * 0.5 + origin)
                d2 = ((p[inside] - centre) ** 2).sum(dim=1)
                weight = 1.0 if (ox, oy, oz) == (0, 0, 0) else 1.0 / 26.0
                val = torch.exp(-d2 / SIGMA2) * (weight / n[inside])
                to = ((b[inside] * grid.nz + j[inside, 2]) * grid.ny + j[inside, 1]) * grid.nx + j[inside, 0]
                canvas.index_put_((to,), val, accumulate=True)
    return canvas.view(B, grid.nz, grid.ny, grid.nx)


result = {"workload": "B=%d %dx%d -> %dx%d, canvas %dx%dx%d, sigma2=%g" % (B, h, w, H, W, grid.nx, grid.ny, grid.nz, SIGMA2),
          "canvas_bytes": 4 * B * grid.nz * grid.ny * grid.nx, "iters": a.iters, "stock_iters": a.stock_iters, "clouds": {}}
gen = torch.Generator(dev).manual_seed(11)
d_canvas = torch.randn(B, grid.nz, grid.ny, grid.nx, device=dev, generator=gen)
for kind in a.kinds.split(","):
    tables = beam_tables() if kind == "beams" else None
    cap = B * 64 * 512 if tables is not None else B * H * W
    cloud = CloudBatch(B, cap, dev)
    pl.project_batch(disp, sizes=sizes, beams=tables, out=cloud, provenance=True)
    n = int(cloud.counts()[-1])
    held, plain = OccupancyBatch(B, grid, dev), OccupancyBatch(B, grid, dev)
    occupancy(cloud.points, cloud.offsets, grid=grid, sigma2=SIGMA2, out=held, provenance=True)
    kept = int((held.point_count[:n] > 0).sum())
    no_rows = torch.zeros_like(cloud.offsets)
    d_points, d_m = torch.empty(cap, 4, device=dev), torch.empty(B, h, w, device=dev)
    runs = {
        "forward": lambda: occupancy(cloud.points, cloud.offsets, grid=grid, sigma2=SIGMA2, out=plain),
        "forward_counts": lambda: occupancy(cloud.points, cloud.offsets, grid=grid, sigma2=SIGMA2, out=held, provenance=True),
        "forward_empty": lambda: occupancy(cloud.points, no_rows, grid=grid, sigma2=SIGMA2, out=plain),
        "backward": lambda: occupancy_backward(held, d_canvas, out=d_points),
        "backward_project": lambda: project_batch_backward(cloud, occupancy_backward(held, d_canvas, out=d_points), out=d_m),
        "memset": lambda: plain.canvas.zero_(),
    }
    stock = {}
    if not a.no_stock:
        image = torch.bucketize(torch.arange(n, device=dev), cloud.offsets.long()[1:-1], right=True)
        leaf = cloud.points[:n, :3].clone().requires_grad_(True)
        s_canvas = stock_canvas(leaf, image)
        stock = {"stock_forward": lambda: stock_canvas(leaf, image),
                 "stock_backward": lambda: torch.autograd.grad(s_canvas, leaf, d_canvas, retain_graph=True)}
    for k, fn in list(runs.items()) + list(stock.items()):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        print("%s %s warmed up" % (kind, k), file=sys.stderr, flush=True)
    rounds = {k: [] for k in list(runs) + list(stock)}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            rounds[k].append(kernels(fn, a.iters))
        for k, fn in stock.items():
            rounds[k].append(kernels(fn, a.stock_iters))
        print("%s round: %s" % (kind, {k: v[-1] for k, v in rounds.items()}), file=sys.stderr, flush=True)
    us = {k: {"rounds": v, "median": med(v)} for k, v in rounds.items()}
    entry = {"points": n, "kept": kept, "us": us,
             "over_memset": {k: round(us[k]["median"] / us["memset"]["median"], 2) for k in runs if k != "memset"}}
    runs["forward_counts"](); runs["backward"]()
    if stock:
        sg, = stock["stock_backward"]()
        entry["over_stock"] = {"forward": round(us["forward"]["median"] / us["stock_forward"]["median"], 4),
                               "backward": round(us["backward"]["median"] / us["stock_backward"]["median"], 4)}
        entry["max_diff"] = {"canvas": float((s_canvas.detach() - held.canvas).abs().max() / held.canvas.abs().max()),
                             "d_points": float((sg - d_points[:n, :3]).abs().max() / d_points[:n, :3].abs().max())}
        del s_canvas, leaf, sg
    result["clouds"][kind] = entry
    del cloud, held, plain
    torch.cuda.empty_cache()
print(json.dumps(result))
