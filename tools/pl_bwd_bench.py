#!/usr/bin/env python3
"""Times the two backwards that carry a gradient from pillar voxels back to the disparity and prints one JSON line.  Workload: B = 12 maps
of 192 x 640 (a seeded KITTI-like scene: tests/pl_batch_cases.py, its NaN and infinity replaced) -> clouds at 375 x 1242, dense and as
64 x 512 beams -> decorated pillars (C = 9) on PointPillars' KITTI grid.
usage: python tools/pl_bwd_bench.py [--batch 12] [--iters 30] [--rounds 3] [--points 32]
Per cloud kind (us, the median of --iters event pairs, alternated --rounds times, every round listed):
  project_plain / project_indexed     the forward without and with the provenance (mcav_pl_batch_project / _indexed)
  pillarize_plain / pillarize_indexed likewise (mcav_pillarize / _indexed)
  pillarize_bwd                       pseudo_lidar.pillarize_backward(out=...)   (mcav_pillarize_bwd: a memset and one launch)
  project_bwd                         pseudo_lidar.project_batch_backward(out=...) (mcav_pl_batch_project_bwd: a memset and two launches)
  stock_pillarize_bwd, stock_project_bwd   torch.autograd.grad through the stock PyTorch formulation of the same two steps on the same
                                      inputs, given the same selection as index tensors: the used slots' rows gathered by index and put into
                                      a zero block, the mean and centre offsets; F.interpolate, the depth, the un-projection, rows by index.
                                      The graph is built once outside the timed region (retain_graph), so this is the backward alone: the
                                      adjoint of the gathers is index_put_(accumulate=True), that of the resize
                                      upsample_bilinear2d_backward.  float32.  Every index occurs once (a formulation that clamps the padded
                                      slots onto row 0 makes index_put_ walk millions of repeats of one index and takes seconds).
max_abs_diff: the largest difference between the two formulations' gradients over the largest magnitude (they differ in rounding, and in
the plane where the stock resize's taps differ from the protocol's by an ulp)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pl_batch_cases as C  # noqa: E402
from pseudo_lidar import (CloudBatch, PillarBatch, PillarGrid, PseudoLiDAR, beam_tables, pillarize, pillarize_backward,  # noqa: E402
                          project_batch_backward)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--points", type=int, default=32)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("pl_bwd_bench: needs the GPU; a CPU run says nothing about these times")
dev = "cuda"
B, h, w, H, W, N = a.batch, 192, 640, 375, 1242, a.points
P, T = C.scaled_P(C.DATES[0], H, W), C.velo_T(C.DATES[0])
maps = np.stack([C.network_map(h, w, 300 + b, "disparity") for b in range(B)])
maps[~np.isfinite(maps)] = np.float32(0.02)
disp = torch.from_numpy(maps).to(dev)
pl = PseudoLiDAR.from_matrices(T, P, 0)
sizes = [(H, W)] * B
grid = PillarGrid()
med = lambda v: sorted(v)[len(v) // 2]


def kernels(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return round(med([1000.0 * e0.elapsed_time(e1) for e0, e1 in ev]), 1)


def stock_cloud(m, flat):
    """float32 torch: resize, depth, un-projection into the velodyne frame, the kept pixels by index -> [n, 3]"""
    v = torch.nn.functional.interpolate(m[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    d = 1.0 / (10.0 * v + 0.01)
    cu, cv, fu, fv = P[0, 2], P[1, 2], P[0, 0], P[1, 1]
    bx, by = P[0, 3] / -fu, P[1, 3] / -fv
    ti = np.linalg.inv(T)
    rr, cc = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    x = (cc - cu) * d / fu + bx
    y = (rr - cv) * d / fv + by
    q = torch.stack([x * ti[j, 0] + y * ti[j, 1] + d * ti[j, 2] + ti[j, 3] for j in range(3)], dim=-1)
    return q.reshape(-1, 3)[flat]


def stock_voxels(pts, where, rows, used, centres):
    """float32 torch: the used slots' rows by index into a zero block, PointPillars' decoration -> [P, N, 9]"""
    vox = torch.zeros(used.shape + (4,), device=dev).index_put(where, pts[rows])
    mean = vox[:, :, :3].sum(dim=1) / used.sum(dim=1)[:, None]
    return torch.cat([vox, (vox[:, :, :3] - mean[:, None, :]) * used[:, :, None], (vox[:, :, :2] - centres[:, None, :]) * used[:, :, None]], dim=2)


result = {"workload": "B=%d %dx%d -> %dx%d, pillars %dx%d N=%d C=9" % (B, h, w, H, W, grid.nx, grid.ny, N), "iters": a.iters, "clouds": {}}
for kind, tables in (("beams", beam_tables()), ("dense", None)):
    cap = B * 64 * 512 if tables is not None else B * H * W
    cloud, plain = CloudBatch(B, cap, dev), CloudBatch(B, cap, dev)
    project = lambda out, **kw: pl.project_batch(disp, sizes=sizes, beams=tables, out=out, **kw)
    project(cloud, provenance=True)
    n = int(cloud.counts()[-1])
    pcap = min(cap, B * grid.nx * grid.ny)
    pillars, pplain = PillarBatch(B, pcap, N, 9, dev), PillarBatch(B, pcap, N, 9, dev)
    voxelise = lambda out, **kw: pillarize(cloud.points, cloud.offsets, grid=grid, max_points=N, decorate=True, out=out, **kw)
    voxelise(pillars, provenance=True)
    Pn = int(pillars.counts()[-1])
    gen = torch.Generator(dev).manual_seed(11)
    d_voxels = torch.randn(pcap, N, 9, device=dev, generator=gen)
    d_points, d_m = torch.empty(cap, 4, device=dev), torch.empty(B, h, w, device=dev)
    runs = {
        "project_plain": lambda: project(plain),
        "project_indexed": lambda: project(cloud, provenance=True),
        "pillarize_plain": lambda: voxelise(pplain),
        "pillarize_indexed": lambda: voxelise(pillars, provenance=True),
        "pillarize_bwd": lambda: pillarize_backward(pillars, d_voxels, out=d_points),
        "project_bwd": lambda: project_batch_backward(cloud, d_points, out=d_m),
    }
    # the stock formulation on the same selection
    off = cloud.offsets.long()
    image = torch.bucketize(torch.arange(n, device=dev), off[1:-1], right=True)
    flat = image * (H * W) + cloud.pixels[:n].long()
    m_leaf = disp.clone().requires_grad_(True)
    s_cloud = stock_cloud(m_leaf, flat)
    pts_leaf = cloud.points[:n].clone().requires_grad_(True)
    slots = pillars.slot_points[:Pn].long()
    used = (slots >= 0).float()
    where = torch.nonzero(slots >= 0, as_tuple=True)                # every used slot once: no index repeats in either gather's adjoint
    co = pillars.coords[:Pn].float()
    centres = torch.stack([co[:, 3] * grid.size[0] + (grid.size[0] * 0.5 + grid.x[0]), co[:, 2] * grid.size[1] + (grid.size[1] * 0.5 + grid.y[0])], dim=1)
    s_vox = stock_voxels(pts_leaf, where, slots[where], used, centres)
    runs["stock_pillarize_bwd"] = lambda: torch.autograd.grad(s_vox, pts_leaf, d_voxels[:Pn], retain_graph=True)
    runs["stock_project_bwd"] = lambda: torch.autograd.grad(s_cloud, m_leaf, d_points[:n, :3], retain_graph=True)
    for k, fn in runs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        print("%s %s warmed up" % (kind, k), file=sys.stderr, flush=True)
    rounds = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            rounds[k].append(kernels(fn))
        print("%s round: %s" % (kind, {k: v[-1] for k, v in rounds.items()}), file=sys.stderr, flush=True)
    runs["pillarize_bwd"](); runs["project_bwd"]()
    sp, = runs["stock_pillarize_bwd"]()
    sm, = runs["stock_project_bwd"]()
    diff = {"d_points": float((sp - d_points[:n]).abs().max() / d_points[:n].abs().max()), "d_m": float((sm - d_m).abs().max() / d_m.abs().max())}
    result["clouds"][kind] = {"points": n, "pillars": Pn, "us": {k: {"rounds": v, "median": med(v)} for k, v in rounds.items()},
                              "max_abs_diff": diff}
    del s_cloud, s_vox, m_leaf, pts_leaf
print(json.dumps(result))
