#!/usr/bin/env python3
"""Times the graph-based depth correction (pseudo_lidar.gdc) and prints one JSON line.  Workload: B = 12 maps of 192 x 640 of the seeded
scene of tests/gdc_cases.py (wall, ground plane, box; a smooth 5-15 % error on the prediction), known depths on every second pixel of four
rows (four synthetic beams), k = 10, radius = 3.
usage: python tools/gdc_bench.py [--batch 12] [--iters 20] [--rounds 3] [--converge 3000]
  graph        mcav_gdc_graph alone: us per dispatch
  iteration    one conjugate-gradient iteration (3 launches): (solve at 150 iterations - solve at 50) / 100, tol = 0 so that none stops
  call_400     pseudo_lidar.gdc as called by default (graph + solve, iters = 400, tol = 1e-4), and the same with tol = 0
  torch        a stock-torch composition of the same iteration on the same graph: a gather and a sum for M p, index_add_ for M^T q, float64
               dots on the device, no host synchronisation; (150 - 50) / 100 as well
Each figure is the median of --iters per-dispatch event pairs (us) after 2 warm-up calls; hip and torch are alternated --rounds times in
one session and every round is listed.  converge: the iterations each image needs to reach tol = 1e-4 (info column 2) with --converge
allowed, and its final rs / rs0.  bytes: the algorithmic traffic of one iteration over the graph pixels -- M p: k (4 + 4 + 4) + 4 + 4 + 1;
the update with M^T q: in-degree (8 + 4) + 8 + 4 + 8 + 4 + 8 + 1 with a mean in-degree of k; p: 4 + 8 + 1 -- 24 k + 54 B per pixel.
The batch's working set (~(16 k + 40) B per pixel, 300 MB at B = 12) is beyond the 32 MiB of L2 and about the Infinity Cache's 256 MiB, so
the bound to hold the iteration against is the memory system's gather rate, not the L2's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gdc_cases as GC  # noqa: E402
from mcav import lib as L  # noqa: E402
from pseudo_lidar import GDCResult, gdc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--converge", type=int, default=3000)
a = ap.parse_args()
dev = "cuda"
B, H, W, k, radius = a.batch, 192, 640, 10, 3
Ks = np.stack([GC.intrinsics(H, W, 0.25 * b) for b in range(B)])
parts = [GC.scene(H, W, Ks[b], 700 + b) for b in range(B)]
truth = np.stack([p[0] for p in parts])
depth = torch.from_numpy(np.stack([p[1] for p in parts])).to(dev)
sparse = torch.from_numpy(np.stack([p[2] for p in parts])).to(dev)
K = torch.from_numpy(Ks).to(dev)
out = GDCResult(B, H, W, k, dev)
res = gdc(depth, sparse, K, k=k, radius=radius, iters=0, out=out)
hl = L.lib()


def graph_only():
    L.check(hl.mcav_gdc_graph(L.ptr(depth), L.ptr(sparse), L.ptr(K), B, H, W, k, radius, 1e-3, 1e-3, 80.0, L.ptr(out.nbr), L.ptr(out.weights),
                              L.ptr(out.flags), L.ptr(out._ws), out._ws.numel(), L.stream()), "mcav_gdc_graph")


def solve_only(iters, tol=0.0):
    L.check(hl.mcav_gdc_solve(L.ptr(depth), L.ptr(sparse), L.ptr(out.nbr), L.ptr(out.weights), L.ptr(out.flags), B, H, W, k, radius, 1, iters,
                              tol, L.ptr(out.depth), L.ptr(out.info), L.ptr(out._ws), out._ws.numel(), L.stream()), "mcav_gdc_solve")


# ---- the stock-torch composition of the iteration, on the kernels' graph
n = H * W
base = (torch.arange(B, device=dev) * n).view(B, 1, 1)
nbr = out.nbr.view(B, n, k).long()
used = (nbr >= 0) & ((out.flags.view(B, n, 1) & 1) != 0)
cols = torch.where(used, nbr + base, torch.zeros_like(nbr)).view(-1, k)
wts = torch.where(used, out.weights.view(B, n, k), torch.zeros_like(out.weights.view(B, n, k))).view(-1, k)
graph_px = ((out.flags.view(-1) & 1) != 0)
unknown = ((out.flags.view(-1) & 3) == 1).float()
flat_cols, flat_w = cols.reshape(-1), wts.reshape(-1)


def M(v):
    return torch.where(graph_px, v - (wts * v[cols]).sum(1), torch.zeros_like(v))


def Mt(q):
    return q - torch.zeros_like(q).index_add_(0, flat_cols, flat_w * q.repeat_interleave(k))


def dots(v):
    return (v.double().view(B, n) ** 2).sum(1)


def torch_solve(iters):
    x = torch.where((out.flags.view(-1) & 3) == 3, sparse.view(-1), depth.view(-1))
    x = torch.where(graph_px, x, torch.zeros_like(x))
    r = -Mt(M(x)) * unknown
    p, rs = r.clone(), dots(r)
    for _ in range(iters):
        q = M(p)
        alpha = (rs / dots(q)).float().repeat_interleave(n)
        x = x + alpha * p
        r = r - alpha * Mt(q) * unknown
        rs_new = dots(r)
        p = r + (rs_new / rs).float().repeat_interleave(n) * p
        rs = rs_new
    return x


def timed(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return sorted(1000.0 * e0.elapsed_time(e1) for e0, e1 in ev)[a.iters // 2]


med = lambda v: sorted(v)[len(v) // 2]
runs = {"graph": graph_only, "solve_50": lambda: solve_only(50), "solve_150": lambda: solve_only(150),
        "call_400": lambda: gdc(depth, sparse, K, k=k, radius=radius, iters=400, out=out),
        "call_400_tol0": lambda: gdc(depth, sparse, K, k=k, radius=radius, iters=400, tol=0.0, out=out),
        "torch_50": lambda: torch_solve(50), "torch_150": lambda: torch_solve(150)}
for fn in runs.values():
    for _ in range(2):
        fn()
torch.cuda.synchronize()
rounds = {name: [] for name in runs}
for _ in range(a.rounds):
    for name, fn in runs.items():
        rounds[name].append(round(timed(fn), 1))
m = {name: med(v) for name, v in rounds.items()}
# the composition computes what the kernels compute
solve_only(5)
same = float((torch_solve(5).view(B, H, W) - out.depth)[graph_px.view(B, H, W)].abs().max())
gdc(depth, sparse, K, k=k, radius=radius, iters=a.converge, tol=1e-4, out=out)
info = out.info.cpu().numpy()
t = truth.astype(np.float64)
err = lambda z: float(np.mean(np.abs(z.cpu().numpy() - t) / t))
gdc(depth, sparse, K, k=k, radius=radius, iters=400, out=out)
graph_pixels = int(info[:, 0].sum())
nbytes = graph_pixels * (24 * k + 54)
it_us = (m["solve_150"] - m["solve_50"]) / 100.0
torch_us = (m["torch_150"] - m["torch_50"]) / 100.0
print(json.dumps({
    "workload": "gdc B=%d %dx%d k=%d radius=%d, %d known pixels per image" % (B, H, W, k, radius, int(info[0, 1])), "iters": a.iters,
    "us_per_dispatch": {name: {"rounds": v, "median": m[name]} for name, v in rounds.items()},
    "graph_us": m["graph"], "iteration_us": round(it_us, 2), "torch_iteration_us": round(torch_us, 2),
    "torch_over_hip": round(torch_us / it_us, 2), "torch_minus_hip_after_5_iterations_m": same,
    "call_400_us": m["call_400"], "call_400_tol0_us": m["call_400_tol0"],
    "converge": {"allowed": a.converge, "iterations": info[:, 2].astype(int).tolist(), "rs_over_rs0": [float("%.3g" % v) for v in info[:, 3]]},
    "mean_relative_error": {"prediction": err(depth), "after_400": err(out.depth)},
    "bytes_per_iteration": nbytes, "gbytes_per_s": round(nbytes / it_us / 1e3, 1)}))
