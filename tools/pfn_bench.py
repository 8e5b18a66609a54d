#!/usr/bin/env python3
"""Times the pillar feature net + pseudo-image call and prints one JSON line.  Workload: B = 12 clouds made by PseudoLiDAR.project_batch from
192 x 640 disparities (a seeded scene: tests/pl_batch_cases.py) at 375 x 1242, dense and as 64 x 512 beams (as tools/pillar_bench.py builds
them), voxelised on PointPillars' KITTI grid (432 x 496) with N = 32 slots and the 9 decorated columns, under a seeded layer of 64 channels:
the canvas is 12 x 64 x 496 x 432 float32 = 658 MB.
usage: python tools/pfn_bench.py [--batch 12] [--iters 30] [--rounds 3] [--points 32] [--channels 64] [--backward | --batch-stats]
  nchw / nhwc  PillarFeatureNet.pseudo_image(out=...) (mcav_pillar_pseudo_image: one launch), nothing read back
  features     PillarFeatureNet.features(out=...): the layer alone, no canvas
  torch        the stock formulation on the same device and inputs: F.linear over [P, N, C], the folded BatchNorm as a scale and a shift,
               relu, max(dim=1), torch.zeros for the canvas, indexed assignment into NCHW.  It is given the pillar count and its int64
               indices for free (read back and built once outside the timed region); the kernel reads the count on the device.
Each figure is the median of --iters per-dispatch event pairs (us) after 5 warm-up calls; the paths are alternated --rounds times in one
session and every round is listed.  max_abs_diff: the torch canvas against the kernel's (the torch path rounds in another order, so the
last bits differ).  bytes: what the call must move -- written: the canvas (and nothing else); read: P N C 4 + 20 P + the layer -- and the
share of 8 TB/s they make at the nchw median; the canvas alone is the floor: a memset of it is timed beside the rest.
--backward times the backward instead (mcav_pillar_pseudo_image_bwd, two launches) on the same clouds under a seeded normal canvas gradient:
  bwd_<layout>[_vox]     PillarFeatureNet.gradients(out=...) alone, without and with d_voxels
  fwdbwd_<layout>[_vox]  pseudo_image(out=...) followed by gradients(out=...)
  torch_fwdbwd[_vox]     autograd through the stock formulation above, forward and backward, the parameters (and the voxels) requiring a
                         gradient; torch_fwd is its forward with the graph recorded
bytes: what a backward must move -- read: P N C 4 + 24 P + P C_out 4 of the gradient (an NCHW gradient comes in 32-byte sectors, so up to
8 times that); written: capacity N C 4 for d_voxels and the slab -- and their share of 8 TB/s at the median.
--batch-stats times training-mode BatchNorm statistics from the voxels' moments on the same clouds:
  moments / moments_bwd  pillar_moments(out=...) (mcav_pillar_moments: two launches) and pillar_moments_backward(out=...) (one launch)
  voxels_sum             torch.sum over the whole voxels tensor: the floor of a pass over it, as the memset is the canvas's
  step_batch             PillarFeatureLayer(batch_stats=True) in train(): forward to the NCHW canvas, backward under a seeded normal canvas
                         gradient with the voxels requiring a gradient, the buffers' update
  step_frozen            the same step of the default layer (frozen statistics): the difference is what batch statistics cost
  torch_step             autograd through F.linear -> BatchNorm1d(train) over the [P N, C_out] rows -> relu -> max -> indexed scatter, the
                         voxels requiring a gradient"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pl_batch_cases as PC  # noqa: E402
from pseudo_lidar import (PillarFeatureLayer, PillarFeatureNet, PillarGrid, PseudoLiDAR, beam_tables, pillar_moments,  # noqa: E402
                          pillar_moments_backward)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--points", type=int, default=32)
ap.add_argument("--channels", type=int, default=64)
ap.add_argument("--backward", action="store_true")
ap.add_argument("--batch-stats", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("pfn_bench: needs the GPU; a CPU run says nothing about these times")
dev = "cuda"
B, N, CO, h, w, H, W = a.batch, a.points, a.channels, 192, 640, 375, 1242
grid = PillarGrid()
disp = torch.from_numpy(np.stack([PC.network_map(h, w, 300 + b, "disparity") for b in range(B)])).to(dev)
pl = PseudoLiDAR.from_matrices(PC.velo_T(PC.DATES[0]), PC.scaled_P(PC.DATES[0], H, W), 0)
clouds = {"dense": pl.project_batch(disp, sizes=[(H, W)] * B), "beams": pl.project_batch(disp, sizes=[(H, W)] * B, beams=beam_tables(64, 512))}

rng = np.random.RandomState(5)
weight = torch.from_numpy((0.1 * rng.randn(CO, 9)).astype(np.float32)).to(dev)
scale = torch.from_numpy((1.0 + 0.1 * rng.randn(CO)).astype(np.float32)).to(dev)
shift = torch.from_numpy((0.1 * rng.randn(CO)).astype(np.float32)).to(dev)
net = PillarFeatureNet((weight * scale[:, None]).contiguous(), shift)                    # the fold, as from_state_dict does it


def kernels(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return sorted(1000.0 * e0.elapsed_time(e1) for e0, e1 in ev)[a.iters // 2]


med = lambda v: sorted(v)[len(v) // 2]
shape = (B, CO, grid.ny, grid.nx)
canvas_bytes = 4 * B * CO * grid.ny * grid.nx
result = {"workload": "pseudo-image B=%d %dx%d grid N=%d C=9 C_out=%d, clouds of %dx%d from %dx%d" % (B, grid.nx, grid.ny, N, CO, H, W, h, w),
          "iters": a.iters, "canvas_bytes": canvas_bytes, "runs": {}}
out_nchw = torch.empty(shape, device=dev)
out_nhwc = torch.empty(shape, device=dev, memory_format=torch.channels_last)


def backward_runs(kind, pb):
    """-> the --backward entry of one cloud kind"""
    P, cap = int(min(pb.counts()[-1], pb.voxels.shape[0])), pb.voxels.shape[0]
    idx = pb.coords[:P].long()
    ib, iy, ix = idx[:, 0].contiguous(), idx[:, 2].contiguous(), idx[:, 3].contiguous()
    gen = torch.Generator(device=dev).manual_seed(9)
    up = {"nchw": torch.randn(shape, device=dev, generator=gen)}
    up["nhwc"] = up["nchw"].contiguous(memory_format=torch.channels_last)
    canvas = {"nchw": out_nchw, "nhwc": out_nhwc}
    small = [torch.empty(s, device=dev) for s in ((CO, 9), (CO,), (CO,))]
    d_vox = torch.empty_like(pb.voxels)
    wt, sc, sh = (t.clone().requires_grad_(True) for t in (weight, scale, shift))

    def torch_form(vox_grad, backward=True):
        v = pb.voxels[:P].detach().requires_grad_(vox_grad)
        f = torch.relu(torch.nn.functional.linear(v, wt) * sc + sh).max(dim=1).values
        c = torch.zeros(shape, device=dev)
        c[ib, :, iy, ix] = f
        if backward:
            c.backward(up["nchw"])
        grads = (wt.grad, sc.grad, sh.grad, v.grad)
        wt.grad = sc.grad = sh.grad = None
        return grads

    runs = {}
    for lay in ("nchw", "nhwc"):
        for vox in (False, True):
            tag = lay + ("_vox" if vox else "")
            bwd = lambda lay=lay, vox=vox: net.gradients(pb, grad_canvas=up[lay], layout=lay, need_voxels=vox, out=small + ([d_vox] if vox else []))
            runs["bwd_" + tag] = bwd
            runs["fwdbwd_" + tag] = lambda lay=lay, bwd=bwd: (net.pseudo_image(pb, layout=lay, out=canvas[lay]), bwd())
    runs.update(torch_fwd=lambda: torch_form(False, False), torch_fwdbwd=lambda: torch_form(False), torch_fwdbwd_vox=lambda: torch_form(True))
    for fn in runs.values():
        for _ in range(5):
            fn()
    rounds = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            rounds[k].append(round(kernels(fn), 1))
    dw, db, dp, dv = (t.clone() for t in runs["bwd_nchw_vox"]())
    tw, ts, tsh, tv = torch_form(True)
    same = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip((dw, db, dp, dv), runs["bwd_nhwc_vox"]()))
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    read = P * N * 9 * 4 + P * 24 + P * CO * 4 + 4 * CO * 11
    slab = 8 * CO * 11 * min(-(-cap // 64), 1024)
    entry = {"pillars": P, "capacity": cap, "us_per_dispatch": {k: {"rounds": v, "median": med(v)} for k, v in rounds.items()},
             "nhwc_equals_nchw": same, "rel_diff_to_torch": {"d_shift": rel(db + dp, tsh), "d_voxels": rel(dv[:P], tv),
                                                              "d_weight": rel(dw, tw / scale[:, None])},
             "bytes": {}}
    for vox in (False, True):
        tag = "bwd_nchw" + ("_vox" if vox else "")
        moved = read + slab + (cap * N * 9 * 4 if vox else 0)
        us = med(rounds[tag])
        entry["bytes"][tag] = {"read": read, "written": moved - read, "gbytes_per_s": round(moved / us / 1e3, 1),
                               "share_of_8TBps": round(moved / us / 1e3 / 8000.0, 4)}
    entry["torch_fwdbwd_over_fwdbwd_nchw"] = round(med(rounds["torch_fwdbwd"]) / med(rounds["fwdbwd_nchw"]), 2)
    entry["torch_fwdbwd_vox_over_fwdbwd_nchw_vox"] = round(med(rounds["torch_fwdbwd_vox"]) / med(rounds["fwdbwd_nchw_vox"]), 2)
    return entry


def batch_stats_runs(kind, pb):
    """-> the --batch-stats entry of one cloud kind"""
    P, cap = int(min(pb.counts()[-1], pb.voxels.shape[0])), pb.voxels.shape[0]
    idx = pb.coords[:P].long()
    ib, iy, ix = idx[:, 0].contiguous(), idx[:, 2].contiguous(), idx[:, 3].contiguous()
    up = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    layers = {}
    for key, flag in (("step_batch", True), ("step_frozen", False)):
        layer = PillarFeatureLayer(9, CO, batch_stats=flag).to(dev).train()
        with torch.no_grad():
            layer.linear.weight.copy_(weight)
            layer.norm.weight.copy_(scale)
            layer.norm.bias.copy_(shift)
        layers[key] = layer
    moments = torch.empty(92, dtype=torch.float64, device=dev)
    grad = torch.randn(92, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(10))
    d_vox = torch.empty_like(pb.voxels)
    stock = torch.nn.BatchNorm1d(CO, eps=1e-3).to(dev).train()
    wt = weight.clone().requires_grad_(True)

    def step(layer):
        for p in layer.parameters():
            p.grad = None
        pb.voxels.grad = None
        layer(pb).backward(up)

    def torch_step():
        v = pb.voxels[:P].detach().requires_grad_(True)
        wt.grad = stock.weight.grad = stock.bias.grad = None
        y = stock(torch.nn.functional.linear(v, wt).reshape(P * N, CO)).reshape(P, N, CO)
        c = torch.zeros(shape, device=dev)
        c[ib, :, iy, ix] = torch.relu(y).max(dim=1).values
        c.backward(up)

    runs = {"moments": lambda: pillar_moments(pb, out=moments), "moments_bwd": lambda: pillar_moments_backward(pb, grad, out=d_vox),
            "voxels_sum": lambda: torch.sum(pb.voxels)}
    pb.voxels.requires_grad_(True)
    runs.update({k: (lambda layer=layer: step(layer)) for k, layer in layers.items()})
    runs["torch_step"] = torch_step
    plain = ("moments", "moments_bwd", "voxels_sum")
    rounds = {k: [] for k in runs}
    for k, fn in runs.items():
        with torch.set_grad_enabled(k not in plain):
            for _ in range(5):
                fn()
    for _ in range(a.rounds):
        for k, fn in runs.items():
            with torch.set_grad_enabled(k not in plain):
                rounds[k].append(round(kernels(fn), 1))
    pb.voxels.requires_grad_(False)
    pb.voxels.grad = None
    used = int(pillar_moments(pb)[1])
    us = {k: med(v) for k, v in rounds.items()}
    return {"pillars": P, "capacity": cap, "used_slots": used, "points_per_pillar": round(used / max(P, 1), 2),
            "us_per_dispatch": {k: {"rounds": v, "median": med(v)} for k, v in rounds.items()},
            "batch_statistics_cost_us": round(us["step_batch"] - us["step_frozen"], 1),
            "torch_step_over_step_batch": round(us["torch_step"] / us["step_batch"], 2),
            "moments_bytes_read": used * 36 + 4 * P, "moments_gbytes_per_s": round((used * 36 + 4 * P) / us["moments"] / 1e3, 1),
            "moments_bwd_bytes_written": cap * N * 36, "moments_bwd_gbytes_per_s": round(cap * N * 36 / us["moments_bwd"] / 1e3, 1),
            "torch_intermediate_bytes": 4 * P * N * CO}


for kind, cb in clouds.items():
    pb = cb.pillars(grid=grid, max_points=N, decorate=True)
    if a.backward or a.batch_stats:
        result["runs"][kind] = (backward_runs if a.backward else batch_stats_runs)(kind, pb)
        continue
    P = int(min(pb.counts()[-1], pb.voxels.shape[0]))
    feat = torch.empty((pb.voxels.shape[0], CO), device=dev)
    idx = pb.coords[:P].long()
    ib, iy, ix = idx[:, 0].contiguous(), idx[:, 2].contiguous(), idx[:, 3].contiguous()

    def torch_form():
        x = torch.nn.functional.linear(pb.voxels[:P], weight)
        x = torch.relu(x * scale + shift)
        f = x.max(dim=1).values
        canvas = torch.zeros(shape, device=dev)
        canvas[ib, :, iy, ix] = f
        return canvas

    runs = {"nchw": lambda: net.pseudo_image(pb, out=out_nchw), "nhwc": lambda: net.pseudo_image(pb, layout="nhwc", out=out_nhwc),
            "features": lambda: net.features(pb, out=feat), "torch": torch_form, "memset": lambda: out_nchw.zero_()}
    for fn in runs.values():
        for _ in range(5):
            fn()
    rounds = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            rounds[k].append(round(kernels(fn), 1))
    got, got_nhwc, want = runs["nchw"](), runs["nhwc"](), runs["torch"]()
    same_layouts = bool(torch.equal(got.view(torch.int32), got_nhwc.contiguous().view(torch.int32)))
    diff = float((got - want).abs().max())
    read = P * N * 9 * 4 + P * 20 + 4 * CO * 11
    us = med(rounds["nchw"])
    result["runs"][kind] = {
        "pillars": P, "us_per_dispatch": {k: {"rounds": v, "median": med(v)} for k, v in rounds.items()},
        "torch_over_nchw": round(med(rounds["torch"]) / us, 2), "nhwc_equals_nchw": same_layouts, "max_abs_diff_to_torch": diff,
        "bytes_written": canvas_bytes, "bytes_read": read, "gbytes_per_s": round((canvas_bytes + read) / us / 1e3, 1),
        "share_of_8TBps": round((canvas_bytes + read) / us / 1e3 / 8000.0, 4),
        "torch_intermediate_bytes": 4 * P * N * CO}
    del want, got, got_nhwc
print(json.dumps(result))
