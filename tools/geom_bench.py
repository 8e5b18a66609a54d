#!/usr/bin/env python3
"""Times the depth geometry-consistency term (mcav_geom_consistency_fwd / _bwd) alone, per dispatch, beside a stock-torch fp32 composition
of the same definition (tests/geom_consistency_ref.py: composition) on the GPU -- the parent has no such path, so that is the baseline.
usage: python tools/geom_bench.py [--batch 12 --height 192 --width 640] [--rot 0.005 --trans 0.02] [--iters 50] [--lds-tile]
--lds-tile: the backward's scatter through an LDS tile flushed once (MCAV_GC_LDS_TILE) instead of four global 64-bit atomics per pixel;
run the tool with and without it to time both forms.  Put tools/loss_bench.py beside it in the same session for the fused loss
kernel's time.
Inputs: smooth disparities in [0.05, 0.6]; --rot / --trans bound pose[:,0] (consecutive frames: small; the tests' 0.02 / 0.15 throw most
taps tens of pixels away)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import geom_consistency_ref as R  # noqa: E402
from losses import Losses  # noqa: E402
from mcav import nn as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--height", type=int, default=192)
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--rot", type=float, default=0.005)
ap.add_argument("--trans", type=float, default=0.02)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--lds-tile", action="store_true")
a = ap.parse_args()
dev = "cuda"
B, H, W = a.batch, a.height, a.width
dt, dr, poses, K = R.inputs(B, H, W, 3, rot=a.rot, trans=a.trans)
x, y, z = (t.float().to(dev).requires_grad_() for t in (dt, dr, poses))
Kd = K.to(dev)
crit = Losses(geometry_consistency=True)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def step():
    for p in (x, y, z):
        p.grad = None
    loss = crit.geometry_consistency_loss(x, y, z, Kd, lds_tile=a.lds_tile)
    loss.backward()
    return loss


for _ in range(10):
    loss = step()
torch.cuda.synchronize()
N.kernel_timer_begin()
for _ in range(a.iters):
    step()
torch.cuda.synchronize()
d = N.kernel_timer_end()
assert len(d) == 3 * a.iters, len(d)           # forward, scatter, combine (the two memset nodes are not kernels)
fwd, sc, cb = (1000.0 * median(d[i::3]) for i in range(3))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.iters):
    step()
e1.record()
torch.cuda.synchronize()
call_us = 1000.0 * e0.elapsed_time(e1) / a.iters
npx = B * H * W
# bytes per pixel of one frame (both directions together).  Algorithmic: each map read once and each gradient written once, forward and
# backward: 2 * 8 + 8 + 8.  As implemented: forward 2 x (4 read + 4 gathered); backward memset 16, scatter 2 x (4 + 4 gathered + 4 direct
# + 8 accumulator write-back), combine 2 x (4 direct + 8 accumulator + 4 map + 4 gradient).
alg, impl = 32.0, 16.0 + 16.0 + 40.0 + 40.0
weighted = crit.geometry_consistency_loss(x.detach(), y.detach(), z.detach(), Kd)
print("geometry consistency %s %dx%dx%d rot %g trans %g: forward %.1f us, scatter %.1f us, combine %.1f us = %.1f us of kernels (median of %d "
      "dispatches each); %.1f us per forward + backward call incl. the two memsets and the host; %.0f B/pixel algorithmic = %.0f GB/s, %.0f "
      "B/pixel as implemented = %.0f GB/s over the kernels; weighted loss %.6f" %
      ("LDS tile" if a.lds_tile else "plain atomics", B, H, W, a.rot, a.trans, fwd, sc, cb, fwd + sc + cb, a.iters, call_us, alg, alg * npx / ((fwd + sc + cb) * 1e-6) / 1e9, impl,
       impl * npx / ((fwd + sc + cb) * 1e-6) / 1e9, float(weighted)))

# the stock-torch fp32 composition of the same definition, forward + backward through autograd
xs, ys, zs = (t.detach().clone().requires_grad_() for t in (x, y, z))
Kf = Kd.float()


def torch_step():
    for p in (xs, ys, zs):
        p.grad = None
    loss = 0.5 * R.composition(xs, ys, zs, Kf)
    loss.backward()
    return loss


for _ in range(5):
    tl = torch_step()
torch.cuda.synchronize()
times = []
for _ in range(a.iters):
    e0.record()
    torch_step()
    e1.record()
    torch.cuda.synchronize()
    times.append(1000.0 * e0.elapsed_time(e1))
print("stock torch fp32 composition: %.1f us per forward + backward (median of %d, events around the call); weighted loss %.6f; d_disp_t "
      "max |difference| / max %.2e" % (median(times), a.iters, float(tl), float((xs.grad - x.grad).abs().max() / xs.grad.abs().max())))
