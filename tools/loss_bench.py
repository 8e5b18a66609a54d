#!/usr/bin/env python3
"""Times the fused loss stage alone (forward call = forward + backward of the loss in ONE launch) at bench.py's shapes.
usage: python tools/loss_bench.py [--ssim] [--min-reprojection] [--automask] [--stereo] [--edge-smooth] [--batch 12 --height 192 --width 640] [--iters 200]
--edge-smooth: Losses(edge_aware_smoothness=True) -- the fused kernel runs with MCAV_WL_NO_SMOOTH, and the edge-aware smoothness launches
(mcav_edge_smooth_fwd / _bwd, scale 0) are timed per dispatch as well.
--stereo: Losses(stereo=True) (mcav_warp_loss_stereo_fwd_bwd) with a stereo frame and baselines of +-0.54 m."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd")]
import torch  # noqa: E402
from losses import Losses  # noqa: E402
from oracle.step import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ssim", action="store_true")
ap.add_argument("--min-reprojection", action="store_true")
ap.add_argument("--automask", action="store_true")
ap.add_argument("--edge-smooth", action="store_true")
ap.add_argument("--stereo", action="store_true")
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--height", type=int, default=192)
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--iters", type=int, default=200)
a = ap.parse_args()
dev = "cuda"
B, H, W = a.batch, a.height, a.width
s = synthetic_batch(B, H, W, seed=3)
tgt, refs, K = s["tgt"].to(dev), [r.to(dev) for r in s["ref_imgs"]], s["intrinsics"].to(dev)
g = torch.Generator().manual_seed(4)
# disparities as a depth network gives them: smooth maps around 0.5 (white-noise disparities scatter the gathers over the whole image and
# take the kernel twice as long: 110 us instead of 54 at 12 x 192 x 640)


def smooth_disp():
    z = torch.randn(B, 1, H // 8 + 2, W // 8 + 2, generator=g)
    z = torch.nn.functional.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)
    return torch.sigmoid(0.3 * z).contiguous().to(dev)


dt, dr = smooth_disp(), smooth_disp()
poses = (0.01 * torch.randn(B, 2, 6, generator=g)).to(dev)
crit = Losses(ssim=a.ssim, min_reprojection=a.min_reprojection, automask=a.automask, edge_aware_smoothness=a.edge_smooth, stereo=a.stereo)
kw = {}
if a.stereo:          # the stereo frame: the target a pixel over (a right view's order of disparity); flipped samples every other one
    kw = dict(stereo=torch.roll(tgt, 1, dims=3).contiguous(), stereo_baseline=torch.tensor([0.54, -0.54] * B, device=dev)[:B].contiguous())
from mcav import nn as N  # noqa: E402

with torch.no_grad():
    for _ in range(20):
        out = crit.forward(tgt, refs, [[dt], [dr]], poses, K, None, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = crit.forward(tgt, refs, [[dt], [dr]], poses, K, None, **kw)
    e1.record()
    torch.cuda.synchronize()
    call_us = 1000.0 * e0.elapsed_time(e1) / a.iters
    # the kernel's own duration: per-dispatch HIP events (csrc/kernel_timer.h), as bench.py's roofline_warp
    N.kernel_timer_begin()
    for _ in range(50):
        out = crit.forward(tgt, refs, [[dt], [dr]], poses, K, None, **kw)
    torch.cuda.synchronize()
    durs = N.kernel_timer_end()
    if a.edge_smooth:                   # a call is [fused kernel, edge-aware smoothness forward]
        durs = durs[0::2]
    durs = sorted(durs)
us = 1000.0 * durs[len(durs) // 2]
print("loss stage %s %dx%dx%d: kernel %.1f us (median of %d dispatches, min %.1f) = %.3f of the 8 TB/s HBM roofline at 52 B/pixel; %.1f us per "
      "back-to-back call incl. the host; losses %s" % (("SSIM+L1" if a.ssim else "L1") + (" min-reprojection" if a.min_reprojection else "") +
                                                       (" automask" if a.automask else "") + (" stereo" if a.stereo else ""), B, H, W, us, len(durs), 1000.0 * durs[0],
                                                       52.0 * B * H * W / (us * 1e-6) / 8e12, call_us, [round(float(x), 6) for x in out]))
if a.edge_smooth:
    # the edge-aware smoothness alone: forward + backward of scale 0, one dispatch each (only the mcav launches are timed)
    x = dt.clone().requires_grad_()
    for _ in range(10):
        crit.edge_aware_smooth_loss(x, tgt).backward()
    torch.cuda.synchronize()
    N.kernel_timer_begin()
    for _ in range(50):
        crit.edge_aware_smooth_loss(x, tgt).backward()
    torch.cuda.synchronize()
    d = N.kernel_timer_end()
    assert len(d) == 100, len(d)
    fwd, bwd = sorted(d[0::2]), sorted(d[1::2])
    fu, bu = 1000.0 * fwd[len(fwd) // 2], 1000.0 * bwd[len(bwd) // 2]
    print("edge-aware smoothness %dx%dx%d: forward %.1f us (min %.1f), backward %.1f us (min %.1f), %.1f us per step; fused kernel %.1f us "
          "(median of 50 dispatches each; 16 B/pixel read forward, 20 B/pixel backward)" % (B, H, W, fu, 1000.0 * fwd[0], bu, 1000.0 * bwd[0],
                                                                                           fu + bu, us))
