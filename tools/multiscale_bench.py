#!/usr/bin/env python3
"""Times multi-scale training of DispResNet: the whole step and the loss stage alone, with the coarse scales going through the fused depth
pyramid (--fused: mcav_depth_pyramid_fwd / _bwd, one launch each) or through the per-scale composition (disp_to_depth + bilinear resize per
scale, pass and direction).  Prints ONE JSON line.
usage: python tools/multiscale_bench.py [--fused] [--upsample depth|disparity] [--scales 4] [--ssim] [--min-reprojection] [--automask]
       [--edge-smooth] [--batch 12 --height 192 --width 640] [--iters 50] [--warmup 10]
--scales 1 is the single-scale step (what turning multi-scale on costs is the difference)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-pseuso-lidar_amd")]
import torch  # noqa: E402
from losses import Losses  # noqa: E402
from mcav import lib as L  # noqa: E402
from oracle.step import synthetic_batch  # noqa: E402

PYRAMID_ENTRIES = ("mcav_depth_pyramid_fwd", "mcav_depth_pyramid_bwd", "mcav_disp_to_depth", "mcav_disp_to_depth_bwd",
                   "mcav_resize_bilinear_fwd", "mcav_resize_bilinear_bwd")


def pyramid_bytes(B, H, W, scales):
    """Algorithmic bytes of one pyramid launch: the coarse maps of both passes read plus nlevels * 2B * H * W * 4 written (forward); the
    backward reads the same amount (and the stored depths once more in disparity order)."""
    coarse = sum(2 * B * (H >> s) * (W >> s) * 4 for s in range(1, scales))
    return coarse + (scales - 1) * 2 * B * H * W * 4


def count_calls(fn):
    """Calls of the depth / resize / pyramid entry points during fn() (every call is one launch)."""
    h, counts, saved = L.lib(), {}, {}
    for name in PYRAMID_ENTRIES:
        saved[name] = getattr(h, name)

        def wrapped(*args, _n=name):
            counts[_n] = counts.get(_n, 0) + 1
            return saved[_n](*args)
        setattr(h, name, wrapped)
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(h, name, f)
    return counts


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--upsample", choices=("depth", "disparity"), default="depth")
    ap.add_argument("--scales", type=int, default=4)
    ap.add_argument("--ssim", action="store_true")
    ap.add_argument("--min-reprojection", action="store_true")
    ap.add_argument("--automask", action="store_true")
    ap.add_argument("--edge-smooth", action="store_true")
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiscale_bench: needs the MI355X (there is no CPU path)")
    from mcav import tape  # noqa: F401  (registers the resize entry points)
    from mcav.optim import FusedAdam
    from mcav.streams import Branch
    from models.depth.resnet_dispnet import DispResNet
    from models.pose.pose_net import PoseNet
    dev = "cuda"
    B, H, W, n = a.batch, a.height, a.width, a.scales
    torch.manual_seed(3)
    depth, pose = DispResNet(scales=n).to(dev).train(), PoseNet()
    pose.init_weights()
    pose.to(dev).train()
    s = synthetic_batch(B, H, W, seed=3)
    tgt, refs, K = s["tgt"].to(dev), [r.to(dev) for r in s["ref_imgs"]], s["intrinsics"].to(dev)
    crit = Losses(ssim=a.ssim, min_reprojection=a.min_reprojection, automask=a.automask, edge_aware_smoothness=a.edge_smooth,
                  multiscale_upsample=a.upsample, fused_pyramid=a.fused)
    opt = FusedAdam(list(depth.parameters()) + list(pose.parameters()), 1e-4)
    branch = Branch()
    last = {}

    def step():
        opt.zero_grad()
        poses = branch.fork(pose, tgt, refs)
        disps = list(depth.forward_pair(tgt, refs[0]))
        poses = branch.join(poses)
        loss = crit.forward(tgt, refs, disps, poses, K, None)
        sum(loss).backward()
        opt.step()
        last["loss"] = loss

    step_ms = timed(step, a.warmup, a.iters)
    losses = [float(x.detach()) for x in last["loss"]]
    # the loss stage alone: forward + backward from the network's own (detached) outputs; the two maps of a scale stay one stacked buffer
    with torch.no_grad():
        dt, dr = depth.forward_pair(tgt, refs[0])
        poses0 = pose(tgt, refs)
    dt, dr = [d.requires_grad_() for d in dt], [d.requires_grad_() for d in dr]
    poses0.requires_grad_()

    def loss_stage():
        for t in dt + dr + [poses0]:
            t.grad = None
        sum(crit.forward(tgt, refs, [dt, dr], poses0, K, None)).backward()

    loss_ms = timed(loss_stage, a.warmup, a.iters)
    calls = count_calls(loss_stage)
    torch.cuda.synchronize()
    nbytes = pyramid_bytes(B, H, W, n) if n > 1 else 0
    print(json.dumps({"tool": "multiscale_bench", "batch": B, "height": H, "width": W, "scales": n, "fused": bool(a.fused), "upsample": a.upsample,
                      "ssim": bool(a.ssim), "min_reprojection": bool(a.min_reprojection), "automask": bool(a.automask),
                      "edge_smooth": bool(a.edge_smooth), "step_ms": round(step_ms, 4), "loss_stage_ms": round(loss_ms, 4),
                      "pyramid_launches": sum(calls.values()), "pyramid_launches_by_entry": calls,
                      "pyramid_fwd_bytes": nbytes, "pyramid_bwd_bytes": nbytes, "losses": losses, "iters": a.iters}))


if __name__ == "__main__":
    main()
