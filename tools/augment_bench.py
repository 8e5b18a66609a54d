#!/usr/bin/env python3
"""Times the training-time augmentation on the GPU (include/mcav_depth.h: mcav_image_preprocess_augment) against the plain transform
(mcav_image_preprocess) for one batch of 12 triplets, 36 frames from 375x1242 to 192x640, every sample coloured and flipped, and Pillow's
host time for the same flip and colour jitter on one core.

    python tools/augment_bench.py [--iters 50] [--pillow-frames 36]

Prints one JSON line: microseconds per launch (device events around `iters` back-to-back launches after a warm-up) and milliseconds of
Pillow per batch.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unsupervised-pseuso-lidar_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--pillow-frames", type=int, default=36)
    args = ap.parse_args()
    import torch
    from dataloaders import AUG_COLOUR, AUG_FLIP, Augmentation, GpuImageTransform
    from make_augment_golden import pil_augment
    assert torch.cuda.is_available(), "augment_bench needs the GPU"
    H0, W0, h, w, n = 375, 1242, 192, 640, 36
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, (n, H0, W0, 3)).astype(np.uint8)
    a = Augmentation(p_color=1.0, p_flip=1.0, seed=1)
    rec = a.draw(a.generator(0), n // 3)
    rec = np.concatenate([rec] * 3)
    assert ((rec["flags"] & (AUG_FLIP | AUG_COLOUR)) == AUG_FLIP | AUG_COLOUR).all()
    t = GpuImageTransform(h, w, "cuda")
    x = torch.from_numpy(frames).cuda()
    # the records stay on the device for the timed loop: this measures the kernels, not the 864-byte copy
    from mcav import lib as L
    import ctypes
    hb, hk, hks = t._axis(W0, w)
    vb, vk, vks = t._axis(H0, h)
    dev_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    lib = L.lib()
    ws = L.workspace(lib.mcav_image_augment_workspace_bytes(n, H0, h, w), x.device, "augment")
    plain = torch.empty((n, 3, h, w), device="cuda")
    aug = torch.empty_like(plain)
    mean, std = (ctypes.c_float * 3)(*t.MEAN), (ctypes.c_float * 3)(*t.STD)

    def run_aug():
        L.check(lib.mcav_image_preprocess_augment(L.ptr(x), n, H0, W0, h, w, L.ptr(hb), L.ptr(hk), hks, L.ptr(vb), L.ptr(vk), vks, mean, std,
                                                  L.ptr(dev_rec), L.ptr(plain), L.ptr(aug), L.ptr(ws), ws.numel(), L.stream()), "augment")

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    res = {}
    for rep in range(2):                                    # alternate, twice: the spread shows in the two numbers
        res.setdefault("plain_us", []).append(round(timed(lambda: t(x)), 1))
        res.setdefault("augment_us", []).append(round(timed(run_aug), 1))
    k = args.pillow_frames
    from PIL import Image
    small = [np.asarray(Image.fromarray(f).resize((w, h), Image.BILINEAR)) for f in frames[:k]]
    t0 = time.perf_counter()
    for f, r in zip(small, rec[:k]):
        pil_augment(f, h, w, True, [int(o) for o in r["order"]], (float(r["brightness"]), float(r["contrast"]), float(r["saturation"])),
                    ((int(r["hue_shift"]) + 128) % 256 - 128) / 255.0)
    res["pillow_flip_jitter_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3 * n / k, 1)
    res.update(frames=n, src=[H0, W0], dst=[h, w], iters=args.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
