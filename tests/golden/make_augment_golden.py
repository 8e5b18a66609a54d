#!/usr/bin/env python3
"""Generate tests/golden/augment.npz: a few seeded frames, augmentation records and what Pillow makes of them.

Run from the repo root:   python tests/golden/make_augment_golden.py
Pillow is the oracle: Image.transpose(FLIP_LEFT_RIGHT) before resize((w, h), BILINEAR) as monodepth2 does, then ImageEnhance.Brightness /
Contrast / Color and torchvision's F_pil.adjust_hue (restated below with PIL and numpy: torchvision is not a dependency) in the drawn
order.  The fixture pins those bytes, so the GPU tests check the kernels against them wherever another Pillow is installed.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = np.dtype([("flags", "<i4"), ("order", "u1", (4,)), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                   ("hue_shift", "<i4")])                   # include/mcav_depth.h: mcav_augment_record
FLIP, COLOUR = 1, 2


def adjust_hue(img, hue_factor):
    """torchvision.transforms._functional_pil.adjust_hue."""
    from PIL import Image
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h += np.int8(hue_factor * 255).view(np.uint8)        # over/underflows, as torchvision intends
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert(img.mode)


def pil_augment(src, h, w, flip, order, factors, hue_factor):
    """src uint8 [H0, W0, 3] -> (plain, augmented) uint8 [h, w, 3] through Pillow.  order: operation ids (0 brightness, 1 contrast,
    2 saturation, 3 hue, others skipped) or None for no colour; factors: (brightness, contrast, saturation) as Python floats."""
    from PIL import Image, ImageEnhance
    img = Image.fromarray(src)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    img = img.resize((w, h), Image.BILINEAR)
    plain = np.asarray(img).copy()
    for op in (order if order is not None else []):
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(factors[0])
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(factors[1])
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(factors[2])
        elif op == 3:
            img = adjust_hue(img, hue_factor)
    return plain, np.asarray(img).copy()


def main():
    rng = np.random.RandomState(20261016)
    H0, W0, h, w = 47, 157, 24, 80
    n = 6
    base = rng.randint(0, 256, (n, H0, W0, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H0, 0:W0]
    grad = np.stack([xx * 255 // (W0 - 1), yy * 255 // (H0 - 1), (xx + yy) % 256], -1).astype(np.uint8)
    frames = np.where(rng.rand(n, H0, W0, 1) < 0.5, base, grad[None]).astype(np.uint8)        # noise over smooth ramps
    recs = np.zeros(n, RECORD)
    hue_factor = np.array([0.1, -0.1, 0.5, -0.5, 0.03, 0.0])
    orders = [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1), (0, 1, 2, 3), (0, 1, 2, 3)]
    recs["flags"] = [FLIP | COLOUR, COLOUR, FLIP | COLOUR, COLOUR, FLIP, 0]
    recs["order"] = orders
    recs["brightness"] = np.float32([0.8, 1.2, 0.93, 1.17, 1.0, 1.0])
    recs["contrast"] = np.float32([1.2, 0.8, 1.11, 0.86, 1.0, 1.0])
    recs["saturation"] = np.float32([0.8, 1.2, 1.04, 0.81, 1.0, 1.0])
    recs["hue_shift"] = [int(np.trunc(x * 255.0)) % 256 for x in hue_factor]
    plain, aug = [], []
    for f, r, hf in zip(frames, recs, hue_factor):
        order = [int(o) for o in r["order"]] if r["flags"] & COLOUR else None
        factors = (float(r["brightness"]), float(r["contrast"]), float(r["saturation"]))
        p, a = pil_augment(f, h, w, bool(r["flags"] & FLIP), order, factors, float(hf))
        plain.append(p)
        aug.append(a)
    np.savez_compressed(os.path.join(HERE, "augment.npz"), frames=frames, records=recs.view(np.uint8).reshape(n, RECORD.itemsize),
                        hue_factor=hue_factor, size=np.array([h, w]), plain=np.stack(plain), aug=np.stack(aug))


if __name__ == "__main__":
    main()
