"""The definition of the training-time augmentation (include/mcav_depth.h: mcav_image_preprocess_augment), restated in numpy.

monodepth2 draws one record per sample: a horizontal flip, and torchvision's ColorJitter (brightness, contrast, saturation, hue in a random
order) on PIL images.  R is the Pillow-resized uint8 frame; with the flip it is mirrored; with colour, each operation reads and writes uint8
exactly as Pillow: convert("L"), ImagingBlend (ImageEnhance.Brightness / Contrast / Color) and Pillow's RGB <-> HSV conversions behind
torchvision's F_pil.adjust_hue.  numpy's float32 and float64 operations round one at a time, which is what makes this the bit-exact target.
tests/test_augment_cpu.py checks it against the installed Pillow; the GPU tests check the kernels against it."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE, NONE = 0, 1, 2, 3, 255
FLIP, COLOUR = 1, 2
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def luma(rgb):
    """convert("L") of uint8 [..., 3] -> int64 [...]."""
    x = rgb.astype(np.int64)
    return (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 0x8000) >> 16


def blend(a, b, alpha):
    """ImagingBlend per byte: t = a + alpha * (b - a) in float32, rounded after each operation; truncated, clipped first when alpha is
    outside [0, 1]."""
    alpha = np.float32(alpha)
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    t = a.astype(np.float32) + alpha * (b - a).astype(np.float32)
    if 0.0 <= alpha <= 1.0:
        return t.astype(np.int64)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64)))


def brightness(R, f):
    return blend(np.zeros_like(R), R, f).astype(np.uint8)


def saturation(R, f):
    return blend(np.repeat(luma(R)[..., None], 3, -1), R, f).astype(np.uint8)


def contrast_mean(R):
    """int(S / n + 0.5) with S the exact integer sum of L over the frame (ImageStat's mean, float64)."""
    S = int(luma(R).sum())
    n = R.shape[0] * R.shape[1]
    return int(S / n + 0.5)


def contrast(R, f):
    return blend(np.full(R.shape, contrast_mean(R), np.int64), R, f).astype(np.uint8)


def rgb_to_hsv(rgb):
    """Pillow's rgb2hsv_row: uint8 [..., 3] -> uint8 [..., 3]."""
    x = rgb.astype(np.int64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = (maxc - minc).astype(np.float32)
    cr = np.where(grey, np.float32(1), cr)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = cr / np.maximum(maxc, 1).astype(np.float32)
    rc = (maxc - r).astype(np.float32) / cr
    gc = (maxc - g).astype(np.float32) / cr
    bc = (maxc - b).astype(np.float32) / cr
    h_r = bc - gc                                                                        # float32
    h_g = ((2.0 + rc.astype(np.float64)) - bc.astype(np.float64)).astype(np.float32)     # double, stored to float
    h_b = ((4.0 + gc.astype(np.float64)) - rc.astype(np.float64)).astype(np.float32)
    h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1)
    return out.astype(np.uint8)


def _round(x):
    """C round() of non-negative doubles (half away from zero); x - floor(x) is exact."""
    f = np.floor(x)
    return f.astype(np.int64) + (x - f >= 0.5)


def hsv_to_rgb(hsv):
    """Pillow's hsv2rgb: uint8 [..., 3] -> uint8 [..., 3]."""
    x = hsv.astype(np.int64)
    h, s, v = x[..., 0], x[..., 1], x[..., 2]
    h6 = h.astype(np.float32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = (h6 - i.astype(np.float32).astype(np.float64)).astype(np.float32)
    fs = (s.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32)
    vd = v.astype(np.float32).astype(np.float64)
    p = np.clip(_round(vd * (1.0 - fs.astype(np.float64))), 0, 255)
    q = np.clip(_round(vd * (1.0 - (fs * f).astype(np.float64))), 0, 255)
    t = np.clip(_round(vd * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64)))), 0, 255)
    sector = i % 6
    r = np.choose(sector, [v, q, p, p, t, v])
    g = np.choose(sector, [t, v, v, q, p, p])
    b = np.choose(sector, [p, p, t, v, v, q])
    grey = s == 0
    out = np.stack([np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)], -1)
    return out.astype(np.uint8)


def hue_shift_of(hue_factor):
    """torchvision: np_h += np.int8(hue_factor * 255).view(np.uint8) -> trunc(h * 255) mod 256."""
    return int(np.trunc(float(hue_factor) * 255.0)) % 256


def hue(R, shift):
    hsv = rgb_to_hsv(R)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + int(shift)) % 256
    return hsv_to_rgb(hsv)


def apply_op(R, op, rec):
    if op == BRIGHTNESS:
        return brightness(R, rec["brightness"])
    if op == CONTRAST:
        return contrast(R, rec["contrast"])
    if op == SATURATION:
        return saturation(R, rec["saturation"])
    if op == HUE:
        return hue(R, int(rec["hue_shift"]) & 255)
    return R


def augment_bytes(R, rec):
    """R: the resized uint8 frame [h, w, 3]; rec: one record (flags, order, brightness, contrast, saturation, hue_shift).
    -> (plain bytes, augmented bytes)."""
    if int(rec["flags"]) & FLIP:
        R = R[:, ::-1]
    R = np.ascontiguousarray(R)
    plain = R
    if int(rec["flags"]) & COLOUR:
        for op in rec["order"]:
            R = apply_op(R, int(op), rec)
    return plain, R


def normalise(R):
    """uint8 [h, w, 3] -> float32 [3, h, w] = (R / 255 - mean) / std, as the kernels."""
    x = R.astype(np.float32) / np.float32(255.0)
    return ((x - MEAN) / STD).transpose(2, 0, 1).copy()


def pil_resize(img, h, w):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR))


def expected(frames, records, h, w):
    """frames: uint8 [N, H0, W0, 3]; records: N records -> (plain, aug) float32 [N, 3, h, w]."""
    plain, aug = [], []
    for f, r in zip(frames, records):
        p, a = augment_bytes(pil_resize(f, h, w), r)
        plain.append(normalise(p))
        aug.append(normalise(a))
    return np.stack(plain), np.stack(aug)
