"""TEST INFRASTRUCTURE: the definition of the pillar feature net and its scatter to a bird's-eye-view pseudo-image (include/mcav_depth.h:
mcav_pillar_pseudo_image, pseudo_lidar.PillarFeatureNet) in numpy, one rounding per operation.

    voxels [capacity, N, C] float32, coords [capacity, 4] int32 = (b, 0, iy, ix), num_points [capacity] int32, offsets int32 [B + 1], as
    pillar_ref.pillarize leaves them; P = min(offsets[B], capacity); weight [C_out, C], bias [C_out], bias_pad [C_out] float32.
    pre      acc = bias[o]; acc = fma32(voxels[p, k, c], weight[o, c], acc) for c = 0 .. C - 1 in ascending order
    act      acc > 0 ? acc : (acc is a NaN ? acc : +0.0)
    feat     the NaN-propagating maximum of act over the slots k < n = clamp(num_points[p], 0, N); act(bias_pad[o]) joins it if n < N
    canvas   [B, C_out, ny, nx]: feat[p] at (b, :, iy, ix) of every row p < P whose (b, iy, ix) lies inside, +0.0 elsewhere
    features [P, C_out]

fma32 is a correctly rounded float32 fused multiply-add without math.fma: the product of two float32 is exact in float64; the float64 sum
of it and the addend gets its TwoSum error term; where that is non-zero the sum is moved to the neighbour with an odd last bit (round to
odd), which makes the final rounding to float32 the rounding of the exact value.  tests/test_pfn_cpu.py holds it against C's fmaf.
"""
import numpy as np

F = np.float32


def fma32(a, b, c):
    """float32(a * b + c) with one rounding, elementwise with broadcasting"""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    shape = np.broadcast(a, b, c).shape
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.atleast_1d(a * b)                             # exact: 24 + 24 bits
        s = p + c
        t = s - p                                            # TwoSum (Knuth): s + err = p + c exactly
        err = (p - (s - t)) + (c - t)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
        bits = np.ascontiguousarray(s).view(np.int64)
        away = (err > 0.0) == (s > 0.0)                      # the exact value lies further from zero than s
        step = np.where(inexact & ((bits & 1) == 0), np.where(away, 1, -1), 0).astype(np.int64)
        return (bits + step).view(np.float64).astype(F).reshape(shape)


def act(v):
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, v, np.where(np.isnan(v), v, F(0.0))).astype(F)


def live_pillars(offsets, capacity):
    return max(min(int(offsets[-1]), int(capacity)), 0)


def features(voxels, num_points, P, weight, bias, bias_pad):
    """-> feat [P, C_out] float32"""
    vox = np.asarray(voxels, F)[:P]
    weight, bias, bias_pad = np.asarray(weight, F), np.asarray(bias, F), np.asarray(bias_pad, F)
    N, C = vox.shape[1:]
    C_out = weight.shape[0]
    assert weight.shape == (C_out, C) and bias.shape == bias_pad.shape == (C_out,)
    acc = np.broadcast_to(bias, (P, N, C_out)).astype(F)
    for c in range(C):
        acc = fma32(vox[:, :, c, None], weight[None, None, :, c], acc)
    a = act(acc)
    n = np.clip(np.asarray(num_points[:P], np.int64), 0, N)
    used = np.arange(N)[None, :] < n[:, None]
    a = np.where(used[:, :, None], a, act(bias_pad)[None, None, :])          # a padding slot holds what joins the maximum for n < N
    return np.max(a, axis=1).astype(F) if P else np.zeros((0, C_out), F)     # np.max propagates a NaN


def inside(coords, B, ny, nx):
    c = np.asarray(coords, np.int64)
    return (c[:, 0] >= 0) & (c[:, 0] < B) & (c[:, 2] >= 0) & (c[:, 2] < ny) & (c[:, 3] >= 0) & (c[:, 3] < nx)


def pseudo_image(voxels, coords, num_points, offsets, nx, ny, weight, bias, bias_pad=None, capacity=None):
    """-> dict(canvas [B, C_out, ny, nx] float32, features [P, C_out] float32); bias_pad=None: bias_pad = bias"""
    bias_pad = bias if bias_pad is None else bias_pad
    B = len(offsets) - 1
    P = live_pillars(offsets, len(voxels) if capacity is None else min(capacity, len(voxels)))
    feat = features(voxels, num_points, P, weight, bias, bias_pad)
    canvas = np.zeros((B, feat.shape[1], ny, nx), F)
    c = np.asarray(coords[:P], np.int64)
    ok = inside(c, B, ny, nx)
    canvas[c[ok, 0], :, c[ok, 2], c[ok, 3]] = feat[ok]
    return dict(canvas=canvas, features=feat)


def fold_batchnorm(w, gamma, beta, mean, var, eps=1e-3, linear_bias=None, zc=None):
    """The evaluation-mode BatchNorm1d behind a Linear folded into it, in float64, rounded once: -> weight, bias, bias_pad (float32).
    A 10-column weight (OpenPCDet's z - zc column) needs zc and folds to 9 columns."""
    w, gamma, beta, mean, var = (np.asarray(v, np.float64) for v in (w, gamma, beta, mean, var))
    lb = np.zeros_like(beta) if linear_bias is None else np.asarray(linear_bias, np.float64)
    scale = gamma / np.sqrt(var + eps)
    wf = w * scale[:, None]
    bf = beta + (lb - mean) * scale
    if w.shape[1] == 10:
        w9 = wf[:, :9].copy()
        w9[:, 2] += wf[:, 9]
        return w9.astype(F), (bf - wf[:, 9] * zc).astype(F), bf.astype(F)
    return wf.astype(F), bf.astype(F), bf.astype(F)
