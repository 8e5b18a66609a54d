"""TEST INFRASTRUCTURE: the definition of the voxels' moments and their adjoint (include/mcav_depth.h: mcav_pillar_moments,
mcav_pillar_moments_bwd; pseudo_lidar.pillar_moments, pillar_moments_backward) in numpy, and the stock formulation of the layer they serve
-- F.linear -> BatchNorm1d(train) -> relu -> max -- in float64 torch, which the fold of the moments is held against
(tests/test_pfn_stats_cpu.py).

    P        min(offsets[B], capacity), never negative; n[p] = clamp(num_points[p], 0, N); the used slots are (p < P, k < n[p])
    moments  float64 [2 + C + C C]: rows = P N, used = sum n[p], s[c] = sum x[p, k, c], M[c][c'] = sum x[p, k, c] x[p, k, c'] over the used
             slots.  A term is exact in float64; the reference sums are math.fsum's, the correctly rounded sums of the exact terms
    adjoint  d_voxels[p, k, c] = float32(g[c] + sum_c' (H[c][c'] + H[c'][c]) x[p, k, c']) in the used slots, +0.0 elsewhere
"""
import math

import numpy as np

import pfn_ref as R

F = np.float32


def size(C):
    return 2 + C + C * C


def used_mask(num_points, P, N):
    n = np.clip(np.asarray(num_points[:P], np.int64), 0, N)
    return np.arange(N)[None, :] < n[:, None], n


def _sum(v):
    """the correctly rounded sum where there is one; NaN / infinities as float64 addition gives them"""
    if np.isfinite(v).all():
        return math.fsum(v.tolist())
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.sum(v))


def moments(voxels, num_points, offsets, capacity=None):
    """-> dict(moments float64 [2 + C + C C], abs: the sums of the terms' magnitudes in the same layout (0 for rows and used),
    terms: the number of used slots)"""
    vox = np.asarray(voxels, F)
    cap = len(vox) if capacity is None else capacity
    P = R.live_pillars(offsets, min(cap, len(vox)))
    N, C = vox.shape[1:]
    used, n = used_mask(num_points, P, N)
    x = vox[:P][used].astype(np.float64)                     # [used, C]
    out, mag = np.zeros(size(C)), np.zeros(size(C))
    out[0], out[1] = P * N, int(n.sum())
    for c in range(C):
        out[2 + c], mag[2 + c] = _sum(x[:, c]), _sum(np.abs(x[:, c]))
        for d in range(c, C):
            with np.errstate(invalid="ignore", over="ignore"):
                t = x[:, c] * x[:, d]                        # exact: 24 + 24 bits
            for i, j in ((c, d), (d, c)):
                out[2 + C + i * C + j], mag[2 + C + i * C + j] = _sum(t), _sum(np.abs(t))
    return dict(moments=out, abs=mag, terms=int(n.sum()))


def moments_bound(want):
    """float64 summation of n terms in any order: n 2^-53 sum |terms|"""
    return want["terms"] * 2.0 ** -53 * want["abs"]


def check_moments(got, want, what=""):
    """got: float64 [2 + C + C C].  rows and used exact, M symmetric in its bits, the sums within moments_bound; non-finite by class"""
    got = np.asarray(got)
    ref, mag = want["moments"], want["abs"]
    assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape)
    C = int(round((-1 + math.sqrt(1 + 4 * (len(ref) - 2))) / 2))
    assert got[0] == ref[0] and got[1] == ref[1], (what, got[:2], ref[:2])
    M = got[2 + C:].reshape(C, C)
    assert np.array_equal(M.view(np.uint64), M.T.copy().view(np.uint64)) or np.isnan(M).any(), (what, "M is not symmetric in its bits")
    assert np.array_equal(np.isnan(M), np.isnan(M.T))
    fin = np.isfinite(ref) & np.isfinite(mag)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaNs elsewhere", got, ref)
    assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]), (what, "infinities")
    err, bound = np.abs(got[fin] - ref[fin]), moments_bound(want)[fin]
    print("%s: moments max err / bound %.3g" % (what, float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0))
    assert (err <= bound).all(), "%s: off by %g where %g is allowed" % (what, (err - bound).max(), bound[np.argmax(err - bound)])


def moments_backward(voxels, num_points, offsets, g, H, capacity=None):
    """-> dict(d_voxels float32 [capacity, N, C], d_voxels64 before the rounding, abs: |g| + sum |H + H^T| |x|, used [capacity, N, C] bool)"""
    vox = np.asarray(voxels, F)
    cap = len(vox) if capacity is None else capacity
    P = R.live_pillars(offsets, min(cap, len(vox)))
    N, C = vox.shape[1:]
    used, _ = used_mask(num_points, P, N)
    g, H = np.asarray(g, np.float64), np.asarray(H, np.float64).reshape(C, C)
    G = H + H.T
    x = np.where(used[:, :, None], vox[:P], F(0)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.where(used[:, :, None], g[None, None, :] + x @ G.T, 0.0)
        mag = np.where(used[:, :, None], np.abs(g)[None, None, :] + np.abs(x) @ np.abs(G).T, 0.0)
    full = lambda v, dt: np.concatenate([v.astype(dt), np.zeros((cap - P, N, C), dt)])
    with np.errstate(over="ignore", invalid="ignore"):
        return dict(d_voxels=full(ref, F), d_voxels64=full(ref, np.float64), abs=full(mag, np.float64), used=full(used[:, :, None] & np.ones(C, bool), bool))


def backward_bound(want):
    """one float32 rounding of a float64 chain of C fmas behind g: 2^-24 |ref| + (C + 1) 2^-53 sum |terms|"""
    C = want["d_voxels"].shape[2]
    return 2.0 ** -24 * np.abs(want["d_voxels64"]) + (C + 1) * 2.0 ** -53 * want["abs"]


def check_backward(got, want, what="", extra=None):
    """got float32 [capacity, N, C]: within backward_bound (+ extra) in the used slots, +0.0 by bits elsewhere"""
    got = np.asarray(got)
    assert got.dtype == F and got.shape == want["d_voxels"].shape, (what, got.dtype, got.shape)
    used = want["used"]
    assert (got[~used].view(np.uint32) == 0).all(), (what, "not +0.0 in an unused slot or behind the last pillar")
    ref = want["d_voxels64"]
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaNs elsewhere")
    fin = used & np.isfinite(ref) & np.isfinite(want["abs"])
    bound = backward_bound(want) + (0.0 if extra is None else extra)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref)
    print("%s: d_voxels max err / bound %.3g over %d elements" % (what, float((err[fin] / np.maximum(bound[fin], 1e-300)).max()) if fin.any() else 0.0, fin.sum()))
    assert (err[fin] <= bound[fin]).all(), "%s: off by %g" % (what, (err[fin] - bound[fin]).max())


# ---------------------------------------------------------------------------------------------- the stock formulation, float64 torch
NEAR = 1e-5                                                  # pfn_bwd_ref.NEAR: the near-tie criterion


def padded_rows(vox, num_points, zc=None):
    """-> x [P, N, C or 10] float64 torch with the unused slots zero (second.pytorch's mask), the z - zc column appended to the used
    ones when zc is given; used [P, N] bool"""
    import torch
    P, N, _ = vox.shape
    n = torch.from_numpy(np.asarray(num_points, np.int64)).clamp(0, N)
    used = torch.arange(N)[None, :] < n[:, None]
    x = vox
    if zc is not None:
        x = torch.cat([x, x[:, :, 2:3] - zc], dim=2)
    return x * used[:, :, None], used


def stock(vox, num_points, weight, gamma, beta, eps, running_mean, running_var, momentum=0.1, zc=None):
    """F.linear -> BatchNorm1d(train) over all P N rows -> relu -> max over the slots, float64 torch with the graph behind it.
    vox [P, N, C] (a leaf or not), weight [C_out, C or 10], gamma, beta: torch float64.  -> dict(features [P, C_out], near [P, C_out]
    (the two best competitors within NEAR relative, the best positive), norm: the BatchNorm1d after the step)"""
    import torch
    x, used = padded_rows(vox, num_points, zc)
    P, N, _ = x.shape
    norm = torch.nn.BatchNorm1d(weight.shape[0], eps=eps, momentum=momentum).double()
    with torch.no_grad():
        norm.running_mean.copy_(running_mean)
        norm.running_var.copy_(running_var)
    norm.train()
    y = torch.nn.functional.linear(x, weight).reshape(P * N, -1)
    y = torch.nn.functional.batch_norm(y, norm.running_mean, norm.running_var, gamma, beta, True,
                                       _factor(norm, momentum), eps).reshape(P, N, -1)
    act = torch.relu(y)
    feat = act.max(dim=1).values
    return dict(features=feat, near=near_ties(act.detach(), used), norm=norm)


def _factor(norm, momentum):
    norm.num_batches_tracked += 1
    return 1.0 / float(norm.num_batches_tracked) if momentum is None else momentum


def near_ties(act, used):
    """act [P, N, C_out], used [P, N]: the competitors are the used slots and the padding term once (its copies in the unused slots are
    one value), as pfn_bwd_ref.torch_autograd has them -> near [P, C_out]"""
    import torch
    P, N, _ = act.shape
    first_unused = used.long().sum(dim=1).clamp(max=N - 1)                                  # a padding slot where there is one
    pad = torch.where((used.sum(dim=1) < N)[:, None], act[torch.arange(P), first_unused], torch.full_like(act[:, 0], -1.0))
    comp = torch.cat([torch.where(used[:, :, None], act, torch.full_like(act, -1.0)), pad[:, None, :]], dim=1)
    top = torch.topk(comp, 2, dim=1).values
    best, second = top[:, 0], top[:, 1]
    return (best > 0) & (best - second <= NEAR * best)
