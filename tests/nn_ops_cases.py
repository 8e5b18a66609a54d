"""Case lists and input builders shared by tests/test_nn_ops_cpu.py and tests/test_nn_ops_gpu.py (test infrastructure).

The shapes are the smallest that reach each code path of csrc/nn_ops.hip / csrc/aux_ops.hip; the comment beside a list says which.
Builders are deterministic (seeded per case) and return float32 CPU tensors: the kernels get them as they are, the references .double() them.
"""
import math

import numpy as np
import torch

F32 = torch.float32
EPS = float(np.float32(1e-5))          # the kernels take eps / momentum / Adam's scalars as C floats: the references get the same values
MOMENTUM = float(np.float32(0.1))


def gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


# ------------------------------------------------------------------------------------------------ mcav_bn_finalize
# mtiles <= 64: bn_finalize_kernel reads the slab itself, 32 slice lanes (31 / 32 / 33: on both sides of them).
# mtiles > 64: bn_partial_finalize_kernel, per_slice = max(8, ceil(mtiles / 128)), slices = ceil(mtiles / per_slice); the finisher's four
# lanes take slices sl, sl + 4, ... : eight at a time while sl + 28 < slices, then a tail.
#   65, 71 -> 9 slices (tail only); 257 -> 33 (one unrolled pass on lane 0..0 + tail); 1024 -> 128 (full passes); 1025 -> per_slice 9, 114.
FIN_MTILES = (1, 31, 32, 33, 64, 65, 71, 257, 1024, 1025)
FIN_WIDTHS = (16, 64, 96, 128, 2048)          # 96: ragged last 64-channel column; 2048: 32 ticket columns
FIN_ROWS = 2                                   # pixels per tile of the synthetic slabs


def fin_slices(mtiles):
    per = max(8, -(-mtiles // 128))
    return -(-mtiles // per)


assert [fin_slices(m) for m in (65, 71, 257, 1024, 1025)] == [9, 9, 33, 128, 114]


def fin_cases():
    """(mtiles, C, groups, running): every (mtiles, C) pair, groups and the presence of running statistics cycling through the pairs, and
    the full groups x running product at the widths 96 (ragged) and 64 for one tile count of each kernel form."""
    out = []
    for i, m in enumerate(FIN_MTILES):
        for j, C in enumerate(FIN_WIDTHS):
            out.append((m, C, 1 + (i + j) % 3, bool((i + j // 3) % 2)))
    for m in (33, 71, 257):
        for C in (96, 64):
            for groups in (1, 2, 3):
                for running in (False, True):
                    if (m, C, groups, running) not in out:
                        out.append((m, C, groups, running))
    return out


FIN_CASES = fin_cases()


def fin_build(mtiles, C, groups, rows=FIN_ROWS, seed=0):
    """A known x [groups, mtiles, rows, C] and the slab of its per-tile sums (sums taken in float64, stored as float32, as an fp32 epilogue
    with a short tile would leave them).  Channel statistics differ per group.  Special channels (where C allows):
      0: constant 1.5 (x^2 exact: variance exactly 0);  1: constant 0.1 ... (whichever of a few constants makes E[x^2] - mean^2 NEGATIVE
      through the rounding of the tile sums: the clamp);  2: mean / std = 1e3."""
    g = gen(mtiles, C, groups, rows, seed)
    mu = 0.7 + torch.randn(groups, 1, 1, C, generator=g)
    sd = 0.5 + torch.rand(groups, 1, 1, C, generator=g)
    x = (mu + sd * torch.randn(groups, mtiles, rows, C, generator=g)).float()
    x[..., 0] = 1.5
    if C > 2:
        x[..., 1] = negative_variance_constant(mtiles, rows)
        x[..., 2] = 1000.0 + torch.randn(groups, mtiles, rows, generator=g)
    xd = x.double()
    slab = torch.stack([xd.sum(2), (xd * xd).sum(2)], 2).float().reshape(groups * mtiles, 2, C).contiguous()
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).float()
    beta = (0.1 * torch.randn(C, generator=g)).float()
    rm = (0.3 * torch.randn(C, generator=g)).float()
    rv = (0.5 + torch.rand(C, generator=g)).float()
    return dict(x=x, slab=slab, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, count=float(mtiles * rows))


def negative_variance_constant(mtiles, rows):
    """A constant c whose float32 tile sums give E[x^2] - mean^2 < 0 in float64: rows * c^2 rounds DOWN to float32."""
    for c in (0.1, 0.3, 0.7, 1.1, 1.3, 0.9, 2.3):
        c32 = float(np.float32(c))
        s2 = float(np.float32(rows * c32 * c32))
        if s2 * mtiles / (mtiles * rows) - c32 * c32 < 0:
            return c32
    raise AssertionError("no constant with a negative raw variance")


# ------------------------------------------------------------------------------------------------ mcav_bn_apply / bn_bwd_*
# bn_bwd_reduce_kernel: a block owns per = ceil(pix / blocks) pixels, blocks = min(ceil(pix / 32), 1024); PL = 256 / (C / 4) pixel lanes
# (C >= 1024: one lane; C = 2048: two passes of the g0 loop); the 4-pixel unrolled loop runs when a block owns more than 3 PL pixels.
BN_WIDTHS = (4, 16, 64, 256, 1024, 2048)      # PL = 256, 64, 16, 4, 1, 1 (x 2 passes)
BN_PIX = (1, 31, 32, 33, 70, 1057)             # per group: one block short / full / two blocks, per = 24 (> 3 PL at C = 256), 34 blocks of 32


def bn_cases():
    """(C, pix per group, groups, relu, dres, dres_accumulate, accumulate)."""
    out = []
    k = 0
    for C in BN_WIDTHS:
        for pix in BN_PIX:
            out.append((C, pix, 1 + k % 3, k % 2 == 0, k % 4 < 2, k % 8 < 2, k % 3 == 1))
            k += 1
    out.append((4, 32769, 2, True, False, False, False))        # 1025 blocks wanted: capped at 1024, per = 33
    out.append((64, 51300, 2, True, True, True, True))          # per = 51 > 48 = 3 PL: the unrolled loop at the stem's width
    out.append((256, 70, 3, True, True, False, False))          # the unrolled loop with the mask, three groups
    out.append((64, 33, 3, False, True, True, True))
    return out


BN_CASES = bn_cases()
BN_WRAP = (64, 33000, 3)     # n4 = 99000 * 16 = 1 584 000 > 4096 * 256: the second trip starts at 1 048 576, group 2 at 1 056 000, inside it


def bn_build(C, pix, groups, seed=0):
    """x, dy, residual [groups * pix, C]; y_act (the activated output the mask is taken from) is built by the caller from the reference's
    forward, with exact +0.0 and -0.0 planted by plant_zeros().  Saved statistics are the exact ones of x, rounded to float32."""
    g = gen(C, pix, groups, seed, 77)
    n = groups * pix
    mu = 0.5 * torch.randn(groups, 1, C, generator=g)
    sd = 0.5 + torch.rand(groups, 1, C, generator=g)
    x = (mu + sd * torch.randn(groups, pix, C, generator=g)).float().reshape(n, C)
    dy = torch.randn(n, C, generator=g).float()
    res = torch.randn(n, C, generator=g).float()
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).float()
    beta = (0.1 * torch.randn(C, generator=g)).float()
    xd = x.double().reshape(groups, pix, C)
    mean = xd.mean(1)
    var = (xd * xd).mean(1) - mean * mean
    invstd = 1.0 / torch.sqrt(var.clamp_min(0) + EPS)
    return dict(x=x, dy=dy, res=res, gamma=gamma, beta=beta, mean=mean.float(), invstd=invstd.float(),
                dgamma0=torch.randn(C, generator=g).float(), dbeta0=torch.randn(C, generator=g).float(),
                dres0=torch.randn(n, C, generator=g).float())


def plant_zeros(y, seed=0):
    """In place: about 2 % of y becomes +0.0 and 2 % -0.0 (ties of the ReLU mask y > 0: both masked)."""
    g = gen(y.numel(), seed, 5)
    r = torch.rand(y.shape, generator=g)
    y[r < 0.02] = 0.0
    y[(r >= 0.02) & (r < 0.04)] = -0.0
    return y


# ------------------------------------------------------------------------------------------------ mcav_bn_eval_coeffs
# bn_eval_coeffs_kernel: one thread per channel, 64-thread blocks, any C > 0.  1, 4: one short block; 63 / 64 / 65: on both sides of the block edge;
# 512, 2048: the widest layers of ResNet-18 / ResNet-50 (8 and 32 blocks).
EVAL_C = (1, 4, 63, 64, 65, 512, 2048)
EVAL_EPS = tuple(float(np.float32(v)) for v in (1e-5, 1e-3))       # nn.BatchNorm2d's default, and one where eps decides at every small variance
EVAL_VARS = (0.0, 1e-12, 1e-6, 1.0, 1e6)                          # running_var: exactly 0 and far below eps (eps alone), around eps, 1, huge
# what a case fills its channels with: one running_var for all of them, `gamma` (zeros and negative values), `cancel` (|running_mean| up to 1e3
# against a small beta, and on every other channel a beta that ALMOST equals mean * scale: shift is what is left of the two), `mixed` (all of
# these, cycling across the channels with coprime periods)
EVAL_KINDS = tuple("var=%g" % v for v in EVAL_VARS) + ("gamma", "cancel", "mixed")
EVAL_CASES = [(C, kind, eps) for C in EVAL_C for kind in EVAL_KINDS for eps in EVAL_EPS]


def eval_build(C, kind, eps, seed=0):
    """gamma, beta, running_mean, running_var [C] float32 of one mcav_bn_eval_coeffs case (EVAL_KINDS)."""
    g = gen(C, EVAL_KINDS.index(kind), int(round(eps * 1e6)), seed, 21)
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).float()
    beta = (0.1 * torch.randn(C, generator=g)).float()
    rm = (0.3 * torch.randn(C, generator=g)).float()
    rv = (0.5 + torch.rand(C, generator=g)).float()
    big = (1e3 * (0.25 + 0.75 * torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)).float()
    small = (1e-3 * torch.randn(C, generator=g)).float()
    c = torch.arange(C)
    if kind.startswith("var="):
        rv[:] = float(kind[4:])
    if kind in ("gamma", "mixed"):
        gamma[c % 3 == 1] *= -1.0
        gamma[c % 7 == 0] = 0.0
        gamma[c % 7 == 3] = -0.0
    if kind == "mixed":
        rv = torch.tensor(EVAL_VARS, dtype=F32)[c % 5].clone()
    if kind in ("cancel", "mixed"):
        period = 2 if kind == "cancel" else 4
        far = c % period == 0
        rm[far], beta[far] = big[far], small[far]
        near = c % period == 1
        rm[near] = big[near]
        beta[near] = (rm[near].double() * gamma[near].double() / torch.sqrt(rv[near].double() + eps) * (1.0 + 1e-4 * torch.randn(int(near.sum()), generator=g).double())).float()
    return dict(gamma=gamma, beta=beta, running_mean=rm, running_var=rv)


# ------------------------------------------------------------------------------------------------ max-pool
POOL_HW =((1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (5, 4), (7, 9), (11, 14))
POOL_CASES = [(B, H, W, C) for (H, W) in POOL_HW for C in (4, 64) for B in (1, 3)]
POOL_WRAP = (1, 2049, 2049, 4)      # 1025 * 1025 outputs x one channel quad > 4096 * 256 (and four times that in the backward)


def pool_build(B, H, W, C, seed=0):
    """ReLU-style input (half the values exact zeros: ties) with scattered NaN, +inf, -inf, -0.0; channel 1 all -inf, channel 2 all equal,
    channel 3 alternating +0.0 / -0.0 (so the 1 x 1 and 2 x 2 maps see every kind of window too)."""
    g = gen(B, H, W, C, seed, 9)
    x = torch.relu(torch.randn(B, H, W, C, generator=g)).float()
    r = torch.rand(B, H, W, C, generator=g)
    x[r < 0.04] = float("nan")
    x[(r >= 0.04) & (r < 0.08)] = float("inf")
    x[(r >= 0.08) & (r < 0.20)] = float("-inf")
    x[(r >= 0.20) & (r < 0.25)] = -0.0
    x[..., 1] = float("-inf")
    x[..., 2] = 0.25
    alt = (torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2
    x[..., 3] = torch.where(alt == 0, torch.tensor(0.0), torch.tensor(-0.0))[None].expand(B, H, W)
    dy = torch.randn(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, generator=g).float()
    dx0 = torch.randn(B, H, W, C, generator=g).float()
    return x, dy, dx0


# ------------------------------------------------------------------------------------------------ Adam
ADAM_GRID = 8192 * 256
ADAM_SIZES = (1, 255, 257, 1000, ADAM_GRID + 1, 2 * ADAM_GRID + 3)      # the last two: a second and a third trip of the grid-stride loop
ADAM_SCALES = (1.0, 0.5, 0.125)
ADAM_STEPS = 5
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))


def adam_cases():
    """(n, first step, grad_scale): every size from step 1 and from step 1000, the scales cycling; every scale at n = 1000 for both."""
    out = []
    for i, n in enumerate(ADAM_SIZES):
        for j, first in enumerate((1, 1000)):
            out.append((n, first, ADAM_SCALES[(i + j) % 3]))
    for first in (1, 1000):
        for s in ADAM_SCALES:
            if (1000, first, s) not in out:
                out.append((1000, first, s))
    return out


ADAM_CASES = adam_cases()


def adam_zero_block(n):
    """the slice where g = m = v = 0"""
    return slice(n // 3, n // 3 + max(1, n // 8))


def adam_build(n, first, seed=0):
    """p, the gradients of ADAM_STEPS steps (log-uniform magnitude over 1e-12 .. 1e3, random sign, 5 % exact zeros), and the moments the
    first step starts from: zero at step 1, 'given' ones otherwise.  One block has g = m = v = 0 throughout."""
    g = gen(n, first, seed, 13)
    p = torch.randn(n, generator=g).float()
    mag = 10.0 ** (-12.0 + 15.0 * torch.rand(ADAM_STEPS, n, generator=g))
    sign = torch.where(torch.rand(ADAM_STEPS, n, generator=g) < 0.5, -1.0, 1.0)
    grads = (mag * sign).float()
    grads[torch.rand(ADAM_STEPS, n, generator=g) < 0.05] = 0.0
    if first == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = (0.3 * grads[0] + 0.01 * torch.randn(n, generator=g)).float()
        v = (grads[0] * grads[0] * (0.5 + torch.rand(n, generator=g))).float()
    z = adam_zero_block(n)
    grads[:, z] = 0.0
    m[z] = 0.0
    v[z] = 0.0
    return p, grads, m.float(), v.float()


# ------------------------------------------------------------------------------------------------ layout, elementwise, helpers
NCHW_TO_NHWC = ((3, 4, 0), (1, 4, 0), (4, 4, 0), (3, 16, 0), (5, 16, 7), (16, 16, 0))      # (C, Cp, choff); Cp = 4, choff = 0: the 16-byte kernel
NHWC_TO_NCHW = ((3, 4, 0), (1, 4, 3), (5, 16, 7), (16, 16, 0), (1, 1, 0))
NCHW3 = ((3, 16), (1, 4), (5, 16))                                                          # (C, Cp)
LAYOUT_BHW = ((1, 1, 1), (2, 3, 5), (3, 7, 13))                                             # odd H, W, and 1 x 1
LAYOUT_WRAP = (1, 1025, 1025)                                                               # pixels > 4096 * 256

ACTS = (0, 1, 2, 3)
ELEMENTWISE_N = (1, 255, 257, 4096 * 256 + 5)

COLSUM_C = (1, 9, 96, 256, 512)
COLSUM_PIX = (1, 127, 129, 5000)

COPY_CHANNELS = ((1, 1, 0, 1, 0, 1), (7, 5, 2, 9, 4, 3), (130, 16, 0, 48, 32, 16), (130, 48, 16, 16, 0, 16))      # (n_pix, Cs, soff, Cd, doff, C)
UPSAMPLE = ((1, 1, 1), (3, 1, 5), (2, 4, 1), (5, 3, 7), (64, 9, 11))                                               # (planes, h, w)
ADJ_FOLD = ((1, 1, 1, 4), (2, 1, 5, 8), (1, 4, 1, 4), (2, 3, 5, 16), (1, 2, 2, 64))                               # (B, Hl, Wl, C)
SPATIAL_MEAN = ((1, 1, 1, 1), (3, 2, 5, 12), (2, 7, 9, 70))                                                        # (B, H, W, C)


def randn(shape, *key):
    return torch.randn(shape, generator=gen(*key)).float()


def act_output(shape, act, *key):
    """A plausible OUTPUT of the activation (the kernels differentiate through the activated value), with exact zeros for the ReLU tie."""
    z = randn(shape, *key)
    if act == 1:
        y = torch.relu(z)
    elif act == 2:
        y = torch.nn.functional.elu(z)
    elif act == 3:
        y = torch.sigmoid(z)
    else:
        y = z
    return y.float()


def ulp_distance(a, b):
    """distance in float32 steps between two finite float32 tensors (sign-magnitude bits mapped onto one ordered integer line)"""
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


assert math.isclose(EPS, 1e-5, rel_tol=1e-6)
