"""float64 definitions of the operations behind csrc/nn_ops.hip and the helpers of csrc/aux_ops.hip (test infrastructure).

Plain torch on the CPU, nothing imported from the product: each function is meant to be read as WHAT the kernel of the same name computes.
Activations are NHWC ([B, H, W, C], or [n_pix, C] where the pixel grid does not matter).  Every function accepts any float dtype and computes
in the dtype it is handed: called on .double() inputs it is the reference, called on the float32 inputs it is the "plain fp32 evaluation of
the same formula" of the three-column rule (tests/arbiter.py).  tests/test_nn_ops_cpu.py checks these against torch's own operators.
"""
import math

import torch

ACT_NONE, ACT_RELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ BatchNorm, training mode
def bn_finalize_ref(slab, count, gamma, beta, eps, momentum, running_mean, running_var, groups):
    """slab: [groups * mtiles, 2, C] per-tile sums of x and x^2 (what the convolution's epilogue leaves, float32); count: pixels per group.
    -> dict of float64 tensors: scale, shift, mean, invstd [groups, C]; var (biased, after the clamp), var_raw (before it);
    running_mean / running_var [C] after the groups were applied in order (None when none were given).
    Biased variance E[x^2] - mean^2 clamped at 0 for the normalisation; the running variance takes the unbiased one (x count / (count - 1),
    only when count > 1), as nn.BatchNorm2d does."""
    C = slab.shape[-1]
    s = slab.double().reshape(groups, -1, 2, C).sum(1)
    mean = s[:, 0] / count
    var_raw = s[:, 1] / count - mean * mean
    var = var_raw.clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    rm = rv = None
    if running_mean is not None:
        rm, rv = running_mean.double().clone(), running_var.double().clone()
        for g in range(groups):
            unbiased = var[g] * count / (count - 1.0) if count > 1 else var[g]
            rm = (1.0 - momentum) * rm + momentum * mean[g]
            rv = (1.0 - momentum) * rv + momentum * unbiased
    return dict(scale=scale, shift=shift, mean=mean, invstd=invstd, var=var, var_raw=var_raw, running_mean=rm, running_var=rv)


def bn_eval_coeffs_ref(gamma, beta, running_mean, running_var, eps):
    """Eval-mode BatchNorm as one multiply-add per element: y = (x - running_mean) / sqrt(running_var + eps) * gamma + beta = x * scale + shift.
    -> (scale, shift) [C]: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale.  running_var is a VARIANCE, eps is
    added to it under the root, and nothing of the batch enters."""
    scale = gamma / torch.sqrt(running_var + eps)
    return scale, beta - running_mean * scale


def bn_apply_ref(x, scale, shift, residual, relu, groups):
    """x: [n_pix, C], group g owns rows [g * n_pix / groups, (g + 1) * n_pix / groups); scale, shift: [groups, C].
    -> act(x * scale + shift (+ residual))."""
    n, C = x.shape
    y = x.reshape(groups, n // groups, C) * scale[:, None, :] + shift[:, None, :]
    y = y.reshape(n, C)
    if residual is not None:
        y = y + residual
    return y.clamp_min(0.0) if relu else y


def bn_bwd_ref(dy, y_act, x, gamma, mean, invstd, relu, groups, sums=None):
    """Backward of bn_apply_ref at given saved mean / invstd [groups, C] (csrc/bn_bwd_formula.h).
    g = dy where y_act > 0 (relu), else dy;  xhat = (x - mean) * invstd;  s1 = sum g, s2 = sum g * xhat per group and channel;
    dx = gamma * invstd * (g - s1 / n - xhat * s2 / n), n = pixels per group;  dgamma = sum_groups s2, dbeta = sum_groups s1.
    sums: use these [groups, 2, C] in the dx formula instead of the exact ones (the second pass on its own).
    -> dict: dx, dres (= g) [n_pix, C]; sums [groups, 2, C]; dgamma, dbeta [C]; abs1, abs2 [groups, C] (sums of |g| and |g * xhat|:
    what the error of a sum is measured against)."""
    n, C = x.shape
    per = n // groups
    g = torch.where(y_act > 0, dy, torch.zeros_like(dy)) if relu else dy          # masked elements are +0.0, whatever dy's sign
    gg, xg = g.reshape(groups, per, C), x.reshape(groups, per, C)
    xhat = (xg - mean[:, None, :]) * invstd[:, None, :]
    s1, s2 = gg.sum(1), (gg * xhat).sum(1)
    exact = torch.stack([s1, s2], 1)
    use = exact if sums is None else sums
    dx = (gamma[None, None, :] * invstd[:, None, :]) * (gg - use[:, 0, None, :] / per - xhat * (use[:, 1, None, :] / per))
    return dict(dx=dx.reshape(n, C), dres=g, sums=exact, dgamma=s2.sum(0), dbeta=s1.sum(0), abs1=gg.abs().sum(1), abs2=(gg * xhat).abs().sum(1),
                xhat=xhat.reshape(n, C))


# ------------------------------------------------------------------------------------------------ MaxPool 3x3, stride 2, padding 1
def pool_out(n):
    return (n - 1) // 2 + 1


def maxpool_ref(x):
    """x: [B, H, W, C] -> (values [B, Ho, Wo, C], winning tap ky * 3 + kx in 0..8, uint8).  The window of output (oy, ox) is rows 2 oy - 1 + ky,
    columns 2 ox - 1 + kx; taps are visited in that order, out-of-bounds ones skipped.  torch's rule: the first in-bounds element initialises;
    a later one replaces it when it is greater or NaN (so a NaN is replaced only by a later NaN, and a window of -inf keeps its first tap)."""
    B, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    oy, ox = torch.arange(Ho), torch.arange(Wo)
    best = torch.zeros((B, Ho, Wo, C), dtype=x.dtype)
    tap = torch.zeros((B, Ho, Wo, C), dtype=torch.uint8)
    first = torch.ones((B, Ho, Wo, C), dtype=torch.bool)
    for ky in range(3):
        iy = 2 * oy - 1 + ky
        for kx in range(3):
            ix = 2 * ox - 1 + kx
            valid = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
            v = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            take = valid[None, :, :, None] & (first | (v > best) | torch.isnan(v))
            best = torch.where(take, v, best)
            tap = torch.where(take, torch.full_like(tap, ky * 3 + kx), tap)
            first = first & ~take
    return best, tap


def maxpool_bwd_ref(dy, tap, in_shape, dx=None):
    """The adjoint of the selection maxpool_ref made: every dy goes to the input element its tap names (added to dx when one is given)."""
    B, H, W, C = in_shape
    Ho, Wo = pool_out(H), pool_out(W)
    out = torch.zeros(in_shape, dtype=dy.dtype) if dx is None else dx.clone()
    t = tap.long()
    b, oy, ox, c = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), torch.arange(C), indexing="ij")
    iy, ix = 2 * oy - 1 + t // 3, 2 * ox - 1 + t % 3
    out.index_put_((b.reshape(-1), iy.reshape(-1), ix.reshape(-1), c.reshape(-1)), dy.reshape(-1), accumulate=True)
    return out


# ------------------------------------------------------------------------------------------------ Adam (torch.optim.Adam's defaults)
def adam_ref(p, g, m, v, lr, b1, b2, eps, step, grad_scale):
    """One update, `step` counted from 1, no weight decay, no amsgrad.  -> (p, m, v) in the dtype of the inputs (hand it doubles)."""
    g = g * grad_scale
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = torch.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


# ------------------------------------------------------------------------------------------------ layout
def nchw_to_nhwc_ref(src, dst, choff):
    """src [B, C, H, W] into channels [choff, choff + C) of dst [B, H, W, Cp]; every other channel keeps what dst held."""
    out = dst.clone()
    out[..., choff:choff + src.shape[1]] = src.permute(0, 2, 3, 1)
    return out


def nhwc_to_nchw_ref(src, C, choff):
    return src[..., choff:choff + C].permute(0, 3, 1, 2).contiguous()


def nchw3_to_nhwc_ref(s0, s1, s2, Cp):
    """cat(s0, s1, s2) along channels -> [B, H, W, Cp], zeros past 3 C."""
    B, C, H, W = s0.shape
    out = torch.zeros((B, H, W, Cp), dtype=s0.dtype)
    out[..., :3 * C] = torch.cat([s0, s1, s2], 1).permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------------ elementwise
def dact_ref(y, act):
    """The activation's derivative written in its OUTPUT y: ReLU 1[y > 0]; ELU (alpha 1) 1 for y > 0, else y + 1; sigmoid y (1 - y)."""
    if act == ACT_RELU:
        return (y > 0).to(y.dtype)
    if act == ACT_ELU:
        return torch.where(y > 0, torch.ones_like(y), y + 1.0)
    if act == ACT_SIGMOID:
        return y * (1.0 - y)
    return torch.ones_like(y)


def act_bwd_ref(dy, y, act, dx=None):
    v = dy * dact_ref(y, act)
    return v if dx is None else dx + v


def act_bwd_strided_ref(dy, y, act, dst, stride):
    """dy * act'(y) for n elements, written to every stride-th element of dst; the others keep what dst held."""
    out = dst.clone().reshape(-1)
    out[:dy.numel() * stride:stride] = (dy * dact_ref(y, act)).reshape(-1)
    return out.reshape(dst.shape)


def spatial_mean_ref(x, scale):
    """x [B, H, W, C] -> scale * mean over H, W: [B, C]."""
    return scale * x.mean((1, 2))


def spatial_mean_bwd_ref(dout, shape, scale):
    B, H, W, C = shape
    return (dout * (scale / (H * W)))[:, None, None, :].expand(B, H, W, C).contiguous()


def copy_channels_ref(src, soff, dst, doff, C, accumulate):
    """src [n_pix, Cs], channels [soff, soff + C) -> (added to, when accumulate) channels [doff, doff + C) of dst [n_pix, Cd]."""
    out = dst.clone()
    if accumulate:
        out[:, doff:doff + C] += src[:, soff:soff + C]
    else:
        out[:, doff:doff + C] = src[:, soff:soff + C]
    return out


def colsum_ref(x, out=None):
    """x [n_pix, C] -> per-channel sums [C] (added to out when one is given)."""
    s = x.sum(0)
    return s if out is None else out + s


def upsample_nearest2x_ref(src):
    """[planes, h, w] -> [planes, 2 h, 2 w], every pixel repeated 2 x 2."""
    return src.repeat_interleave(2, 1).repeat_interleave(2, 2)


def upsample_nearest2x_bwd_ref(g):
    """adjoint: [planes, 2 h, 2 w] -> [planes, h, w], the sum of each 2 x 2 block."""
    P, H, W = g.shape
    return g.reshape(P, H // 2, 2, W // 2, 2).sum((2, 4))


def replicate_ring_ref(x):
    """[B, Hl, Wl, C] -> [B, Hl + 2, Wl + 2, C]: the map with its border pixels replicated into a ring of one (the operator whose adjoint
    upsample_adj_fold_ref is, before the activation factor)."""
    B, Hl, Wl, C = x.shape
    iy = torch.arange(-1, Hl + 1).clamp(0, Hl - 1)
    ix = torch.arange(-1, Wl + 1).clamp(0, Wl - 1)
    return x[:, iy][:, :, ix]


def upsample_adj_fold_ref(tmp, aux, act, addend):
    """tmp: gradient on the edge-replicated domain [B, Hl + 2, Wl + 2, C].  The ring is folded (added) onto the border pixel it was
    replicated from -- a corner of the ring onto the corner pixel, and with Hl or Wl = 1 both sides onto the same pixel -- then
    * act'(aux) (aux None: no factor) + addend (None: nothing)."""
    B, Hp, Wp, C = tmp.shape
    Hl, Wl = Hp - 2, Wp - 2
    iy = torch.arange(-1, Hl + 1).clamp(0, Hl - 1)
    ix = torch.arange(-1, Wl + 1).clamp(0, Wl - 1)
    rows = torch.zeros((B, Hl, Wp, C), dtype=tmp.dtype).index_add_(1, iy, tmp)
    out = torch.zeros((B, Hl, Wl, C), dtype=tmp.dtype).index_add_(2, ix, rows)
    if aux is not None:
        out = out * dact_ref(aux, act)
    return out if addend is None else out + addend
