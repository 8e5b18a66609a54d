"""The one-channel disparity head of csrc/narrow_conv.hip in plain torch on the CPU, and how far an fp32 kernel may be from that definition.

The definition is tests/halo_ref.py's with Cout = 1 and reflect = True: F.pad(mode="reflect"), F.conv2d and autograd in float64 (or, with
dtype=torch.float32, in float32: the self-check of tests/test_head_cpu.py).  Every function returns the result together with an elementwise
bound on |kernel - want64| that is computed from the INPUTS and float64 alone, never from a kernel's output.  Tensors are NCHW here.

The envelope is halo_ref's, ks(K) * S with ks(K) = 2 (K + 2) 2^-24 and S the same expression on |operands|; its derivation covers this
kernel's order of evaluation:

  forward        9 C products, summed per lane (3 taps x 4 channels), across the three rows of the rotating accumulators, across the C / 4
                 lanes of a pixel, plus the bias: any order of K = 9 C products.  halo_ref.forward.
  dx             the kernel gathers G[tap] = dpre[p + 1 - tap] and, next to the border, adds the at most three outputs whose padded tap
                 reflected onto p: at most 3 additions, then 9 products and 8 additions, fewer than the 16 products + additions of
                 halo_ref.adjoint's K = 16 Cout = 16.  * act_x'(x) + addend is that function's epilogue: |a'| (ks(16) + 3 u) S + u |addend|.
                 All three act_x go through the OUTPUT x: NONE (1) and RELU (x > 0) are exact, ELU (x > 0 ? 1 : x + 1) is one fp32 addition,
                 which the 3 u of the epilogue term already holds.
  dw, db         dw[c][tap] = sum_p G[p][tap] x[p][c]: every output q with dpre[q] != 0 sends its value to exactly one p per tap, so at most
                 |P| of the products are non-zero (P = the support of dy) and G's own additions are at most 3; the lane chains, the wavefront
                 shuffles, the LDS rows, the slab rows of the other workgroups (exact zeros where a workgroup saw no support) and the finalize
                 tree are one more order of the same sum.  halo_ref.wgrad: K = |P| + 8.

What the head has on top:

  the fused form (y given, act SIGMOID or RELU).  The kernel forms dpre^ = fl(dy * fl(y * fl(1 - y))) where the definition forms
                 dpre = dy y (1 - y) in float64 from the same fp32 y and dy: dpre^ = dpre (1 + d), |d| <= 3 u to first order.  dx, dw and db
                 are linear in dpre, so each moves by at most 3 u times its own S-expression (the adjoint of |dpre| and |w|, times |a'|;
                 wgrad(|x|, |dpre|); sum |dpre|).  The envelope gains exactly that term.  With y = NULL (dy is dpre already: act NONE) the
                 term is absent.  RELU's derivative (y > 0) is exact; the term is kept for it as well, it only needs to be an upper bound.
  accumulate = 1 the finalize adds the reduced sum s^ onto what the buffer holds by one IEEE addition: fl(fill + s^) differs from fill + s by
                 at most |s^ - s| + u |fill + s^|; u |s^| sits in the + 8 of K, u |fill| is added (accumulated()).

Where S = 0 the envelope of dx is u |addend| and the kernel's own arithmetic there is 0 * a' + addend: the test asks for the addend's exact
bits (an exact zero with no addend).  A NaN (an element a kernel never stored) is outside every envelope.

restate() writes the backward the way the KERNEL formulates it -- the gather G with its yt / yb / xl / xr and corner terms -- in plain torch,
in float32 or float64; in float64 it must equal the autograd definition (tests/test_head_cpu.py), and with one named term dropped it is a
mutant that the envelope has to reject."""
import torch
import torch.nn.functional as F

import halo_ref as R
from halo_ref import F32, F64, U, ks, outside, ratio  # noqa: F401  (the judge is halo_ref's)

ACT_NONE, ACT_RELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3      # include/mcav_conv.h


def act_fwd(v, act):
    return {ACT_NONE: lambda t: t, ACT_RELU: torch.relu, ACT_ELU: F.elu, ACT_SIGMOID: torch.sigmoid}[act](v)


def act_bwd(y, act):
    """act'(.) through the activation's OUTPUT y, as the kernels form it"""
    if act == ACT_RELU:
        return (y > 0).to(y.dtype)
    if act == ACT_ELU:
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    if act == ACT_SIGMOID:
        return y * (1 - y)
    return torch.ones_like(y)


def pre_gradient(dy, y, act, dtype=F64):
    """dpre = dy * act'(y) (dy itself when y is None), every operation in dtype"""
    dy = dy.to(dtype)
    return dy if y is None else dy * act_bwd(y.to(dtype), act)


def forward(x, w, b, dtype=F64):
    """x [B, C, H, W], w [1, C, 3, 3], b [1] or None -> (pre-activation, envelope)"""
    return R.forward(x, w, b, True, dtype=dtype)


def backward(x, w, dy, y=None, act=ACT_NONE, x_act=ACT_ELU, addend=None, dtype=F64):
    """-> dict(dx, edx, S, dw, edw, Sw, db, edb, Sb): the three gradients of the head with their envelopes; S, Sw, Sb are the S-expressions
    of the adjoint (where it is 0 no output with a non-zero dy reaches the pixel), of dw and of db.  y given: the fused form."""
    fused = y is not None
    dpre = pre_gradient(dy, y, act, dtype)
    g, E = R.adjoint(dpre, w, dtype=dtype)
    S = E / ks(16)
    a = act_bwd(x.to(dtype), x_act)
    add = addend.to(dtype) if addend is not None else torch.zeros_like(g)
    edx = a.double().abs() * (ks(16) + 3 * U + (3 * U if fused else 0.0)) * S + U * add.double().abs()
    dw, edw, db, edb = R.wgrad(x, dpre, True, dtype=dtype)
    k = ks(R.support_pixels(dpre) + 8)
    Sw, Sb = edw / k, edb / k
    if fused:
        edw, edb = edw + 3 * U * Sw, edb + 3 * U * Sb
    return dict(dx=g * a + add, edx=edx, S=S, dw=dw, edw=edw, Sw=Sw, db=db, edb=edb, Sb=Sb)


def accumulated(want, env, fill):
    """accumulate = 1 onto a buffer holding `fill`: -> (fill + want, env + u |fill|)"""
    return want.double() + fill, env + U * abs(fill)


# ------------------------------------------------------------------------------------------------ the kernel's own formulation
BORDER_TERMS = ("yt", "yb", "xl", "xr", "yt&xl", "yt&xr", "yb&xl", "yb&xr")
MUTANTS = BORDER_TERMS + ("swap ky",)


def restate(x, w, dpre, x_act=ACT_ELU, addend=None, dtype=F64, drop=None, skip=None):
    """dx, dw, db from G, as conv3x3r_c1_bwd_kernel gathers it.  drop: one of MUTANTS (that term is left out / ky is not mirrored);
    skip = (n, y0, y1, x0, x1): that tile is never walked -- its dx stays NaN and its pixels add nothing to dw and db."""
    x, w, dpre = x.to(dtype), w.to(dtype), dpre.to(dtype)
    B, C, H, W = x.shape
    Z = F.pad(dpre[:, 0], (1, 1, 1, 1))                                   # zero outside the image, as the tile's dpre halo
    N = [[Z[:, a:a + H, b:b + W] for b in range(3)] for a in range(3)]    # N[a][b](py, px) = dpre[py - 1 + a][px - 1 + b]
    G = [[(N[ky][2 - kx] if drop == "swap ky" else N[2 - ky][2 - kx]).clone() for kx in range(3)] for ky in range(3)]
    py, px = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    on = lambda name, m: m.to(dtype) if drop != name else torch.zeros_like(m, dtype=dtype)      # noqa: E731
    yt, yb, xl, xr = py == 1, py == H - 2, px == 1, px == W - 2
    for kx in range(3):
        G[0][kx] = G[0][kx] + on("yt", yt) * N[0][2 - kx]
        G[2][kx] = G[2][kx] + on("yb", yb) * N[2][2 - kx]
    for ky in range(3):
        G[ky][0] = G[ky][0] + on("xl", xl) * N[2 - ky][0]
        G[ky][2] = G[ky][2] + on("xr", xr) * N[2 - ky][2]
    G[0][0] = G[0][0] + on("yt&xl", yt & xl) * N[0][0]
    G[0][2] = G[0][2] + on("yt&xr", yt & xr) * N[0][2]
    G[2][0] = G[2][0] + on("yb&xl", yb & xl) * N[2][0]
    G[2][2] = G[2][2] + on("yb&xr", yb & xr) * N[2][2]
    Gt = torch.stack([G[ky][kx] for ky in range(3) for kx in range(3)], 1)      # [B, 9, H, W]
    dx = torch.einsum("bthw,ct->bchw", Gt, w[0].reshape(C, 9)) * act_bwd(x, x_act)
    if addend is not None:
        dx = dx + addend.to(dtype)
    center = dpre[:, 0]
    if skip is not None:
        n, y0, y1, x0, x1 = skip
        Gt, center = Gt.clone(), center.clone()
        Gt[n, :, y0:y1, x0:x1] = 0
        center[n, y0:y1, x0:x1] = 0
        dx[n, :, y0:y1, x0:x1] = float("nan")
    dw = torch.einsum("bthw,bchw->ct", Gt, x).reshape(1, C, 3, 3)
    return dx, dw, center.sum().reshape(1)
