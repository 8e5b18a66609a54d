"""TEST INFRASTRUCTURE: the depth pyramid's definition in float64 (include/mcav_depth.h: mcav_depth_pyramid_fwd / _bwd).

The taps are csrc/pyramid_math.h's bil_src restated in numpy float32, operation by operation (scale = h / H in float32), so that on
non-dyadic ratios the float64 reference uses the SAME weights as the kernels: there the float32 weights alone move a result by more than
the rounding the tests look for.  Everything after the weights is float64.  For dyadic ratios the weights are exact and the same numbers
come out of F.interpolate in float64 (tests/test_pyramid_cpu.py checks both statements).
"""
import numpy as np
import torch

EPS = 2.0 ** -24


def taps(h, H, fma=False):
    """bil_src for every output: (i0 [H], i1 [H], lam [H] float32).  fma: scale * (o + 0.5) - 0.5 rounded once, as the device code does (the
    compiler contracts it to one fused multiply-add); otherwise product and difference round separately, as in the host check's build."""
    f = np.float32
    scale = f(h) / f(H)
    o = np.arange(H, dtype=np.float32)
    if fma:     # the product of two float32 is exact in float64, and so is the difference (under 40 significant bits): one rounding
        s = (np.float64(scale) * (o + f(0.5)).astype(np.float64) - 0.5).astype(np.float32)
    else:
        s = scale * (o + f(0.5)) - f(0.5)
    s = np.where(s < 0, f(0), s).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), h - 1)
    i1 = i0 + (i0 < h - 1)
    lam = (s - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, lam


def axis_matrix(h, H, fma=False):
    """[H, h] float64: row o holds the weights (float32 values, widened) of output o."""
    i0, i1, lam = taps(h, H, fma)
    A = np.zeros((H, h))
    o = np.arange(H)
    np.add.at(A, (o, i0), (np.float32(1) - lam).astype(np.float64))
    np.add.at(A, (o, i1), lam.astype(np.float64))
    return torch.from_numpy(A)


def window_sizes(h, H, fma=False):
    """Number of outputs whose taps touch each source index (taps counted by index: lower tap i - 1 or i)."""
    i0, _, _ = taps(h, H, fma)
    return torch.tensor([int(((i0 == i - 1) | (i0 == i)).sum()) for i in range(h)], dtype=torch.float64)


def depth_of(d):
    return 1.0 / (10.0 * d + 0.01)


def forward64(disp, H, W, resize_then_depth, fma=False):
    """disp [B,h,w] -> (out [B,H,W] float64, scale [B,H,W]: the largest of the four contributing depths)."""
    d = disp.double()
    _, h, w = d.shape
    Ay, Ax = axis_matrix(h, H, fma), axis_matrix(w, W, fma)
    D = depth_of(d)
    if resize_then_depth:
        out = depth_of(torch.einsum("yi,bij,xj->byx", Ay, d, Ax))
    else:
        out = torch.einsum("yi,bij,xj->byx", Ay, D, Ax)
    y0, y1, _ = taps(h, H, fma)
    x0, x1, _ = taps(w, W, fma)
    corner = lambda ys, xs: D[:, torch.from_numpy(ys)][:, :, torch.from_numpy(xs)]
    scale = torch.stack([corner(y0, x0), corner(y0, x1), corner(y1, x0), corner(y1, x1)]).amax(0)
    return out, scale


def backward64(disp, d_out, resize_then_depth, fma=False):
    """-> (d_disp [B,h,w] float64, S: the same adjoint applied to |d_out| |dD/d.|, N: terms in each element's window)."""
    d = disp.double()
    g = d_out.double()
    _, h, w = d.shape
    H, W = g.shape[-2:]
    Ay, Ax = axis_matrix(h, H, fma), axis_matrix(w, W, fma)
    adj = lambda t: torch.einsum("yi,byx,xj->bij", Ay, t, Ax)
    if resize_then_depth:
        slope = -10.0 * depth_of(torch.einsum("yi,bij,xj->byx", Ay, d, Ax)) ** 2
        grad, S = adj(g * slope), adj(g.abs() * slope.abs())
    else:
        slope = -10.0 * depth_of(d) ** 2
        grad, S = slope * adj(g), slope.abs() * adj(g.abs())
    N = window_sizes(h, H, fma)[:, None] * window_sizes(w, W, fma)[None, :]
    return grad, S, N


def backward_bound(S, N):
    """Worst-case rounding of a float32 sum of N terms in any order, plus the handful of operations that form each term."""
    return (N + 8.0) * EPS * S
