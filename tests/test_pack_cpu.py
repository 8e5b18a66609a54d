"""No GPU: tests/pack_ref.py -- the restatement of the packed filter copies that tests/test_pack_gpu.py holds the kernels to -- against plain
float64 torch.  Each copy is used the way include/mcav_conv.h says the kernels use it, and the result must be the convolution (or its adjoint)
of the OIHW filter: a restatement that mislabels a tap, a parity class or a padding row would compute something else.  Everything here is exact
arithmetic on small integers stored in float64, so the comparisons are equalities."""
import pytest
import torch
import torch.nn.functional as F

import pack_ref as R
from nn_ops_ref import upsample_adj_fold_ref

F64 = torch.float64


def ints(g, *shape):
    """small integers: every product and sum below is exact in float32 and float64"""
    return torch.randint(-3, 4, shape, generator=g).to(torch.float32)


def im2col(x, k, stride, pad):
    """[B, Ho, Wo, taps, C]: tap (ky, kx) of output pixel (y, x) reads the zero-padded x at (y * stride + ky - pad, x * stride + kx - pad)"""
    B, C, H, W = x.shape
    cols = F.unfold(x, k, padding=pad, stride=stride)                     # [B, C * taps, L], rows ordered (c, ky, kx)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return cols.view(B, C, k * k, Ho, Wo).permute(0, 3, 4, 2, 1)


@pytest.mark.parametrize("shape", [(3, 2, 3, 1, 1), (5, 3, 7, 2, 3), (2, 5, 1, 1, 0), (4, 3, 5, 2, 2)], ids=lambda s: "%dx%dx%d_s%d" % s[:4])
def test_forward_copy_contracted_with_im2col_is_conv2d(shape):
    Cout, Cin, k, stride, pad = shape
    g = torch.Generator().manual_seed(11)
    w, x = ints(g, Cout, Cin, k, k), ints(g, 2, Cin, 6, 7)
    for Kp in (4, 16) if Cin <= 4 else (16,):
        Np, taps = R.up16(Cout), k * k
        p = R.pack_forward(w, Np, Kp)
        assert p.shape == (Np, R.kstride(taps, Kp)) and p.dtype == torch.float32
        cols = im2col(x.to(F64), k, stride, pad)                          # [B, Ho, Wo, taps, Cin]
        colsp = torch.zeros(cols.shape[:4] + (Kp,), dtype=F64)
        colsp[..., :Cin] = cols
        flat = torch.ones(cols.shape[:3] + (p.shape[1],), dtype=F64)      # (ones where no tap x channel lies: the copy's tail must be zero)
        flat[..., :taps * Kp] = colsp.reshape(cols.shape[:3] + (taps * Kp,))
        y = torch.einsum("bhwk,nk->bnhw", flat, p.to(F64))
        assert torch.equal(y[:, :Cout], F.conv2d(x.to(F64), w.to(F64), stride=stride, padding=pad))
        assert not y[:, Cout:].any()
        colsp[..., Cin:] = 1.0                                            # ... and the padding columns k >= Cin
        flat[..., :taps * Kp] = colsp.reshape(cols.shape[:3] + (taps * Kp,))
        assert torch.equal(torch.einsum("bhwk,nk->bnhw", flat, p.to(F64))[:, :Cout], F.conv2d(x.to(F64), w.to(F64), stride=stride, padding=pad))


@pytest.mark.parametrize("shape", [(3, 2, 3), (5, 3, 1), (2, 17, 3)], ids=lambda s: "%dx%dx%d" % s)
def test_transposed_copy_gives_conv_transpose2d(shape):
    """The data gradient of a stride-1 convolution: dx[pix, ci] = sum over taps and co of dy(pix + pad - tap)[co] * copy[ci][tap][co]."""
    Cout, Cin, k = shape
    g = torch.Generator().manual_seed(12)
    w, dy = ints(g, Cout, Cin, k, k), ints(g, 2, Cout, 5, 6)
    p = R.pack_transposed(w)
    Np, Kp, taps, pad = R.up16(Cin), R.up16(Cout), k * k, k // 2
    assert p.shape == (Np, taps * Kp)
    dyp = torch.ones(2, Kp, 5, 6, dtype=F64)                              # (ones in the padding channels: their filter columns must be zero)
    dyp[:, :Cout] = dy
    # tap (ky, kx) of the adjoint reads dy at (y + pad - ky, x + pad - kx): im2col of the flipped window
    cols = im2col(dyp, k, 1, pad).flip(3)                                 # [B, H, W, taps, Kp]
    dx = torch.einsum("bhwtk,ntk->bnhw", cols, p.view(Np, taps, Kp).to(F64))
    assert torch.equal(dx[:, :Cin], F.conv_transpose2d(dy.to(F64), w.to(F64), padding=pad))
    assert not dx[:, Cin:].any()


def test_bf16_planes_add_up_to_the_filter():
    g = torch.Generator().manual_seed(13)
    v = torch.randn(64, 144, generator=g) * torch.logspace(-6, 3, 64).view(64, 1)
    v[0, :8] = torch.tensor([0.0, -0.0, 1.0, 2.0 ** -126, 3.0e38, -1.0 - 2.0 ** -8, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9])      # ties and the ends of the range
    pl = R.planes(v)
    assert pl.dtype == torch.bfloat16 and pl.shape == (192, 144)
    h, m, l = (t.to(F64) for t in pl.view(3, 64, 144))
    assert torch.equal(pl[:64], R.to_bf16(v))
    # round to nearest EVEN: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 and goes to the even 1; 1 + 3 * 2^-9 lies above the tie
    assert h[0, 5] == -1.0 and h[0, 6] == 1.0 and h[0, 7] == 1.0 + 2.0 ** -7
    err = (h + m + l - v.to(F64)).abs()
    assert bool((err <= 2.0 ** -24 * v.to(F64).abs()).all()), float((err / v.abs().clamp_min(1e-45)).max())


def parity_conv(a, w, C1):
    """conv2d(reflect_pad(up2(a)), w[:, :C1]) in float64"""
    up = F.interpolate(a.to(F64), scale_factor=2, mode="nearest")
    return F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), w[:, :C1].to(F64))


def test_merged_tap_copy_is_the_upsample_convolution_per_parity_class():
    """Output pixel (2 s + py, 2 t + px) = the 2x2 convolution of the EDGE-REPLICATED low-resolution a, window rows s - 1 + py + {0, 1} (columns
    alike), with the class's four merged filters."""
    B, Hl, Wl, C1, Cin, Cout = 1, 3, 4, 2, 5, 3
    g = torch.Generator().manual_seed(14)
    w, a = ints(g, Cout, Cin, 3, 3), ints(g, B, C1, Hl, Wl)
    Np = R.up16(Cout)
    p = R.pack_upmerge(w, C1, Np).to(F64)
    assert p.shape == (4, Np, 4, C1) and not p[:, Cout:].any()
    want = parity_conv(a, w, C1)
    ar = F.pad(a.to(F64), (1, 1, 1, 1), mode="replicate")                 # index s + 1 holds row s
    for py in range(2):
        for px in range(2):
            wm = p[py * 2 + px, :Cout].view(Cout, 2, 2, C1).permute(0, 3, 1, 2)             # [Cout][C1][a][b]
            y = F.conv2d(ar[:, :, py:py + Hl + 1, px:px + Wl + 1], wm)
            assert torch.equal(y, want[:, :, py::2, px::2]), (py, px)


def test_merged_tap_adjoint_copy_in_the_headers_recipe_is_the_gradient():
    """1. the copy; 2. a 4x4 stride-2 convolution of dy, offset -3, zero padded, onto (Hl + 2) x (Wl + 2); 3. the ring fold."""
    B, Hl, Wl, C1, Cin, Cout = 1, 3, 4, 2, 5, 3
    g = torch.Generator().manual_seed(15)
    w, dy = ints(g, Cout, Cin, 3, 3), ints(g, B, Cout, 2 * Hl, 2 * Wl)
    a = torch.zeros(B, C1, Hl, Wl, dtype=F64).requires_grad_()
    parity_conv(a, w, C1).backward(dy.to(F64))
    Np, Kp = R.up16(C1), R.up16(Cout)
    p = R.pack_upmerge_adj(w, C1, Np, Kp).to(F64)
    assert p.shape == (Np, 16 * Kp)
    v = p.view(Np, 4, 4, Kp)
    assert not v[C1:].any() and not v[..., Cout:].any()
    dyp = torch.ones(B, Kp, 2 * Hl, 2 * Wl, dtype=F64)                    # (ones in the padding channels)
    dyp[:, :Cout] = dy
    # destination pixel d, tap u reads dy at 2 d + u - 3: a stride-2 convolution with zero padding 3
    tmp = F.conv2d(dyp, v.permute(0, 3, 1, 2), stride=2, padding=3)
    assert tmp.shape == (B, Np, Hl + 2, Wl + 2)
    out = upsample_adj_fold_ref(tmp.permute(0, 2, 3, 1), None, 0, None).permute(0, 3, 1, 2)
    assert torch.equal(out[:, :C1], a.grad)
    assert not out[:, C1:].any()
