"""Plain torch restatements of the packed filter copies of include/mcav_conv.h (mcav_pack_weights ... mcav_pack_weights_upmerge_adj), written
from the header's text: element by element, no kernel's index arithmetic.  Every function takes the OIHW float32 filter on the CPU and returns
the copy as the header lays it out, padding zeros included, so a comparison with a kernel's destination can be bit for bit.

The fp32 copies only move data.  The bf16 copies round to nearest even (torch's float32 -> bfloat16 conversion).  The merged-tap copies SUM
filter taps in float32: the sums are taken in the kernels' stated order (ky outer, kx inner, starting from 0.f), which makes them bit-exact too.
tests/test_pack_cpu.py checks these restatements against float64 convolutions; tests/test_pack_gpu.py checks the kernels against them."""
import torch

F32 = torch.float32
S = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}          # S(parity, merged tap): the filter taps a merged tap stands for
SY = {0: (2,), 1: (1, 2), 2: (0, 1), 3: (0,)}                              # Sy(u): the filter taps of adjoint tap u


def up16(v):
    return (v + 15) // 16 * 16


def kstride(taps, Kp):
    """row stride of a packed copy: taps * Kp rounded up to 16"""
    return up16(taps * Kp)


def pack_forward(w, Np, Kp):
    """[Np][Kstride], element [n][tap * Kp + k] = w[n][k][tap]; rows n >= Cout, columns k >= Cin and the tail past taps * Kp are zero"""
    Cout, Cin, kh, kw = w.shape
    taps = kh * kw
    out = torch.zeros(Np, kstride(taps, Kp), dtype=F32)
    body = torch.zeros(Np, taps, Kp, dtype=F32)
    body[:Cout, :, :Cin] = w.reshape(Cout, Cin, taps).permute(0, 2, 1)
    out[:, :taps * Kp] = body.reshape(Np, taps * Kp)
    return out


def pack_transposed(w):
    """the data-gradient filter [up16(Cin)][taps * up16(Cout)], element [ci][tap * Kp + co] = w[co][ci][tap]"""
    Cout, Cin, kh, kw = w.shape
    taps, Np, Kp = kh * kw, up16(Cin), up16(Cout)
    body = torch.zeros(Np, taps, Kp, dtype=F32)
    body[:Cin, :, :Cout] = w.reshape(Cout, Cin, taps).permute(1, 2, 0)
    return body.reshape(Np, taps * Kp)


def to_bf16(p):
    """round to nearest even"""
    return p.to(torch.bfloat16)


def planes(p):
    """[3 * rows][cols] bf16: h = bf16(v), m = bf16(v - h), l = bf16((v - h) - m), the differences in float32"""
    h = p.to(torch.bfloat16)
    r1 = p - h.to(F32)
    m = r1.to(torch.bfloat16)
    l = (r1 - m.to(F32)).to(torch.bfloat16)
    return torch.cat([h, m, l], 0)


def _sum_in_order(w, kys, kxs):
    """sum of w[..., ky, kx] over ky in kys (outer), kx in kxs (inner), float32, starting from zero"""
    acc = torch.zeros(w.shape[:-2], dtype=F32)
    for ky in kys:
        for kx in kxs:
            acc = acc + w[..., ky, kx]
    return acc


def pack_upmerge(w, C1, Np):
    """[4 classes (py, px)][Np][4 merged taps (a, b)][C1]: the sum of w[n][c][ky][kx] over ky in S(py, a), kx in S(px, b); rows n >= Cout zero"""
    Cout = w.shape[0]
    out = torch.zeros(4, Np, 4, C1, dtype=F32)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    out[py * 2 + px, :Cout, a * 2 + b, :] = _sum_in_order(w[:, :C1], S[(py, a)], S[(px, b)])
    return out


def pack_upmerge_adj(w, C1, Np, Kp):
    """[Np][16 taps u * 4 + v][Kp]: V[u][v][c1][co] = the sum of w[co][c1][ky][kx] over ky in Sy(u), kx in Sy(v); rows c1 >= C1 and columns
    co >= Cout zero"""
    Cout = w.shape[0]
    out = torch.zeros(Np, 16, Kp, dtype=F32)
    for u in range(4):
        for v in range(4):
            out[:C1, u * 4 + v, :Cout] = _sum_in_order(w[:, :C1], SY[u], SY[v]).t()
    return out.reshape(Np, 16 * Kp)
