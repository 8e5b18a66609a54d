"""The halo-tile convolutions of csrc/conv_halo.hip in plain torch on the CPU, and how far an fp32 kernel may be from that definition.

Every function evaluates one kernel form with F.pad(mode="reflect") / zero padding, F.interpolate(nearest), F.conv2d and autograd -- in float64
(the definition) or, with dtype=torch.float32, in float32 (the self-check of tests/test_halo_cpu.py) -- and returns (want, envelope): the
result and an elementwise bound on |kernel - want64| that is computed from the INPUTS and float64 alone, never from a kernel's output.
Tensors are NCHW here; the tests permute.

The envelope.  u = 2^-24 is the unit roundoff of fp32.  A sum of K products evaluated in fp32 in ANY order (a chain, the MFMA's four-product
steps, partial sums per wavefront that are added later) differs from the exact sum by at most ((1 + u)^(K + 1) - 1) * sum |products|: every
product is rounded once and passes through at most K - 1 additions, plus one for the bias / the accumulate into the gradient buffer.  To first
order that is (K + 2) u sum|products|.  The MFMA is not required to round its internal additions to nearest; a truncating add loses at most
2 u instead of u per operation, so the bound carries a factor 2:

    ks(K) = 2 (K + 2) 2^-24            envelope = ks(K) * S,  S = the same expression evaluated on |operands|

K is the worst-case number of products of one output element:

  forward (activation NONE)   want = conv(x, w) + b, S = conv(|x|, |w|) + |b|, K = 9 C.  The merged-tap form adds at most four weights in
                              fp32 first (3 additions, relative error <= 3 u on a sum of at most 4 |w|) and then sums 4 C products:
                              (3 + 4 C + 2) u < (9 C + 2) u, the same expression covers it.
  reflect-adjoint             want = d/dx <dy, conv(reflect_pad(x), w)> by autograd, S = the same gradient for |dy| and |w|.  An interior pixel
                              collects 9 Cout products; the pixel (1, 1) also collects line 0 under ky = 0 (3), column 0 under kx = 0 (3) and
                              the corner (1): K = 16 Cout.
      pool                    the 2x2 sum of four such pixels: want and S are sum-pooled, K is multiplied by 4.
      * act'(aux) + addend    the kernel computes r = fl(fl(g^ * a^) + add) with g^ = g + d, |d| <= E = ks(K) S, and a^ = a' (1 + e1): the ELU
                              derivative through its output, aux > 0 ? 1 : aux + 1, is one fp32 addition of an fp32 number (exact in float64).
                              r = ((g + d) a' (1 + e1)(1 + e2) + add)(1 + e3), |e_i| <= u, so to first order
                                  |r - (g a' + add)| <= |a'| E + |g a'| (e1 + e2 + e3) + |add| e3 <= |a'| (ks(K) + 3 u) S + u |add|
                              because |g| <= S.  The second-order terms are below u^2 K S and sit inside the factor 2 of ks.
  weight / bias gradient      want = d/dw <dy, conv(pad(up(x)), w)> by autograd, S the same for |x| and |dy|; db = sum dy, S = sum |dy|.  Only
                              pixels on which dy is non-zero contribute a non-zero product, and adding a zero partial (other lanes' k-steps,
                              other wavefronts, other workgroups' slab rows) is exact: K = |P| + 8, P = the pixels with dy != 0 in any
                              channel; the 8 allow for the un-merge of the merged-tap form (4 classes), the slab reduction's own order and the
                              accumulate into the gradient buffer.

Where S = 0 the envelope is 0 and the kernel must store an exact zero; a NaN (an element a kernel never stored) is outside every envelope."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32


def ks(K):
    return 2.0 * (K + 2) * U


def _conv(x, w, b, reflect, up):
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    x = F.pad(x, (1, 1, 1, 1), mode="reflect") if reflect else F.pad(x, (1, 1, 1, 1))
    return F.conv2d(x, w, b)


def forward(x, w, b, reflect, up=False, dtype=F64):
    """x [B, C, H, W] (half size when up), w [Cout, C, 3, 3], b [Cout] or None -> (conv + b, envelope)"""
    x, w, b = x.to(dtype), w.to(dtype), (None if b is None else b.to(dtype))
    want = _conv(x, w, b, reflect, up)
    S = _conv(x.abs(), w.abs(), None if b is None else b.abs(), reflect, up)
    return want, ks(9 * w.shape[1]) * S.double()


def _sum_pool(t):
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 2, 2, W // 2, 2).sum((3, 5))


def elu_bwd(y):
    """act'(.) of the ELU through its output y, as the kernels form it"""
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def adjoint(dy, w, pool=False, aux=None, addend=None, dtype=F64):
    """dy [B, Cout, H, W], w [Cout, C, 3, 3] -> (gradient at the reflection-padded conv's input [B, C, H(/2), W(/2)], envelope);
    aux: the producer's ELU OUTPUT, addend: added last (both at the result's size)"""
    dy, w = dy.to(dtype), w.to(dtype)
    B, Cout, H, W = dy.shape

    def grad(d, ww):
        x = torch.zeros(B, w.shape[1], H, W, dtype=dtype, requires_grad=True)
        return torch.autograd.grad(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), ww), x, d)[0]

    g, S, K = grad(dy, w), grad(dy.abs(), w.abs()).double(), 16 * Cout
    if pool:
        g, S, K = _sum_pool(g), _sum_pool(S), 4 * K
    if aux is None and addend is None:
        return g, ks(K) * S
    a = elu_bwd(aux.to(dtype)) if aux is not None else torch.ones_like(g)
    add = addend.to(dtype) if addend is not None else torch.zeros_like(g)
    return g * a + add, a.double().abs() * (ks(K) + 3 * U) * S + U * add.double().abs()


def support_pixels(dy):
    """|P|: the pixels (n, y, x) on which dy is non-zero in any channel"""
    return int((dy != 0).any(1).sum())


def wgrad(x, dy, reflect, up=False, dtype=F64):
    """x [B, C, H, W] (half size when up), dy [B, Cout, H, W] -> (dw [Cout, C, 3, 3], its envelope, db [Cout], its envelope)"""
    x, dy = x.to(dtype), dy.to(dtype)

    def grad(xx, d):
        w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=dtype, requires_grad=True)
        return torch.autograd.grad(_conv(xx, w, None, reflect, up), w, d)[0]

    k = ks(support_pixels(dy) + 8)
    return grad(x, dy), k * grad(x.abs(), dy.abs()).double(), dy.sum((0, 2, 3)), k * dy.abs().sum((0, 2, 3)).double()


def outside(got, want64, envelope):
    """elementwise: got is not within the envelope of want64 (a NaN is outside)"""
    return ~((got.double() - want64.double()).abs() <= envelope)


def ratio(got, want64, envelope):
    """elementwise |got - want64| / envelope; 0 where both are 0, inf where only the envelope is (or got is a NaN)"""
    err = (got.double() - want64.double()).abs()
    r = err / envelope
    r = torch.where((envelope == 0) & (err == 0), torch.zeros_like(r), r)
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
