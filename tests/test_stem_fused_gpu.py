"""GPU: the fused stem kernels (csrc/stem_ops.hip) against the separate passes they stand for, which stay in the library.

forward   mcav_stem_bn_relu_pool_fwd        ==  mcav_bn_apply(ReLU) -> mcav_maxpool3s2_fwd                      (bit for bit: f0, p0, idx)
backward  mcav_stem_pool_bn_bwd_reduce      ~   mcav_maxpool3s2_bwd(accumulate) -> mcav_bn_bwd_reduce(relu)      (dgamma, dbeta, sums)
          mcav_stem_pool_bn_bwd_apply, or the masked gradient left by the reduce pass + mcav_bn_bwd_apply(relu = 0)  ~  mcav_bn_bwd_apply(relu)

The backward results are held to a float64 evaluation of the same formulas from the same device tensors: the fused error is at most 1.5x the
separate chain's, or 5e-7 of the tensor's largest magnitude (the rule of tests/test_split_gpu.py for a kernel that replaces another).  On top
of that the ReLU mask recomputed from c1, scale and shift is asserted to be the bit (f0 > 0) on every element, and with the separate chain's
sums the fused second pass must reproduce its dc1 bit for bit (same gather, same per-element formula).
Inputs: normal c1 with a log-normal scale per channel; c1 quantised to a few values with power-of-two coefficients, so that whole windows tie
and many pre-activations sit exactly on the ReLU edge; NaN and +-inf planted in c1 and a zero scale (inf * 0), forward only.
"""
import pytest
import torch

from conftest import rel_err
from conv_plan_cases import recorded_routes
from guarded import guard_allocations

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 64
UNGUARDED = ()          # (no whole-network test in this module)
SHAPES = [(2, 17, 23), (4, 96, 320)]          # ragged last window row and column; the benchmark's map at a third of its batch


@pytest.fixture(autouse=True)
def guarded_outputs(request):
    """Every mcav.nn.empty() of a kernel-level test is a NaN-filled window between sentinel bands (tests/guarded.py), checked after the test."""
    if request.node.originalname in UNGUARDED:
        yield
        return
    with guard_allocations() as guards:
        yield
        guards.check()


def no_worse(err_fused, err_separate, floor=5e-7):
    """tests/test_split_gpu.py's rule for a kernel that replaces another: within 1.5x of its error, or under a floor of a few ulp."""
    return err_fused <= max(1.5 * err_separate, floor)


class BN:
    """What mcav.nn's BatchNorm calls read of a holder: weight and bias with .grad."""

    def __init__(self, gamma, beta):
        self.weight, self.bias = torch.nn.Parameter(gamma.clone()), torch.nn.Parameter(beta.clone())


def make_case(kind, B, H, W, groups):
    """-> (c1 NHWC, BNState with [groups][C] coefficients, gamma, beta), all on the GPU."""
    from mcav import nn as N
    g = torch.Generator().manual_seed(1000 * H + 10 * groups + len(kind))
    c1 = torch.randn(B, H, W, C, generator=g) * torch.exp(1.5 * torch.randn(1, 1, 1, C, generator=g))
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    if kind == "ties":
        c1 = torch.round(torch.randn(B, H, W, C, generator=g) * 1.2) * 0.5          # -2 .. 2 in steps of 0.5: equal windows everywhere
    xg = c1.double().reshape(groups, -1, C)
    mean, var = xg.mean(1), xg.var(1, unbiased=False)
    invstd = (1.0 / torch.sqrt(var + 1e-5)).float()
    mean = mean.float()
    scale = gamma[None] * invstd
    shift = beta[None] - mean * scale
    if kind == "ties":
        # exact products and sums: x * scale + shift lands on 0 for a fifth of the elements (and on both sides of it)
        scale = torch.tensor([2.0, 0.5, 1.0, 4.0]).repeat(groups, C // 4).contiguous()
        shift = (torch.tensor([-1.0, 0.25, 0.0, 2.0, -0.5, 0.5, 1.0, -2.0]).repeat(groups, C // 8) * (1 + torch.arange(groups)[:, None])).contiguous()
    if kind == "nonfinite":
        flat = c1.view(-1)
        where = torch.randperm(flat.numel(), generator=g)[:3 * 97]
        flat[where[0::3]] = float("nan")
        flat[where[1::3]] = float("inf")
        flat[where[2::3]] = float("-inf")
        c1[0, 0, 0, :8] = float("nan")                                               # a corner window that starts with NaN
        c1[-1, H - 1, W - 1, 8:16] = float("inf")
        scale = scale.clone()
        scale[:, 5] = 0.0                                                            # inf * 0 = NaN inside the BatchNorm expression
    st = N.BNState()
    buf = torch.stack([scale, shift, mean, invstd]).to(DEV).contiguous()
    st.scale, st.shift, st.mean, st.invstd = buf[0], buf[1], buf[2], buf[3]
    st.groups = groups
    return c1.to(DEV).contiguous(), st, gamma.to(DEV), beta.to(DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def separate_forward(c1, st):
    from mcav import nn as N
    f0 = N.bn_apply(c1, st, True)
    p0, idx = N.maxpool_fwd(f0)
    return f0, p0, idx


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["normal", "ties", "nonfinite"])
def test_fused_forward_is_bit_identical_to_bn_apply_then_maxpool(kind, shape, groups):
    from mcav import nn as N
    c1, st, _, _ = make_case(kind, *shape, groups)
    f0, p0, idx = separate_forward(c1, st)
    g0, q0, jdx = N.stem_bn_relu_pool_fwd(c1, st)
    h0, r0, kdx = N.stem_bn_relu_pool_fwd(c1, st)
    torch.cuda.synchronize()
    if kind == "ties":                                                               # the case is what it claims to be
        C4 = (c1.reshape(groups, -1, C) * st.scale[:, None] + st.shift[:, None]) == 0
        assert float(C4.float().mean()) > 0.05 and int(idx.max()) == 8 and float((idx == 0).float().mean()) > 0.2
    if kind == "nonfinite":
        assert bool(torch.isinf(p0).any())
    for name, a, b in (("f0", f0, g0), ("p0", p0, q0), ("idx", idx, jdx)):
        n = int((bits(a) != bits(b)).sum())
        print("%s %s %s groups=%d: %d of %d elements differ" % (kind, shape, name, groups, n, a.numel()))
        assert same_bits(a, b), name
    assert same_bits(g0, h0) and same_bits(q0, r0) and same_bits(jdx, kdx)          # run to run


def reference_backward(c1, st, gamma, f0, idx, dy0, dp0):
    """float64 on the CPU, from the device tensors: -> (dgamma, dbeta, dc1)."""
    B, H, W, _ = c1.shape
    G = st.groups
    Ho, Wo = idx.shape[1], idx.shape[2]
    dp, ix = dp0.double().cpu(), idx.cpu()
    gp = torch.zeros(B, 2 * Ho + 2, 2 * Wo + 2, C, dtype=torch.float64)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        gp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += dp * (ix == tap)               # padded row 2 oy + ky = input row 2 oy - 1 + ky, plus one
    dz = (dy0.double().cpu() + gp[:, 1:H + 1, 1:W + 1]) * (f0.cpu() > 0)
    dz = dz.reshape(G, -1, C)
    n = dz.shape[1]
    mean, invstd = st.mean.double().cpu()[:, None], st.invstd.double().cpu()[:, None]
    xh = (c1.double().cpu().reshape(G, -1, C) - mean) * invstd
    s1, s2 = dz.sum(1, keepdim=True), (dz * xh).sum(1, keepdim=True)
    dc1 = (gamma.double().cpu() * invstd) * (dz - s1 / n - xh * (s2 / n))
    return s2.sum(0)[0], s1.sum(0)[0], dc1.reshape(c1.shape)


def separate_backward(c1, st, gamma, beta, f0, idx, dy0, dp0):
    """The chain that stays in the library, call by call -> (dgamma, dbeta, sums, dc1)."""
    from mcav import lib as L
    from mcav import nn as N
    B, H, W, _ = c1.shape
    h, P = L.lib(), N.P
    n_pix, G = B * H * W, st.groups
    df0 = N.maxpool_bwd(dp0, idx, tuple(c1.shape), dx=dy0.clone(), accumulate=True)
    ws = L.workspace(h.mcav_bn_bwd_workspace_bytes(n_pix, C, G), c1.device, "bn_bwd")
    sums, dgamma, dbeta = N.empty((G, 2, C), c1), torch.zeros_like(gamma), torch.zeros_like(beta)
    L.check(h.mcav_bn_bwd_reduce(P(df0), P(f0), P(c1), P(st.mean), P(st.invstd), 1, n_pix, C, P(dgamma), P(dbeta), 1, P(sums), G, P(ws), ws.numel(),
                                 L.stream()), "mcav_bn_bwd_reduce")
    dc1 = torch.empty_like(c1)
    L.check(h.mcav_bn_bwd_apply(P(df0), P(f0), P(c1), P(gamma), P(st.mean), P(st.invstd), P(sums), 1, n_pix, C, P(dc1), None, 0, G, L.stream()),
            "mcav_bn_bwd_apply")
    return dgamma, dbeta, sums, dc1


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_fused_backward_matches_float64_as_the_separate_chain_does(kind, shape, groups):
    from mcav import lib as L
    from mcav import nn as N
    B, H, W = shape
    c1, st, gamma, beta = make_case(kind, B, H, W, groups)
    f0, p0, idx = separate_forward(c1, st)
    g = torch.Generator().manual_seed(7 + H)
    dy0 = (torch.randn(B, H, W, C, generator=g) * torch.exp(1.5 * torch.randn(1, 1, 1, C, generator=g))).to(DEV)
    dp0 = (torch.randn(p0.shape, generator=g) * torch.exp(1.5 * torch.randn(1, 1, 1, C, generator=g))).to(DEV)
    h, P = L.lib(), N.P

    # the mask the fused passes recompute is the stored activation's sign bit: a gradient of ones through the reduce pass comes back as the mask
    ones, zeros, scratch = torch.ones_like(c1), torch.zeros_like(p0), BN(gamma, beta)
    N.stem_pool_bn_backward(scratch, st, ones, zeros, idx, c1, regather=False)
    assert bool(torch.equal(ones != 0, f0 > 0)), "recomputed ReLU mask differs from (f0 > 0)"
    assert bool(((ones == 0) | (ones == 1)).all())

    want = reference_backward(c1, st, gamma, f0, idx, dy0, dp0)
    sgamma, sbeta, ssums, sdc1 = separate_backward(c1, st, gamma, beta, f0, idx, dy0, dp0)
    runs = {}
    for regather in (False, True):
        for rep in range(2):
            bn, dy = BN(gamma, beta), dy0.clone()
            dc1 = N.stem_pool_bn_backward(bn, st, dy, dp0, idx, c1, regather=regather)
            runs[regather, rep] = (bn.weight.grad, bn.bias.grad, dc1)
            if regather:
                assert same_bits(dy, dy0)                                           # this form leaves the incoming gradient untouched
        assert all(same_bits(a, b) for a, b in zip(runs[regather, 0], runs[regather, 1])), "two runs differ (regather=%s)" % regather
    torch.cuda.synchronize()
    for regather in (False, True):
        for name, got, sep, ref in zip(("dgamma", "dbeta", "dc1"), runs[regather, 0], (sgamma, sbeta, sdc1), want):
            e_fused, e_sep = rel_err(got, ref), rel_err(sep, ref)
            print("%s %s groups=%d regather=%d %s: fused %.3g separate %.3g (relative to max |ref|), bit-equal %s"
                  % (kind, shape, groups, regather, name, e_fused, e_sep, same_bits(got, sep)))
            assert no_worse(e_fused, e_sep), (name, regather, e_fused, e_sep)

    # with the separate chain's sums the second pass is the same per-element formula on the same gathered, masked gradient
    dc1 = torch.empty_like(c1)
    L.check(h.mcav_stem_pool_bn_bwd_apply(P(dy0), P(dp0), P(idx), P(c1), P(st.scale), P(st.shift), P(gamma), P(st.mean), P(st.invstd), P(ssums),
                                          B, H, W, C, groups, P(dc1), L.stream()), "mcav_stem_pool_bn_bwd_apply")
    assert same_bits(dc1, sdc1), "second pass with the separate chain's sums: %d elements differ" % int((bits(dc1) != bits(sdc1)).sum())
    # ... and the masked gradient the reduce pass leaves is the one the separate chain masks on the fly: elements that received a pooled
    # gradient agree, ties included
    dz = dy0.clone()
    N.stem_pool_bn_backward(BN(gamma, beta), st, dz, dp0, idx, c1, regather=False)
    df0 = N.maxpool_bwd(dp0, idx, tuple(c1.shape), dx=dy0.clone(), accumulate=True)
    assert same_bits(dz, torch.where(f0 > 0, df0, torch.zeros_like(df0)))


def test_fused_stem_refuses_other_widths():
    from mcav import lib as L
    from mcav import nn as N
    x = torch.zeros(1, 4, 4, 32, device=DEV)
    st = N.BNState()
    st.scale = st.shift = torch.zeros(1, 32, device=DEV)
    st.groups = 1
    assert not N.stem_fusable(32)
    with pytest.raises(L.MCAVError):
        N.stem_bn_relu_pool_fwd(x, st)


STEM_LEAN = 1 << 16          # desc.tile bit 16: the depth stem with the shared 4-byte-store epilogue


@pytest.mark.parametrize("B,H,W", [(2, 45, 70), (4, 192, 640)])
def test_stem_wide_store_epilogue_writes_the_lean_epilogues_bits(B, H, W):
    """csrc/conv_stem.hip stem_epilogue_wide: the same accumulators, transposed across lane quads for 16-byte stores -> c1 bit-equal; the
    statistics are summed before the transpose in the lean epilogue's order -> slab rows held to float64 as the lean epilogue's are."""
    from mcav import nn as N
    g = torch.Generator().manual_seed(29 + H)
    x = torch.randn(B, 3, H, W, generator=g) * torch.exp(torch.randn(1, 3, 1, 1, generator=g))
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1 * torch.exp(1.5 * torch.randn(64, 1, 1, 1, generator=g))
    spec = N.ConvSpec(torch.nn.Parameter(w.to(DEV)), None, 2, 3, 0, smallc=True)
    x4 = N.nchw_to_nhwc(x.to(DEV), 4)
    with recorded_routes(N) as routes:
        lean, slab_lean = N.conv_fwd(spec, x4, stats=True, groups=2, tile=STEM_LEAN)
        wide, slab_wide = N.conv_fwd(spec, x4, stats=True, groups=2)
        again, slab_again = N.conv_fwd(spec, x4, stats=True, groups=2)
        plain = N.conv_fwd(spec, x4)                                                 # without statistics (eval mode)
    assert [(k, r.family, r.variant) for k, r in routes] == [("fwd", N.IGEMM_STEM, N.RV_LEAN)] + [("fwd", N.IGEMM_STEM, 0)] * 3      # bit 16 forces the lean epilogue
    torch.cuda.synchronize()
    assert getattr(spec, "_stem", None) is not None, "the stem launch did not take the patch kernel"
    assert H % 2 == 0 or (wide.shape[1] % 8 and wide.shape[2] % 32), "the odd case has ragged tiles both ways"
    print("c1 %s: %d of %d elements differ; slab bit-equal %s" % ((B, H, W), int((bits(lean) != bits(wide)).sum()), lean.numel(), same_bits(slab_lean, slab_wide)))
    assert same_bits(lean, wide) and same_bits(wide, again) and same_bits(slab_wide, slab_again) and same_bits(wide, plain)
    assert same_bits(slab_lean, slab_wide)          # more than the float64 rule below asks: with it a whole training step keeps its bits
    y = lean.double().cpu()                                                          # what both epilogues summed: the stored c1
    mt = slab_lean.shape[0] // 2
    for grp in range(2):
        part = y[grp * (B // 2):(grp + 1) * (B // 2)]
        for which, ref in enumerate((part.sum((0, 1, 2)), (part ** 2).sum((0, 1, 2)))):
            tot = lambda s: s[grp * mt:(grp + 1) * mt, which].double().sum(0).cpu()
            assert no_worse(rel_err(tot(slab_wide), ref), rel_err(tot(slab_lean), ref))
