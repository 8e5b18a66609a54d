"""GPU: the image boundary of both networks -- the two 7x7 stride-2 stems reading the NCHW images themselves (mcav_*_desc.x_planar,
csrc/conv_stem.hip kPlanar) and conv1's weight gradient applying bn1's backward formula to its dy tile (mcav_wgrad_desc.dy_bn_*, kBN) --
against the launches they replace, which stay in the library.

Every comparison is bit equality (torch.equal on the int32 view), old path against new path on the same seeded inputs: the folded form runs
the same device function (csrc/bn_bwd_formula.h) on the same values in the same tile walk, so nothing may differ.
"""
import ctypes

import pytest
import torch

from guarded import guard_allocations, guarded_spec
from test_stem_fused_gpu import BN, make_case, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_INVALID = -1
# the whole networks keep torch.empty (the windows would keep every activation alive)
UNGUARDED = ("test_whole_networks_keep_every_gradient_and_buffer_bit_for_bit",)


@pytest.fixture(autouse=True)
def guarded_outputs(request):
    """Every mcav.nn.empty() of a kernel-level test is a NaN-filled window between sentinel bands (tests/guarded.py), checked after the test."""
    if request.node.originalname in UNGUARDED:
        yield
        return
    with guard_allocations() as guards:
        yield
        guards.check()


def depth_spec(seed):
    from mcav import nn as N
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1 * torch.exp(1.5 * torch.randn(64, 1, 1, 1, generator=g))
    return guarded_spec(N.ConvSpec(torch.nn.Parameter(w.to(DEV)), None, 2, 3, 0, smallc=True))


def pose_spec(seed):
    from mcav import nn as N
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(16, 9, 7, 7, generator=g) * 0.1 * torch.exp(1.5 * torch.randn(16, 1, 1, 1, generator=g))
    return guarded_spec(N.ConvSpec(torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(torch.randn(16, generator=g).to(DEV)), 2, 3, 0))


def images(n, Bp, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(Bp, 3, H, W, generator=g) * torch.exp(torch.randn(1, 3, 1, 1, generator=g))).to(DEV).contiguous() for _ in range(n)]


def stacked_nhwc4(imgs):
    from mcav import nn as N
    Bp, _, H, W = imgs[0].shape
    x4 = torch.zeros((len(imgs) * Bp, H, W, 4), device=DEV)
    for i, t in enumerate(imgs):
        N.nchw_to_nhwc(t, 4, x4[i * Bp:(i + 1) * Bp])
    return x4


# B per source x H x W.  1x38x70: output 19 x 35, ragged in both tile dimensions, odd source size, two sources of one image each.
PLANAR_SHAPES = [(1, 38, 70), (2, 64, 128)]


@pytest.mark.parametrize("Bp,H,W", PLANAR_SHAPES)
def test_depth_stem_forward_reads_planar_images_bit_for_bit(Bp, H, W):
    from mcav import nn as N
    imgs, spec = images(2, Bp, H, W, 17 + H), depth_spec(7)
    c_old, slab_old = N.conv_fwd(spec, stacked_nhwc4(imgs), stats=True, groups=2)
    c_new, slab_new = N.conv_fwd(spec, N.PlanarImages(imgs, N.PLANAR_BATCH, 4), stats=True, groups=2)
    c_one = N.conv_fwd(spec, N.PlanarImages(imgs[:1], N.PLANAR_BATCH, 4))                 # a single source, no statistics (eval mode)
    torch.cuda.synchronize()
    assert getattr(spec, "_stem", None) is not None, "the stem launch did not take the patch kernel"
    assert float(c_old.abs().max()) > 0
    print("depth fwd %s: %d of %d elements differ" % ((Bp, H, W), int((c_old.view(torch.int32) != c_new.view(torch.int32)).sum()), c_old.numel()))
    assert same_bits(c_old, c_new) and same_bits(slab_old, slab_new) and same_bits(c_one, c_old[:Bp])


@pytest.mark.parametrize("Bp,H,W", PLANAR_SHAPES)
def test_pose_stem_forward_reads_three_planar_images_bit_for_bit(Bp, H, W):
    from mcav import nn as N
    imgs, spec = images(3, Bp, H, W, 23 + H), pose_spec(9)
    y_old = N.conv_fwd(spec, N.nchw3_to_nhwc(imgs[0], imgs[1], imgs[2], 16), act=N.ACT_RELU)
    y_new = N.conv_fwd(spec, N.PlanarImages(imgs, N.PLANAR_CHANNELS, 16), act=N.ACT_RELU)
    torch.cuda.synchronize()
    assert getattr(spec, "_stem", None) is not None, "the stem launch did not take the patch kernel"
    assert float(y_old.abs().max()) > 0
    print("pose fwd %s: %d of %d elements differ" % ((Bp, H, W), int((y_old.view(torch.int32) != y_new.view(torch.int32)).sum()), y_old.numel()))
    assert same_bits(y_old, y_new)


@pytest.mark.parametrize("Bp,H,W", PLANAR_SHAPES)
def test_both_stem_weight_gradients_read_planar_images_bit_for_bit(Bp, H, W):
    from mcav import nn as N
    Hd, Wd = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(41 + H)
    imgs = images(2, Bp, H, W, 19 + H)
    dy = (torch.randn(2 * Bp, Hd, Wd, 64, generator=g) * torch.exp(torch.randn(1, 1, 1, 64, generator=g))).to(DEV)
    old, new = depth_spec(7), depth_spec(7)
    N.conv_wgrad(old, stacked_nhwc4(imgs), dy)
    N.conv_wgrad(new, N.PlanarImages(imgs, N.PLANAR_BATCH, 4), dy)
    torch.cuda.synchronize()
    assert float(old.weight.grad.abs().max()) > 0 and same_bits(old.weight.grad, new.weight.grad)
    imgs = images(3, Bp, H, W, 29 + H)
    dy = (torch.randn(Bp, Hd, Wd, 16, generator=g) * torch.exp(torch.randn(1, 1, 1, 16, generator=g))).to(DEV)
    old, new = pose_spec(9), pose_spec(9)
    N.conv_wgrad(old, N.nchw3_to_nhwc(imgs[0], imgs[1], imgs[2], 16), dy)
    N.conv_wgrad(new, N.PlanarImages(imgs, N.PLANAR_CHANNELS, 16), dy)
    torch.cuda.synchronize()
    assert float(old.weight.grad.abs().max()) > 0 and float(old.bias.grad.abs().max()) > 0
    assert same_bits(old.weight.grad, new.weight.grad) and same_bits(old.bias.grad, new.bias.grad)


def bn_backward_sums(g, c1, st):
    """-> sums [groups][2][C] of the masked gradient g, as mcav_bn_bwd_finalize leaves them."""
    from mcav import lib as L
    from mcav import nn as N
    h, P = L.lib(), N.P
    n_pix, C, G = c1.shape[0] * c1.shape[1] * c1.shape[2], c1.shape[3], st.groups
    ws = L.workspace(h.mcav_bn_bwd_workspace_bytes(n_pix, C, G), c1.device, "bn_bwd")
    sums, dgamma, dbeta = N.empty((G, 2, C), c1), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    L.check(h.mcav_bn_bwd_reduce(P(g), None, P(c1), P(st.mean), P(st.invstd), 0, n_pix, C, P(dgamma), P(dbeta), 0, P(sums), G, P(ws), ws.numel(),
                                 L.stream()), "mcav_bn_bwd_reduce")
    return sums


# 2x38x70: c1 is 19 x 35, ragged in both tile dimensions.  6x192x256: c1 is 96 x 128 = 576 tiles of 4 x 32, more than the 512 persistent
# workgroups, so some workgroups walk from image 0 to image 5 across the group boundary (groups = 2) and reload their coefficients.
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("B,H,W", [(2, 38, 70), (6, 192, 256)])
def test_depth_stem_wgrad_with_folded_bn_backward_is_bn_bwd_apply_then_wgrad(B, H, W, kind, groups):
    from mcav import lib as L
    from mcav import nn as N
    Hd, Wd = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    c1, st, gamma, beta = make_case(kind, B, Hd, Wd, groups)
    gen = torch.Generator().manual_seed(31 * H + groups)
    x4 = N.nchw_to_nhwc((torch.randn(B, 3, H, W, generator=gen) * torch.exp(torch.randn(1, 3, 1, 1, generator=gen))).to(DEV), 4)
    f0 = N.bn_apply(c1, st, True)
    g = torch.randn(B, Hd, Wd, 64, generator=gen) * torch.exp(1.5 * torch.randn(1, 1, 1, 64, generator=gen))
    if kind == "ties":
        g = torch.round(g * 2) * 0.25
    g = torch.where(f0 > 0, g.to(DEV), torch.zeros((), device=DEV)).contiguous()          # a masked gradient, as the reduce pass leaves it
    bn = BN(gamma, beta)
    sums = bn_backward_sums(g, c1, st)
    h, P = L.lib(), N.P

    old = depth_spec(5)
    dc1 = torch.empty_like(c1)
    L.check(h.mcav_bn_bwd_apply(P(g), None, P(c1), P(bn.weight), P(st.mean), P(st.invstd), P(sums), 0, B * Hd * Wd, 64, P(dc1), None, 0, groups,
                                L.stream()), "mcav_bn_bwd_apply")
    N.conv_wgrad(old, x4, dc1)
    runs = []
    for _ in range(2):
        new = depth_spec(5)
        N.conv_wgrad(new, x4, g, dy_bn=N.DyBn(c1, bn.weight, st.mean, st.invstd, sums, groups))
        runs.append(new.weight.grad)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(old.weight.grad).all()) and float(old.weight.grad.abs().max()) > 0
    n = int((old.weight.grad.view(torch.int32) != runs[0].view(torch.int32)).sum())
    print("%s %s groups=%d: %d of %d gradient elements differ" % (kind, (B, H, W), groups, n, runs[0].numel()))
    assert same_bits(runs[0], old.weight.grad)
    assert same_bits(runs[0], runs[1])                                                   # run to run


def wgrad_desc(spec, x, dy):
    from mcav import nn as N
    d = N.WgradDesc()
    d.x1, d.B, d.Hs, d.Ws, d.C1 = N.P(x), x.shape[0], x.shape[1], x.shape[2], x.shape[3]
    d.kh, d.kw, d.Kp = spec.kh, spec.kw, spec.kp
    d.mode = N.G_SMALLC if spec.smallc else N.G_DIRECT
    d.stride, d.sign, d.offset, d.pad_mode = spec.stride, 1, -spec.pad, spec.pad_mode
    d.dy, d.Hd, d.Wd, d.Cdy = N.P(dy), dy.shape[1], dy.shape[2], dy.shape[3]
    d.Cout, d.Cin = spec.cout, spec.cin
    d.dw_oihw, d.accumulate = N.P(N.grad_buffer(spec.weight)), 1
    return d


def set_bn_fields(d, c1like, coeffs, groups=1):
    from mcav import nn as N
    d.dy_bn_x, d.dy_bn_gamma, d.dy_bn_mean, d.dy_bn_invstd, d.dy_bn_sums = N.P(c1like), N.P(coeffs), N.P(coeffs), N.P(coeffs), N.P(coeffs)
    d.dy_bn_groups, d.dy_bn_inv_count = groups, 1.0 / (c1like.shape[0] * c1like.shape[1] * c1like.shape[2])


def refused(d):
    """The descriptor has no workspace size and mcav_wgrad returns MCAV_E_INVALID before it launches anything (the gradient stays zero)."""
    from mcav import lib as L
    h = L.lib()
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    assert h.mcav_wgrad_workspace_bytes(ctypes.byref(d)) == 0
    rc = h.mcav_wgrad(ctypes.byref(d), ws.data_ptr(), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return rc == E_INVALID and not bool(ws.any())


def test_bn_fields_are_refused_outside_the_depth_stem():
    from mcav import nn as N
    coeffs = torch.ones(2 * 64, device=DEV)
    # a 3x3 layer
    spec = guarded_spec(N.ConvSpec(torch.nn.Parameter(torch.zeros(64, 64, 3, 3, device=DEV)), None, 1, 1, 0))
    x, dy = torch.ones(1, 8, 8, 64, device=DEV), torch.ones(1, 8, 8, 64, device=DEV)
    d = wgrad_desc(spec, x, dy)
    assert N.L.lib().mcav_wgrad_workspace_bytes(ctypes.byref(d)) > 0               # launchable without the fields
    set_bn_fields(d, dy, coeffs)
    assert refused(d) and not bool(spec.weight.grad.any())
    # the depth stem with a bias gradient
    stem = depth_spec(3)
    x4, dy = torch.ones(1, 16, 64, 4, device=DEV), torch.ones(1, 8, 32, 64, device=DEV)
    d = wgrad_desc(stem, x4, dy)
    assert N.L.lib().mcav_wgrad_workspace_bytes(ctypes.byref(d)) > 0
    set_bn_fields(d, dy, coeffs)
    assert N.L.lib().mcav_wgrad_workspace_bytes(ctypes.byref(d)) > 0               # the depth stem takes them ...
    dbias = torch.zeros(64, device=DEV)
    d.dbias = dbias.data_ptr()
    assert refused(d) and not bool(dbias.any()) and not bool(stem.weight.grad.any())   # ... but conv1 has no bias
    # ... and dy must be exactly the 64 channels the coefficients are indexed by: no channel offset into a wider map
    wide = torch.ones(1, 8, 32, 128, device=DEV)
    d = wgrad_desc(stem, x4, wide)
    d.dy_choff = 64
    assert N.L.lib().mcav_wgrad_workspace_bytes(ctypes.byref(d)) > 0               # launchable without the fields
    set_bn_fields(d, wide, coeffs)
    assert refused(d) and not bool(stem.weight.grad.any())


def test_planar_fields_are_refused_outside_the_stems():
    from mcav import lib as L
    from mcav import nn as N
    spec = guarded_spec(N.ConvSpec(torch.nn.Parameter(torch.ones(64, 64, 3, 3, device=DEV)), None, 1, 1, 0))
    x, y = torch.ones(1, 8, 8, 64, device=DEV), torch.zeros(1, 8, 8, 64, device=DEV)
    img = torch.ones(1, 3, 8, 8, device=DEV)
    d = N.IgemmDesc()
    d.x1, d.B, d.Hs, d.Ws, d.C1 = N.P(x), 1, 8, 8, 64
    d.kh, d.kw, d.Np, d.Kp = 3, 3, spec.np, spec.kp
    d.mode, d.stride, d.sign, d.offset, d.pad_mode = N.G_DIRECT, 1, 1, -1, N.PAD_ZERO
    d.y, d.Hd, d.Wd, d.Cd, d.n_begin, d.n_count = N.P(y), 8, 8, 64, 0, 64
    d.w, d.groups = N.P(spec.packed_fwd()), 1
    h = L.lib()
    assert h.mcav_igemm_mtiles(ctypes.byref(d)) > 0                                  # launchable without the fields
    d.x_planar[0], d.planar_B, d.planar_stack = N.P(img), 1, N.PLANAR_BATCH
    assert h.mcav_igemm_mtiles(ctypes.byref(d)) == E_INVALID
    rc = h.mcav_igemm(ctypes.byref(d), L.stream())
    torch.cuda.synchronize()
    assert rc == E_INVALID and not bool(y.any())
    # ... and on a 3x3 weight gradient
    dy = torch.ones(1, 8, 8, 64, device=DEV)
    w = wgrad_desc(spec, x, dy)
    w.x_planar[0], w.planar_B, w.planar_stack = N.P(img), 1, N.PLANAR_BATCH
    assert refused(w) and not bool(spec.weight.grad.any())


SWITCHES = ("STEM_WGRAD_BN", "STEM_PLANAR")


def run_networks(on):
    """One forward and backward of DispResNet(18).forward_pair + PoseNet at 2 x 64 x 128 -> {name: tensor} of every gradient and BatchNorm buffer."""
    from losses import Losses
    from mcav import nn as N
    from mcav.streams import Branch
    from models.depth.resnet_dispnet import DispResNet
    from models.pose.pose_net import PoseNet
    from oracle.step import synthetic_batch
    saved = {k: getattr(N, k) for k in SWITCHES}
    N.LAUNCHES.clear()
    try:
        for k in SWITCHES:
            setattr(N, k, on)
        torch.manual_seed(11)
        dnet, pnet = DispResNet(18), PoseNet()
        pnet.init_weights()
        dnet.to(DEV).train(); pnet.to(DEV).train()
        s = synthetic_batch(2, 64, 128, seed=7)
        tgt, refs, K = s["tgt"].to(DEV), [r.to(DEV) for r in s["ref_imgs"]], s["intrinsics"].to(DEV)
        branch = Branch()
        poses = branch.fork(pnet, tgt, refs)
        disps = list(dnet.forward_pair(tgt, refs[0]))
        poses = branch.join(poses)
        loss = Losses().forward(tgt, refs, disps, poses, K, None)
        sum(loss).backward()
        torch.cuda.synchronize()
        out = {}
        for tag, net in (("depth", dnet), ("pose", pnet)):
            for name, p in net.named_parameters():
                if p.grad is not None:                                                  # (the encoder's unused fc has none)
                    out["%s.%s.grad" % (tag, name)] = p.grad.detach().clone()
            for name, b in net.named_buffers():
                out["%s.%s" % (tag, name)] = b.detach().clone()
        out["loss"] = torch.stack([l.detach() for l in loss])
        # the forms under test were the ones launched (one stacked depth pass, one pose pass): nothing fell back to the launches they replace
        want = {"wgrad_dy_bn": 1, "fwd_planar": 2, "wgrad_planar": 2} if on else {}
        assert dict(N.LAUNCHES) == want, dict(N.LAUNCHES)
        return out
    finally:
        for k, v in saved.items():
            setattr(N, k, v)


def test_whole_networks_keep_every_gradient_and_buffer_bit_for_bit():
    off, on = run_networks(False), run_networks(True)
    assert off.keys() == on.keys() and len(off) > 100
    differing = [k for k in off if not same_bits(off[k], on[k])]
    print("%d tensors compared, differing: %s" % (len(off), differing))
    assert not differing
    assert float(off["depth.encoder.encoder.conv1.weight.grad"].abs().max()) > 0 and float(off["pose.conv1.0.weight.grad"].abs().max()) > 0
