"""GPU: the descriptor contract of the convolution ABI (include/mcav_conv.h), kernel form by kernel form, through mcav_igemm / mcav_wgrad
themselves on descriptors built here.

  * A launch "computes filter rows [n_begin, n_begin + n_count) and writes them to channels [y_choff, y_choff + n_count) of y, whose pixel stride
    is Cd floats", with dact_aux / addend in y's layout.  y is allocated as the whole [B, Hd, Wd, Cd] (the pooled size with pool) inside a
    Guarded window (tests/guarded.py) that starts as NaN sentinels: the channels of the launch must equal the float64 reference, every other
    channel of every pixel must still hold the sentinel BITS, and the bands around the window must be intact.  A form that does not support a
    sub-range has to hand the launch to one that does (or refuse it, y untouched): a wrong or partial result is the failure.
  * mcav_wgrad with accumulate = 0 must store every OIHW element of its input-channel window [ci_offset, ci_offset + Cin) of
    [Cout][Cin_total][kh][kw] and nothing else; with accumulate = 1 it adds into what is there; dy is read at [dy_choff, dy_choff + Cout) of Cdy.
  * Descriptors the kernels cannot honour are refused by the planner entries first (which launch nothing) and only then handed to the launch
    entries, which must answer MCAV_E_INVALID and leave the outputs untouched (tests/conv_contract_cases.py).

References are float64 torch on the CPU; for mma = 1 on operands rounded to bf16 (as tests/test_bf16_gpu.py).  Tolerances are the suite's own
through conftest.rel_err: 2e-5 forward / data gradient, 5e-5 weight / bias gradient, 2e-5 for bf16 against its rounded-operand reference (the
reflection adjoint's border pixels at 1e-2, the inner ones at 2e-5: test_bf16_gpu.py's statement), and for the split forms (mma = 2 / 3) the
rule of test_split_conv_fwd_dgrad_wgrad_match_float64_as_the_fp32_kernels_do: below 3e-6 and no worse than the fp32 kernel on the same launch.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_contract_cases as K
from conftest import rel_err
from guarded import Guarded, P, band_for, is_sentinel
from test_bf16_gpu import r16, ref_conv64
from test_split_gpu import no_worse, rms_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_INVALID = K.E_INVALID


def window(shape, init=None):
    return Guarded(shape, init=init, band=band_for(shape))


def to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def dev_nhwc(t):
    return to_nhwc(t.float()).to(DEV)


def elu_d(aux):
    """act'(aux) of MCAV_ACT_ELU as a function of the OUTPUT"""
    return torch.where(aux > 0, torch.ones_like(aux), aux + 1)


# ================================================================================================ C1: sub-range stores
class Form:
    """One launch family: kind 'fwd' (filter rows = output channels) or 'dgrad' (filter rows = the convolution's input channels).
    conv = (B, H, W, Cin, Cout, k, stride, pad, pad_mode) with H x W the convolution's INPUT; up = (C1, C2): the input is cat(up2(a), skip)."""

    def __init__(self, name, kind, conv, n_count, Cd, n_begins, choffs, mma=0, tile=0, pool=0, up=None, stored=None, inner=False):
        self.name, self.kind, self.conv, self.n_count, self.Cd, self.n_begins, self.choffs = name, kind, conv, n_count, Cd, n_begins, choffs
        self.mma, self.tile, self.pool, self.up, self.stored, self.inner = mma, tile, pool, up, stored, inner


Z, R = 0, 1          # pad modes
FORMS = [
    # DIRECT table kernels with the lean epilogue: 32 -> 64 at 2 x 6 x 10, 32 rows into a 64-channel pixel (auto = 128 x 32 tiles)
    Form("direct tile0", "fwd", (2, 6, 10, 32, 64, 3, 1, 1, Z), 32, 64, (0, 32), (0, 16, 32)),
    Form("direct tile2", "fwd", (2, 6, 10, 32, 64, 3, 1, 1, Z), 32, 64, (0, 32), (0, 16, 32), tile=2),
    Form("direct tile10", "fwd", (2, 6, 10, 32, 64, 3, 1, 1, Z), 32, 64, (0, 32), (0, 16, 32), tile=10),
    Form("direct tile12", "fwd", (2, 6, 10, 32, 64, 3, 1, 1, Z), 32, 64, (0, 32), (0, 16, 32), tile=12),
    # the same launch on the general kernels (bit 8) and their pointer-store epilogue
    Form("general tile0", "fwd", (2, 6, 10, 32, 64, 3, 1, 1, Z), 32, 64, (0, 32), (0, 16, 32), tile=0x100),
    Form("general tile2", "fwd", (2, 6, 10, 32, 64, 3, 1, 1, Z), 32, 64, (0, 32), (0, 16, 32), tile=0x102),
    # a source that is no multiple of 4 channels: ONE stored channel of Kp = 16 (the generic gather)
    Form("one stored channel", "fwd", (2, 7, 11, 1, 32, 3, 1, 1, Z), 16, 48, (0, 16), (0, 16, 32), stored=1),
    # the reflection adjoint: table kernel with its border wavefronts, and the general kernel
    Form("reflect adjoint", "dgrad", (2, 6, 10, 64, 64, 3, 1, 1, R), 32, 64, (0, 32), (0, 16, 32)),
    Form("reflect adjoint general", "dgrad", (2, 6, 10, 64, 64, 3, 1, 1, R), 32, 64, (0, 32), (0, 16, 32), tile=0x100),
    # the stride-2 adjoint on odd sizes: all four parity classes ragged (dy is 1 x 5 x 6)
    Form("stride-2 adjoint", "dgrad", (1, 9, 11, 128, 64, 3, 2, 1, Z), 64, 96, (0, 32), (0, 16, 32)),
    # pooled data gradient of a decoder level (y is the pooled 2 x 3 x 5)
    Form("pooled dgrad", "dgrad", (2, 6, 10, 96, 32, 3, 1, 1, R), 32, 48, (0, 32), (0, 16), pool=1),
    Form("pooled dgrad general", "dgrad", (2, 6, 10, 96, 32, 3, 1, 1, R), 32, 48, (0, 32), (0, 16), pool=1, tile=0x100),
    # merged-tap forward: a of 32 channels stored at 5 x 7, skip of 64 at 10 x 14, 32 rows into Cd = 48
    Form("merged-tap forward", "fwd", (2, 10, 14, 96, 32, 3, 1, 1, R), 32, 48, (0,), (0, 16), up=(32, 64)),
    # bf16 MFMA kernels (mma = 1): zero padding, and the reflection adjoint
    Form("bf16 zero pad", "fwd", (2, 12, 20, 64, 128, 3, 1, 1, Z), 64, 96, (32, 0), (32, 0, 16), mma=1),
    Form("bf16 reflect adjoint", "dgrad", (2, 6, 10, 64, 64, 3, 1, 1, R), 32, 64, (0, 32), (0, 16, 32), mma=1, inner=True),
    # the split forms: the patch kernel (mma = 2) and the table kernels (mma = 3, the 1x1 stride-2 downsample on odd sizes)
    Form("split patch", "fwd", (2, 12, 20, 64, 128, 3, 1, 1, Z), 64, 96, (32, 0), (32, 0, 16), mma=2),
    Form("split table", "fwd", (2, 9, 15, 64, 128, 1, 2, 0, Z), 64, 96, (32, 0), (32, 0, 16), mma=3),
    # the fp32 patch-in-LDS kernel (bit 13)
    Form("fp32 patch", "fwd", (2, 12, 20, 64, 128, 3, 1, 1, Z), 64, 96, (32, 0), (32, 0, 16), tile=1 << 13),
    # halo shapes: the halo kernels refuse y_choff != 0 (the table kernel must then get it right) and take Cd > n_count with y_choff = 0
    Form("halo forward", "fwd", (2, 9, 35, 16, 16, 3, 1, 1, R), 16, 48, (0,), (16, 0, 32)),
    Form("halo adjoint", "dgrad", (2, 4, 16, 32, 16, 3, 1, 1, R), 32, 48, (0,), (0, 16)),
    Form("halo adjoint, second half of the rows", "dgrad", (2, 4, 16, 32, 16, 3, 1, 1, R), 16, 48, (16,), (0, 32)),
]


class Case:
    """The operands of a Form on both sides: float64 reference rows [B, Hy, Wy, Nall] (NHWC, before the epilogue) and the device tensors."""

    def __init__(self, f):
        from mcav import nn as N
        B, H, W, Cin, Cout, k, stride, pad, pm = f.conv
        g = torch.Generator().manual_seed(sum(f.conv) + 7 * len(f.name))
        self.f = f
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
        self.bias = 0.1 * torch.randn(Cout, generator=g)
        rnd = r16 if f.mma == 1 else (lambda t: t.double())
        self.a = self.skip = None
        if f.up is not None:                                   # x = cat(up2(a), skip): a is what the launch reads at half the size
            C1, C2 = f.up
            a = torch.randn(B, C1, H // 2, W // 2, generator=g)
            x = torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), x[:, C1:]], 1)
            self.a, self.skip = dev_nhwc(a), dev_nhwc(x[:, C1:])
        if f.kind == "fwd":
            self.rows = to_nhwc(ref_conv64(rnd(x), rnd(w), None, stride, pad, pm))
            self.src = dev_nhwc(x[:, :f.stored] if f.stored else x)
        else:
            Ho, Wo = N.out_size(H, k, stride, pad), N.out_size(W, k, stride, pad)
            dy = torch.randn(B, Cout, Ho, Wo, generator=g)
            xr = x.double().requires_grad_()
            ref_conv64(xr, rnd(w), None, stride, pad, pm).backward(rnd(dy))
            gx = xr.grad
            if f.pool:
                gx = F.avg_pool2d(gx, 2) * 4
            self.rows = to_nhwc(gx)
            self.src = dev_nhwc(dy)
        self.spec = N.ConvSpec(torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(self.bias.to(DEV)) if f.kind == "fwd" else None, stride, pad, pm)
        yshape = tuple(self.rows.shape[:3]) + (f.Cd,)
        self.yshape = yshape
        self.aux = torch.randn(yshape, generator=g)
        self.add = torch.randn(yshape, generator=g)
        self.aux_d, self.add_d = self.aux.to(DEV), self.add.to(DEV)

    def desc(self, y, n_begin, choff, epi, mma):
        from mcav import nn as N
        f, spec = self.f, self.spec
        B, H, W, Cin, Cout, k, stride, pad, pm = f.conv
        d = N.IgemmDesc()
        if f.kind == "fwd":
            if f.up is not None:
                d.x1, d.x2, d.C1, d.C2, d.up1 = P(self.a), P(self.skip), f.up[0], f.up[1], 1
            else:
                d.x1, d.C1 = P(self.src), self.src.shape[3]
            d.B, d.Hs, d.Ws = B, H, W
            d.kh, d.kw, d.Np, d.Kp = k, k, spec.np, spec.kp
            d.mode, d.stride, d.sign, d.offset, d.pad_mode = N.G_DIRECT, stride, 1, -pad, pm
            d.Hd, d.Wd = N.out_size(H, k, stride, pad), N.out_size(W, k, stride, pad)
            d.bias, d.act = P(spec.bias), N.ACT_ELU
        else:
            d.x1, d.B, d.Hs, d.Ws, d.C1 = P(self.src), B, self.src.shape[1], self.src.shape[2], Cout
            d.kh, d.kw, d.Np, d.Kp = k, k, N.up16(Cin), N.up16(Cout)
            if stride == 1 and pm == R:
                d.mode, d.stride, d.sign, d.offset = N.G_ADJ_REFLECT, 1, -1, 1
            elif stride == 1:
                d.mode, d.stride, d.sign, d.offset = N.G_DIRECT, 1, -1, pad
            else:
                d.mode, d.stride, d.sign, d.offset = N.G_ADJ_STRIDE2, 2, -1, pad
            d.pad_mode = N.PAD_ZERO
            d.Hd, d.Wd = H, W
        d.y, d.Cd, d.n_begin, d.n_count, d.y_choff = P(y), f.Cd, n_begin, f.n_count, choff
        d.pool, d.tile, d.groups = f.pool, f.tile, 1
        if epi:
            d.dact_aux, d.dact, d.addend = P(self.aux_d), N.ACT_ELU, P(self.add_d)
        spec.mma = mma
        N._weights_for(spec, d, f.kind == "dgrad")
        if f.up is not None:
            d.w_upmerge = P(spec.packed_upmerge(f.up[0]))
        return d

    def want(self, n_begin, choff, epi):
        f = self.f
        v = self.rows[..., n_begin:n_begin + f.n_count]
        if f.kind == "fwd":
            v = F.elu(v + self.bias[n_begin:n_begin + f.n_count].double())
        if epi:
            v = v * elu_d(self.aux[..., choff:choff + f.n_count].double()) + self.add[..., choff:choff + f.n_count].double()
        return v

    def launch(self, n_begin, choff, epi, mma):
        """-> (the launch's channels of y on the CPU, the descriptor); asserts the return code, the bands and the untouched channels"""
        from mcav import lib as L
        f = self.f
        y = window(self.yshape)
        d = self.desc(y, n_begin, choff, epi, mma)
        assert L.lib().mcav_igemm_mtiles(ctypes.byref(d)) > 0, "the planner refuses a sub-range that lies inside y"
        rc = L.lib().mcav_igemm(ctypes.byref(d), L.stream())
        torch.cuda.synchronize()
        what = "%s n_begin=%d y_choff=%d epilogue=%d mma=%d" % (f.name, n_begin, choff, epi, mma)
        assert rc == 0, "%s: mcav_igemm returned %d" % (what, rc)
        assert y.intact(), "%s: wrote outside y" % what
        got = y.cpu()
        other = torch.ones(f.Cd, dtype=torch.bool)
        other[choff:choff + f.n_count] = False
        stray = int((~is_sentinel(got[..., other])).sum())
        assert stray == 0, "%s: %d elements outside channels [%d, %d) were stored" % (what, stray, choff, choff + f.n_count)
        return got[..., choff:choff + f.n_count], d


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name.replace(" ", "_").replace(",", ""))
def test_sub_range_stores(form):
    from mcav import lib as L
    c = Case(form)
    f = form
    for n_begin in f.n_begins:
        for choff in f.choffs:
            for epi in (0, 1):
                want = c.want(n_begin, choff, epi)
                got, d = c.launch(n_begin, choff, epi, f.mma)
                left = int(is_sentinel(got).sum())
                what = "%s n_begin=%d y_choff=%d epilogue=%d" % (f.name, n_begin, choff, epi)
                assert left == 0, "%s: %d elements of the launch's channels were never stored" % (what, left)
                err = rel_err(got, want)
                print("%-28s n_begin %2d y_choff %2d epilogue %d: rel_err %.2e" % (f.name, n_begin, choff, epi, err))
                if f.mma in (1, 2, 3):
                    assert L.lib().mcav_igemm_uses_bf16(ctypes.byref(d)) == 1, "%s: the launch left the bf16 MFMA kernels" % what
                if f.mma >= 2:
                    got32, _ = c.launch(n_begin, choff, epi, 0)                 # the same launch on the fp32 MFMA kernels
                    e32 = rel_err(got32, want)
                    assert err < 3e-6, (what, err, e32)
                    assert no_worse(err, e32) or rms_err(got, want) <= 1.25 * rms_err(got32, want), (what, err, e32)
                elif f.inner:                                                   # bf16 reflection adjoint: border sources are summed before the rounding
                    H, W = want.shape[1], want.shape[2]
                    assert rel_err(got[:, 2:H - 2, 2:W - 2], want[:, 2:H - 2, 2:W - 2]) < 2e-5, what
                    assert err < 1e-2, what
                else:
                    assert err < 2e-5, (what, err)


# ================================================================================================ C2: K-split finish
@pytest.mark.parametrize("combo", ["aux", "addend", "both", "both, factor after the addend"])
def test_ksplit_finish_epilogue(combo):
    """The data gradient of a 256 -> 256 3x3 stride-2 layer at 3 x 3 x 10 (PoseNet conv6 / 7): a handful of tiles with a long K loop, cut over
    several workgroups per tile; splitk_finish_kernel sums the partials and applies the epilogue.  Two timed dispatches = the K-split ran."""
    from mcav import lib as L
    from mcav import nn as N
    B, H, W, C = 3, 3, 10, 256
    g = torch.Generator().manual_seed(61)
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
    dy = torch.randn(B, C, 2, 5, generator=g)
    aux, add = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g)
    xr = torch.zeros(B, C, H, W, dtype=torch.float64).requires_grad_()
    ref_conv64(xr, w, None, 2, 1, 0).backward(dy.double())
    want = to_nhwc(xr.grad)
    use_aux, use_add, after = combo != "addend", combo != "aux", combo.endswith("addend") and combo != "addend"
    if use_aux and not after:
        want = want * elu_d(aux.double())
    if use_add:
        want = want + add.double()
    if after:
        want = want * elu_d(aux.double())
    spec = N.ConvSpec(torch.nn.Parameter(w.to(DEV)), None, 2, 1, 0)
    dyd, auxd, addd = dev_nhwc(dy), aux.to(DEV), add.to(DEV)
    y = window((B, H, W, C))
    d = N.IgemmDesc()
    d.x1, d.B, d.Hs, d.Ws, d.C1 = P(dyd), B, 2, 5, C
    d.kh, d.kw, d.Np, d.Kp = 3, 3, C, C
    d.mode, d.stride, d.sign, d.offset, d.pad_mode = N.G_ADJ_STRIDE2, 2, -1, 1, N.PAD_ZERO
    d.y, d.Hd, d.Wd, d.Cd, d.n_begin, d.n_count, d.y_choff = P(y), H, W, C, 0, C, 0
    d.dact_aux, d.dact = (P(auxd), N.ACT_ELU | (N.DACT_AFTER_ADDEND if after else 0)) if use_aux else (None, 0)
    d.addend = P(addd) if use_add else None
    d.groups = 1
    N._weights_for(spec, d, True)
    N.kernel_timer_begin()
    try:
        rc = L.lib().mcav_igemm(ctypes.byref(d), L.stream())
        dispatches = L.lib().mcav_kernel_timer_count()
    finally:
        N.kernel_timer_end()
    torch.cuda.synchronize()
    assert rc == 0 and y.intact()
    assert dispatches == 2, "the launch did not take the K-split (%d timed dispatches)" % dispatches
    got = y.cpu()
    assert int(is_sentinel(got).sum()) == 0
    err = rel_err(got, want)
    print("K-split finish, %s: rel_err %.2e" % (combo, err))
    assert err < 2e-5


# ================================================================================================ C3: weight gradient
class WCase:
    """One weight-gradient geometry: conv = (B, H, W, Cin, Cout, k, stride, pad, pad_mode); stored: channels physically in x (Kp);
    up: x is stored at half the size and nearest-upsampled by the gather; smallc: the NHWC4 image stem."""

    def __init__(self, name, conv, stored=None, up=False, smallc=False, bias=True, tile=0, mma=0, planes=0, generic_ok=True):
        self.name, self.conv, self.up, self.smallc, self.bias, self.tile, self.mma, self.planes = name, conv, up, smallc, bias, tile, mma, planes
        self.stored = stored if stored is not None else conv[3]
        self.generic_ok = generic_ok          # the form also exists for a dy whose stride is no multiple of 4 (dy_choff = 2)


WCASES = [
    WCase("table", (2, 6, 10, 32, 64, 3, 1, 1, Z)),
    WCase("fast (bit 8)", (2, 6, 10, 32, 64, 3, 1, 1, Z), tile=0x100),
    WCase("table, Cin 9 of Kp 16, Cout 12", (2, 7, 11, 9, 12, 3, 1, 1, Z), stored=16),
    WCase("bit 8, Cin 9 of Kp 16, Cout 12", (2, 7, 11, 9, 12, 3, 1, 1, Z), stored=16, tile=0x100),
    WCase("Cout 1", (2, 8, 12, 16, 1, 3, 1, 1, R)),
    WCase("bit 8, Cout 1", (2, 8, 12, 16, 1, 3, 1, 1, R), tile=0x100),
    WCase("one stored channel (generic gather)", (2, 7, 11, 1, 32, 3, 1, 1, Z), stored=1, tile=0x100),
    WCase("halo", (2, 7, 19, 16, 16, 3, 1, 1, R)),
    WCase("halo, upsampled source", (2, 14, 38, 16, 16, 3, 1, 1, R), up=True),
    WCase("depth stem", (2, 45, 70, 3, 64, 7, 2, 3, Z), stored=4, smallc=True, bias=False, generic_ok=False),
    WCase("pose stem", (2, 45, 70, 9, 16, 7, 2, 3, Z), stored=16, generic_ok=False),
    WCase("bf16", (2, 12, 20, 64, 64, 3, 1, 1, Z), mma=1, planes=1, generic_ok=False),
    WCase("split where ahead", (2, 12, 20, 64, 64, 3, 1, 1, Z), mma=2, planes=6, generic_ok=False),
    WCase("split everywhere", (2, 12, 20, 64, 64, 3, 1, 1, Z), mma=3, planes=6, generic_ok=False),
    WCase("split everywhere, 1x1 stride 2", (2, 9, 15, 64, 64, 1, 2, 0, Z), mma=3, planes=6, generic_ok=False),
]


def wgrad_desc(c, x, dy, Cdy, dy_choff, dw, dbias, accumulate, mma):
    from mcav import nn as N
    B, H, W, Cin, Cout, k, stride, pad, pm = c.conv
    d = N.WgradDesc()
    d.x1, d.B, d.Hs, d.Ws, d.C1, d.up1 = P(x), B, H, W, c.stored, int(c.up)
    d.kh, d.kw, d.Kp = k, k, 4 if c.smallc else N.up16(c.stored)
    d.mode = N.G_SMALLC if c.smallc else N.G_DIRECT
    d.stride, d.sign, d.offset, d.pad_mode = stride, 1, -pad, pm
    d.dy, d.Hd, d.Wd, d.Cdy, d.dy_choff = P(dy), N.out_size(H, k, stride, pad), N.out_size(W, k, stride, pad), Cdy, dy_choff
    d.Cout, d.Cin = Cout, Cin
    d.dw_oihw, d.accumulate, d.dbias = P(dw), accumulate, P(dbias)
    d.tile, d.mma = c.tile, mma
    return d


def run_wgrad(d, outs, expect=0):
    """mcav_wgrad with a workspace of exactly mcav_wgrad_workspace_bytes in a guarded window (NaN-filled: a slab element that is read before
    it is written shows in the gradient); asserts the return code and the bands of the workspace and of every output."""
    from mcav import lib as L
    nbytes = L.lib().mcav_wgrad_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0 and nbytes % 4 == 0, nbytes
    ws = Guarded((nbytes // 4,), band=256)
    rc = L.lib().mcav_wgrad(ctypes.byref(d), P(ws), nbytes, L.stream())
    torch.cuda.synchronize()
    assert rc == expect, "mcav_wgrad returned %d" % rc
    assert ws.intact(), "mcav_wgrad wrote outside its workspace of %d bytes" % nbytes
    for o in outs:
        assert o is None or o.intact(), "mcav_wgrad wrote outside a gradient"


def wgrad_operands(c):
    """-> x NCHW as the convolution sees it, the stored NHWC device tensor, dy, and the float64 gradients for the case's mma"""
    from mcav import nn as N
    B, H, W, Cin, Cout, k, stride, pad, pm = c.conv
    g = torch.Generator().manual_seed(sum(c.conv) + 3 * len(c.name))
    if c.up:
        low = torch.randn(B, Cin, H // 2, W // 2, generator=g)
        x, stored = F.interpolate(low, scale_factor=2, mode="nearest"), low
    else:
        x = stored = torch.randn(B, Cin, H, W, generator=g)
    xs = to_nhwc(stored)
    if c.stored > Cin:
        xs = torch.cat([xs, torch.zeros(*xs.shape[:3], c.stored - Cin)], 3)
    dy = torch.randn(B, Cout, N.out_size(H, k, stride, pad), N.out_size(W, k, stride, pad), generator=g)
    rnd = r16 if c.mma == 1 else (lambda t: t.double())
    wr = torch.zeros(Cout, Cin, k, k, dtype=torch.float64).requires_grad_()
    ref_conv64(rnd(x), wr, None, stride, pad, pm).backward(rnd(dy))
    return xs.contiguous().to(DEV), dy, wr.grad, dy.double().sum((0, 2, 3))          # (the bias gradient sums the unrounded dy)


def wide_dy(dy, Cdy, choff, g):
    """dy's channels at [choff, choff + Cout) of a Cdy-channel NHWC tensor whose other channels hold noise the launch must not read"""
    t = torch.randn(dy.shape[0], dy.shape[2], dy.shape[3], Cdy, generator=g) * 100.0
    t[..., choff:choff + dy.shape[1]] = to_nhwc(dy)
    return t.contiguous().to(DEV)


@pytest.mark.parametrize("c", WCASES, ids=lambda c: c.name.replace(" ", "_").replace(",", ""))
def test_wgrad_overwrite_accumulate_and_dy_window(c):
    from mcav import lib as L
    from mcav import nn as N
    B, H, W, Cin, Cout, k, stride, pad, pm = c.conv
    x, dy, want_w, want_b = wgrad_operands(c)
    g = torch.Generator().manual_seed(97)
    start_w, start_b = torch.randn(Cout, Cin, k, k, generator=g), torch.randn(Cout, generator=g)
    variants = [("overwrite", Cout, 0, 0), ("accumulate", Cout, 0, 1), ("dy_choff 16", Cout + 32, 16, 0)]
    if c.generic_ok:
        variants.append(("dy_choff 2 (generic loader)", Cout + 2, 2, 0))
    for what, Cdy, choff, acc in variants:
        dyd = wide_dy(dy, Cdy, choff, g)
        res = {}
        for mma in ((c.mma, 0) if c.mma >= 2 else (c.mma,)):                       # split forms: the fp32 kernels on the same launch beside them
            dw = window((Cout, Cin, k, k), init=start_w if acc else None)
            db = window((Cout,), init=start_b if acc else None) if c.bias else None
            d = wgrad_desc(c, x, dyd, Cdy, choff, dw, db, acc, mma)
            if mma:
                assert L.lib().mcav_wgrad_uses_bf16(ctypes.byref(d)) == 1, "%s, %s: the launch left the bf16 MFMA kernels" % (c.name, what)
            run_wgrad(d, (dw, db))
            gw, gb = dw.cpu(), (db.cpu() if db is not None else None)
            left = int(is_sentinel(gw).sum()) + (int(is_sentinel(gb).sum()) if gb is not None else 0)
            assert left == 0, "%s, %s: %d gradient elements were never stored" % (c.name, what, left)
            ww, wb = (want_w + start_w.double(), want_b + start_b.double()) if acc else (want_w, want_b)
            res[mma] = (rel_err(gw, ww), rel_err(gb, wb) if gb is not None else 0.0, rms_err(gw, ww))
        ew, eb, rw = res[c.mma]
        print("%-36s %-28s dw %.2e dbias %.2e" % (c.name, what, ew, eb))
        if c.mma >= 2:
            assert ew < 3e-6 and eb < 3e-6, (c.name, what, res)
            assert no_worse(ew, res[0][0]) or rw <= 1.25 * res[0][2], (c.name, what, res)
        else:
            assert ew < 5e-5 and eb < 5e-5, (c.name, what, ew, eb)
    if c.planes:                                                                    # ... and through the product's launcher: which pipe it reports
        dw = window((Cout, Cin, k, k), init=0.0)
        db = window((Cout,), init=0.0)
        d = wgrad_desc(c, x, dev_nhwc(dy), Cout, 0, dw, db, 1, c.mma)
        N.launch_wgrad(d, (x,))
        torch.cuda.synchronize()
        assert N.LAST_WGRAD_PLANES == c.planes and dw.intact() and db.intact()
        assert rel_err(dw.cpu(), want_w) < (3e-6 if c.mma >= 2 else 5e-5)


@pytest.mark.parametrize("tile", [0, 0x100])
def test_wgrad_input_channel_windows_of_a_decoder_level(tile):
    """The filter of conv(cat(up2(a), skip)) in two launches (mcav_wgrad_desc.Cin_total / ci_offset): the skip half writes input channels
    [C1, C1 + C2) of [Cout][C1 + C2][3][3] and the merged-tap half (upm = 1) channels [0, C1); with accumulate = 0 each on a gradient of its
    own that starts as sentinels, so a launch that spills into its neighbour's input channels shows."""
    B, h, w_, C1, C2, Cout = 2, 5, 7, 32, 64, 64
    g = torch.Generator().manual_seed(23)
    a, skip = torch.randn(B, C1, h, w_, generator=g), torch.randn(B, C2, 2 * h, 2 * w_, generator=g)
    dy = torch.randn(B, Cout, 2 * h, 2 * w_, generator=g)
    wr = torch.zeros(Cout, C1 + C2, 3, 3, dtype=torch.float64).requires_grad_()
    xcat = torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), skip], 1).double()
    ref_conv64(xcat, wr, None, 1, 1, 1).backward(dy.double())
    ad, sd, dyd = dev_nhwc(a), dev_nhwc(skip), dev_nhwc(dy)
    halves = [("skip half", WCase("skip", (B, 2 * h, 2 * w_, C2, Cout, 3, 1, 1, R), tile=tile), sd, C1, C2, 0, True),
              ("merged-tap half", WCase("upm", (B, 2 * h, 2 * w_, C1, Cout, 3, 1, 1, R), up=True), ad, 0, C1, 1, False)]
    for what, c, x, off, cin, upm, with_bias in halves:
        if upm and tile:
            continue                                                                # (the merged form exists in the table-driven kernel only)
        dw = window((Cout, C1 + C2, 3, 3))
        db = window((Cout,)) if with_bias else None
        d = wgrad_desc(c, x, dyd, Cout, 0, dw, db, 0, 0)
        d.Cin_total, d.ci_offset, d.upm = C1 + C2, off, upm
        run_wgrad(d, (dw, db))
        gw = dw.cpu()
        inside = torch.zeros(C1 + C2, dtype=torch.bool)
        inside[off:off + cin] = True
        stray = int((~is_sentinel(gw[:, ~inside])).sum())
        assert stray == 0, "%s: %d elements outside input channels [%d, %d) were stored" % (what, stray, off, off + cin)
        assert int(is_sentinel(gw[:, inside]).sum()) == 0, "%s: elements of its window were never stored" % what
        err = rel_err(gw[:, inside], wr.grad[:, inside])
        print("%-16s tile %#x: dw %.2e" % (what, tile, err))
        assert err < 5e-5
        if with_bias:
            assert rel_err(db.cpu(), dy.double().sum((0, 2, 3))) < 5e-5


# ================================================================================================ C4: refusals
def test_igemm_refuses_what_it_cannot_honour():
    """Order is the safety rule: the planner entry (which launches nothing) must refuse first; only then is the descriptor -- some describe a
    2 GiB output -- handed to mcav_igemm, which must answer MCAV_E_INVALID with y untouched."""
    from mcav import lib as L
    from mcav import nn as N
    h = L.lib()
    x, w = torch.ones(1, 8, 8, 64, device=DEV), torch.ones(64, 9 * 64, device=DEV)
    for name, change in K.IGEMM_REFUSED.items():
        y = window((1, 8, 8, 64))
        d = K.igemm_base(N, P(x), P(w), P(y))
        assert h.mcav_igemm_mtiles(ctypes.byref(d)) > 0
        change(d)
        assert h.mcav_igemm_mtiles(ctypes.byref(d)) == E_INVALID, name
        rc = h.mcav_igemm(ctypes.byref(d), L.stream())
        torch.cuda.synchronize()
        assert rc == E_INVALID and y.untouched(), name


def test_wgrad_refuses_what_it_cannot_honour():
    from mcav import lib as L
    from mcav import nn as N
    h = L.lib()
    x, dy = torch.ones(1, 8, 8, 64, device=DEV), torch.ones(1, 8, 8, 64, device=DEV)
    for name, change in K.WGRAD_REFUSED.items():
        dw, db, ws = window((64, 64, 3, 3)), window((64,)), Guarded((1 << 20,), band=256)
        d = K.wgrad_base(N, P(x), P(dy), P(dw))
        d.dbias = P(db)
        assert h.mcav_wgrad_workspace_bytes(ctypes.byref(d)) > 0
        change(d)
        assert h.mcav_wgrad_workspace_bytes(ctypes.byref(d)) == 0, name
        rc = h.mcav_wgrad(ctypes.byref(d), P(ws), 4 << 20, L.stream())
        torch.cuda.synchronize()
        assert rc == E_INVALID and dw.untouched() and db.untouched() and ws.untouched(), name
        item = N.WgradReduceItem()
        rc = h.mcav_wgrad_deferred(ctypes.byref(d), P(ws), 4 << 20, ctypes.byref(item), L.stream())
        torch.cuda.synchronize()
        assert rc == E_INVALID and ws.untouched(), name
