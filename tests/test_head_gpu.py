"""GPU: the one-channel disparity head of csrc/narrow_conv.hip against float64, element by element, at every alignment of the image border
against the kernels' grids and where a workgroup walks from one tile to the next.

Cases: tests/head_cases.py (tests/test_head_cpu.py shows that every alignment class is hit for every channel count and that the walk cases
walk).  Definition and bound: tests/head_ref.py -- |got - want64| <= envelope at EVERY element, the envelope computed from the inputs alone;
the same file's mutants (one border term of the kernel's gather dropped, a walked tile skipped) fall outside it on the CPU.  Launches go
through the C ABI into NaN-filled windows between sentinel bands (tests/guarded.py) for y, dx, dw and dbias: an element a kernel never stores
stays a NaN, which is outside every envelope, and a launch never sees the previous launch's answer.  Where dy is zero around a pixel the
kernel's dx must be the addend's exact bits.

The fused activations of the forward (sigmoid, as the network runs the head) are held to the project's 2e-5 of the largest entry: the device
expf error is not derived (as in tests/test_halo_gpu.py).  Dense weight / bias gradients are held to the project's 5e-5 max-norm; on the band
and tile supports every element is inside the envelope.

Also here: the same head through mcav.nn on both sides of its 65536-pixel switch, and the other implementation of the same convolution
(conv_fwd / act_bwd_padded + conv_wgrad / conv_dgrad with a one-output ConvSpec: the halo and the general fp32 kernels) held to the same
envelopes.  Run with -s for the worst ratio to the envelope per form."""
import functools

import pytest
import torch

import head_cases as K
import head_ref as R
from conftest import rel_err
from conv_plan_cases import recorded_routes
from guarded import Guarded, P, band_for, guard_allocations, guarded_spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}                                  # form -> the largest |got - want64| / envelope seen in this process
IDS = [K.case_id(c) for c in K.CASES]
FILL_DW, FILL_DB = 0.75, -1.5               # what dw / dbias hold before an accumulating launch
ONCE_PER_C = [ci for ci, c in enumerate(K.CASES) if (c.H, c.W) == (17, K.pxb(c.C) + 1)]       # the forms that run once per channel count


@pytest.fixture(autouse=True)
def guards():
    with guard_allocations() as g:
        yield g
        g.check()


@pytest.fixture(scope="module")
def N():
    from mcav import nn
    return nn


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous()


def window(guards, shape, init=None):
    return guards.add(Guarded(shape, init=init, band=band_for(shape)))


# ------------------------------------------------------------------------------------------------ the judge
def judge(what, c, got, want, env):
    """every element of got ([B, channels, H, W] on the CPU) inside the envelope of want; the failure names the worst element and where it lies"""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    r = R.ratio(got, want, env)
    worst = float(r.max())
    WORST[what] = max(WORST.get(what, 0.0), worst)
    bad = R.outside(got, want, env)
    if bool(bad.any()):
        n, ch, y, x = (int(v) for v in torch.unravel_index(torch.argmax(r), r.shape))
        classes = {}
        for yy, xx in {(int(p[2]), int(p[3])) for p in bad.nonzero()[:4096]}:
            classes[K.pixel_class(c, yy, xx)] = classes.get(K.pixel_class(c, yy, xx), 0) + 1
        raise AssertionError("%s %s: %d of %d elements outside the envelope (pixels by class: %s); worst (n=%d, y=%d, x=%d, channel=%d) [%s] in tile %d: "
                             "got %r, float64 %r, %.3g envelopes" % (
                                 what, K.case_id(c), int(bad.sum()), bad.numel(), classes, n, y, x, ch, K.pixel_class(c, y, x),
                                 (n * K.tiles_y(c) + y // K.TH) * K.tiles_x(c) + x // K.pxb(c.C), float(got[n, ch, y, x]), float(want[n, ch, y, x]), worst))
    return worst


def judge_filter(what, c, got, want, env, support=""):
    """the same for the weight gradient [1, C, 3, 3] or the bias gradient [1]"""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    r = R.ratio(got, want, env)
    worst = float(r.max())
    WORST[what] = max(WORST.get(what, 0.0), worst)
    bad = R.outside(got, want, env)
    if bool(bad.any()):
        at = tuple(int(v) for v in torch.unravel_index(torch.argmax(r), r.shape))
        raise AssertionError("%s %s, dy on %s: %d of %d elements outside the envelope; worst %s at %s: got %r, float64 %r, %.3g envelopes" % (
            what, K.case_id(c), support, int(bad.sum()), bad.numel(), "(co, ci, ky, kx)" if got.dim() == 4 else "(co)", at, float(got[at]), float(want[at]), worst))
    return worst


def exact_where_nothing_arrives(what, c, got, S, addend):
    """dy is zero on every output that reaches the pixel: the kernel's 0 * act' + addend is the addend's own bits (an exact zero without one)"""
    m = (S == 0).expand_as(got)
    want = addend if addend is not None else torch.zeros_like(got)
    same = got[m] == want[m]
    assert bool(same.all()), "%s %s: %d of %d elements that no gradient reaches are not the exact %s" % (
        what, K.case_id(c), int((~same).sum()), int(m.sum()), "addend" if addend is not None else "zero")


# ------------------------------------------------------------------------------------------------ the launches
class Device:
    """one case's inputs on the GPU, in the kernels' layouts (activations NHWC, the filter OIHW)"""

    def __init__(self, c):
        i = K.inputs(c)
        self.x, self.addend = nhwc(i["x"]), nhwc(i["addend"])
        self.w, self.b = i["w"].contiguous().to(DEV), i["b"].to(DEV)
        self.y = nhwc(i["y"])


def launch_fwd(guards, c, d, act, bias=True):
    from mcav import lib as L
    y = window(guards, (c.B, c.H, c.W, 1))
    rc = L.lib().mcav_conv3x3r_c1_fwd(P(d.x), c.B, c.H, c.W, c.C, P(d.w), P(d.b) if bias else None, act, P(y), L.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert y.intact(), "mcav_conv3x3r_c1_fwd wrote outside y"
    return nchw(y.t)


def launch_bwd(guards, c, d, dy, fused, x_act=R.ACT_ELU, addend=True, accumulate=0, dbias=True, act=R.ACT_SIGMOID):
    """dy NCHW on the CPU -> (dx NCHW, dw [1, C, 3, 3], db [1] or None) on the CPU"""
    from mcav import lib as L
    h = L.lib()
    dx = window(guards, (c.B, c.H, c.W, c.C))
    dw = window(guards, (1, c.C, 3, 3), init=FILL_DW if accumulate else None)
    db = window(guards, (1,), init=FILL_DB if accumulate else None) if dbias else None
    ws = L.workspace(h.mcav_conv3x3r_c1_bwd_workspace_bytes(c.C), torch.device(DEV, torch.cuda.current_device()), "narrow")
    rc = h.mcav_conv3x3r_c1_bwd(P(d.x), c.B, c.H, c.W, c.C, P(d.w), P(nhwc(dy)), P(d.y) if fused else None, act if fused else R.ACT_NONE, x_act,
                                P(d.addend) if addend else None, P(dx), P(dw), P(db), accumulate, P(ws), ws.numel(), L.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert dx.intact() and dw.intact() and (db is None or db.intact()), "mcav_conv3x3r_c1_bwd wrote outside an output"
    return nchw(dx.t), dw.cpu(), (db.cpu() if db is not None else None)


@functools.lru_cache(maxsize=4)
def reference(c, support, fused, x_act=R.ACT_ELU, act=R.ACT_SIGMOID, images=None):
    """the float64 gradients without the addend (it enters dx as + addend and its envelope as + u |addend|); images = (n0, n1): of those
    images only (the others hold no dy: they contribute exact zeros)"""
    i = K.inputs(c)
    sl = slice(None) if images is None else slice(*images)
    dy = (i["dy"] * K.support_mask(c, support))[sl]
    return R.backward(i["x"][sl], i["w"], dy, i["y"][sl] if fused else None, act if fused else R.ACT_NONE, x_act)


def check_bwd(name, c, got, ref, support, addend, accumulate, images=None):
    """dx, dw, db of one launch against the reference of (case, support, form)"""
    dx, dw, db = got
    sl = slice(None) if images is None else slice(*images)
    add = K.inputs(c)["addend"] if addend else None
    want, env = ref["dx"], ref["edx"]
    if addend:
        want, env = want + add[sl].double(), env + R.U * add[sl].double().abs()
    worst = [judge("dx " + name, c._replace(B=want.shape[0]), dx[sl], want, env)]
    exact_where_nothing_arrives("dx " + name, c, dx[sl], ref["S"], add[sl] if addend else None)
    if images is not None:                                  # no dy in the other images: the addend's bits, whichever workgroup walked them
        rest = torch.ones(c.B, dtype=torch.bool)
        rest[sl] = False
        assert torch.equal(dx[rest], add[rest] if addend else torch.zeros_like(dx[rest])), "dx %s %s: images without dy are not the exact addend" % (name, K.case_id(c))
    for what, g, w, e, fill in (("dw", dw, ref["dw"], ref["edw"], FILL_DW), ("db", db, ref["db"], ref["edb"], FILL_DB)):
        if g is None:
            continue
        if accumulate:
            w, e = R.accumulated(w, e, fill)
        if support == "dense":                              # the project's max-norm criterion
            err = rel_err(g, w)
            print("    %s %s dense: %.3g of the largest entry" % (what, name, err))
            assert err < 5e-5, (what, name, K.case_id(c), err)
        else:
            worst.append(judge_filter("%s %s" % (what, name), c, g, w, e, K.support_id(support)))
    return max(worst)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("ci", range(len(K.CASES)), ids=IDS)
def test_forward_inside_the_envelope(guards, ci):
    c, i, d = K.CASES[ci], K.inputs(K.CASES[ci]), Device(K.CASES[ci])
    pre, env = R.forward(i["x"], i["w"], i["b"])
    print("%s %d tiles: with bias %.3f of the envelope" % (K.case_id(c), K.tiles(c), judge("fwd act none", c, launch_fwd(guards, c, d, R.ACT_NONE), pre, env)))
    pre0, env0 = R.forward(i["x"], i["w"], None)
    print("    bias = NULL %.3f" % judge("fwd act none, bias NULL", c, launch_fwd(guards, c, d, R.ACT_NONE, bias=False), pre0, env0))
    err = rel_err(launch_fwd(guards, c, d, R.ACT_SIGMOID), torch.sigmoid(pre))
    print("    sigmoid: %.3g of the largest entry" % err)
    assert err < 2e-5, err
    if ci in ONCE_PER_C:        # |relu(a) - relu(b)| <= |a - b|: the envelope of the pre-activation holds
        print("    relu %.3f" % judge("fwd act relu", c, launch_fwd(guards, c, d, R.ACT_RELU), torch.relu(pre), env))


# ------------------------------------------------------------------------------------------------ backward
FORMS = tuple((fused, addend, accumulate) for fused in (True, False) for addend in (True, False) for accumulate in (0, 1))


def form_name(fused, addend, accumulate, x_act=R.ACT_ELU):
    return "%s, x_act %s%s%s" % ("fused" if fused else "pre-multiplied", {R.ACT_NONE: "none", R.ACT_RELU: "relu", R.ACT_ELU: "elu"}[x_act],
                                 ", addend" if addend else "", ", accumulate" if accumulate else "")


@pytest.mark.parametrize("ci", range(len(K.CASES)), ids=IDS)
def test_backward_inside_the_envelope(guards, ci):
    c, i, d = K.CASES[ci], K.inputs(K.CASES[ci]), Device(K.CASES[ci])
    for support in K.supports(c):
        dy = i["dy"] * K.support_mask(c, support)
        for fused, addend, accumulate in FORMS:
            name = form_name(fused, addend, accumulate)
            got = launch_bwd(guards, c, d, dy, fused, addend=addend, accumulate=accumulate)
            worst = check_bwd(name, c, got, reference(c, support, fused), support, addend, accumulate)
            print("%s %-52s dy on %-6s: worst %.3f of the envelope" % (K.case_id(c), name, K.support_id(support), worst))
        if ci in ONCE_PER_C:
            for x_act in (R.ACT_NONE, R.ACT_RELU):
                name = form_name(True, True, 0, x_act)
                got = launch_bwd(guards, c, d, dy, True, x_act=x_act)
                print("%s %-52s dy on %-6s: worst %.3f" % (K.case_id(c), name, K.support_id(support),
                                                         check_bwd(name, c, got, reference(c, support, True, x_act), support, True, 0)))
            for accumulate in (0, 1):
                name = form_name(False, True, accumulate) + ", dbias NULL"
                got = launch_bwd(guards, c, d, dy, False, accumulate=accumulate, dbias=False)
                print("%s %-52s dy on %-6s: worst %.3f" % (K.case_id(c), name, K.support_id(support),
                                                         check_bwd(name, c, got, reference(c, support, False), support, True, accumulate)))
            name = "fused relu, x_act elu, addend"            # act = RELU through the output y: the derivative is exact
            got = launch_bwd(guards, c, d, dy, True, act=R.ACT_RELU)
            print("%s %-52s dy on %-6s: worst %.3f" % (K.case_id(c), name, K.support_id(support),
                                                     check_bwd(name, c, got, reference(c, support, True, R.ACT_ELU, R.ACT_RELU), support, True, 0)))


# ------------------------------------------------------------------------------------------------ where a workgroup walks
def test_forward_where_a_workgroup_walks_two_tiles(guards):
    """16386 tiles on 16384 workgroups: workgroups 0 and 1 refill the row ring and the halo columns for a second tile (of 16 rows and of 1)"""
    c = K.FWD_WALK_CASE
    i, d = K.inputs(c), Device(c)
    per = K.tiles_per_workgroup(c, K.FWD_BLOCKS)
    print("%s: %d tiles on %d workgroups, %d of them walk 2" % (K.case_id(c), K.tiles(c), len(per), per.count(2)))
    pre, env = R.forward(i["x"], i["w"], i["b"])
    print("    act none: worst %.3f of the envelope" % judge("fwd walk", c, launch_fwd(guards, c, d, R.ACT_NONE), pre, env))
    err = rel_err(launch_fwd(guards, c, d, R.ACT_SIGMOID), torch.sigmoid(pre))
    assert err < 2e-5, err


@pytest.mark.parametrize("c", K.WALK_CASES, ids=[K.case_id(c) for c in K.WALK_CASES])
def test_backward_where_a_workgroup_walks_tiles(guards, c):
    """more than 2048 tiles: dpre, the prefetch registers and the carried dw / db accumulators go from a workgroup's tile to its next one of
    another row count.  dy on one tile: dw, db and that image's dx elementwise, every other image the addend's exact bits."""
    i, d = K.inputs(c), Device(c)
    per = K.tiles_per_workgroup(c, K.BWD_BLOCKS)
    print("%s: %d tiles on %d workgroups, %d..%d tiles each" % (K.case_id(c), K.tiles(c), len(per), min(per), max(per)))
    for k, fused, accumulate in zip(K.walk_tiles(c), (True, False, True), (0, 1, 1)):
        support, n = ("tile", k), K.tile_origin(c, k)[0]
        name = "walk, " + form_name(fused, True, accumulate)
        got = launch_bwd(guards, c, d, i["dy"] * K.support_mask(c, support), fused, accumulate=accumulate)
        worst = check_bwd(name, c, got, reference(c, support, fused, images=(n, n + 1)), support, True, accumulate, images=(n, n + 1))
        print("    dy on tile %5d (%2d rows, walked as number %d by workgroup %d): worst %.3f of the envelope" % (
            k, K.tile_rows(c, k), k // K.BWD_BLOCKS + 1, k % K.BWD_BLOCKS, worst))
    name = "walk, " + form_name(True, True, 0)
    got = launch_bwd(guards, c, d, i["dy"], True)
    print("    dense: dx worst %.3f of the envelope" % check_bwd(name, c, got, reference(c, "dense", True), "dense", True, 0))


# ------------------------------------------------------------------------------------------------ through mcav.nn
NN_CASES = [K.CASES[ci] for ci in ONCE_PER_C] + [K.Case(1, 255, 257, 16), K.Case(1, 256, 256, 16)]      # ... and both sides of the 65536-pixel switch


@pytest.mark.parametrize("c", NN_CASES, ids=[K.case_id(c) for c in NN_CASES])
def test_through_the_host_wrappers(N, c):
    """conv3x3r_c1_fwd / conv3x3r_c1_bwd as the decoder calls them (their outputs are mcav.nn.empty windows here); from 65536 pixels on the
    wrapper forms dy * act'(y) in a pass of its own (the same three roundings) and launches the pre-multiplied form"""
    i, d = K.inputs(c), Device(c)
    param = lambda t: torch.nn.Parameter(t.detach().clone().to(DEV))      # noqa: E731
    spec = guarded_spec(N.ConvSpec(param(i["w"]), param(i["b"]), 1, 1, N.PAD_REFLECT))
    assert N.narrow_ok(spec, d.x) and (c.B * c.H * c.W >= 1 << 16) == (c.H == 256)
    pre, env = R.forward(i["x"], i["w"], i["b"])
    judge("nn fwd act none", c, nchw(N.conv3x3r_c1_fwd(spec, d.x, N.ACT_NONE)), pre, env)
    y = N.conv3x3r_c1_fwd(spec, d.x, N.ACT_SIGMOID)
    assert rel_err(nchw(y), torch.sigmoid(pre)) < 2e-5
    dyd = nhwc(i["dy"])
    ref = R.backward(i["x"], i["w"], i["dy"], nchw(y), R.ACT_SIGMOID, R.ACT_ELU)        # from the disparity the kernel stored, as the network does
    add = i["addend"].double()
    dx = N.conv3x3r_c1_bwd(spec, d.x, dyd, y, N.ACT_SIGMOID, N.ACT_ELU, addend=d.addend)
    worst = judge("nn dx, addend", c, nchw(dx), ref["dx"] + add, ref["edx"] + R.U * add.abs())
    ew, eb = rel_err(spec.weight.grad, ref["dw"]), rel_err(spec.bias.grad, ref["db"])
    assert ew < 5e-5 and eb < 5e-5, (ew, eb)
    dx = N.conv3x3r_c1_bwd(spec, d.x, dyd, y, N.ACT_SIGMOID, N.ACT_ELU)                  # accumulates into .grad; no addend
    worst = max(worst, judge("nn dx", c, nchw(dx), ref["dx"], ref["edx"]))
    ew2, eb2 = rel_err(spec.weight.grad, 2 * ref["dw"]), rel_err(spec.bias.grad, 2 * ref["db"])
    print("%s through mcav.nn: dx worst %.3f of the envelope; dw %.3g, db %.3g, accumulated twice %.3g, %.3g of the largest entry" % (K.case_id(c), worst, ew, eb, ew2, eb2))
    assert ew2 < 5e-5 and eb2 < 5e-5, (ew2, eb2)


# ------------------------------------------------------------------------------------------------ the other implementation of the same head
OTHER = [ci for ci, c in enumerate(K.CASES) if c.C in (16, 32)]
DIFF = {}


@pytest.mark.parametrize("ci", OTHER, ids=[IDS[ci] for ci in OTHER])
def test_the_convolution_kernels_on_the_same_head(N, guards, ci):
    """what the decoder runs where narrow_ok is false: conv_fwd, act_bwd_padded + conv_wgrad, conv_dgrad (* ELU'(x) + addend) with a one-output
    ConvSpec.  With tile = 0 the planner takes the forward and the weight gradient of these 16- and 32-channel shapes to the halo kernels and
    the data gradient (dy padded to 4 channels) to the general fp32 kernels; TILE_GENERAL takes all three to the general fp32 family.  Both are
    held to the stencil's envelopes (the fused one: act_bwd_padded forms dy * y * (1 - y) with the same three roundings)."""
    c, i, d = K.CASES[ci], K.inputs(K.CASES[ci]), Device(K.CASES[ci])
    param = lambda t: torch.nn.Parameter(t.detach().clone().to(DEV))      # noqa: E731
    pre, env = R.forward(i["x"], i["w"], i["b"])
    stencil = {"y": launch_fwd(guards, c, d, R.ACT_NONE)}
    for support in ("dense", "band"):
        dy = i["dy"] * K.support_mask(c, support)
        ref = reference(c, support, True)
        stencil[support] = launch_bwd(guards, c, d, dy, True, accumulate=1)
        for tile, label in ((0, "planner's choice"), (N.TILE_GENERAL, "general fp32")):
            spec = guarded_spec(N.ConvSpec(param(i["w"]), param(i["b"]), 1, 1, N.PAD_REFLECT), fill=FILL_DW)
            spec.bias.grad.fill_(FILL_DB)
            with recorded_routes(N) as log:
                y = nchw(N.conv_fwd(spec, d.x, act=N.ACT_NONE, tile=tile))
                dpre = N.act_bwd_padded(nhwc(dy), d.y, N.ACT_SIGMOID, 4)
                N.conv_wgrad(spec, d.x, dpre, tile=tile)
                dx = nchw(N.conv_dgrad(spec, dpre, (c.H, c.W), dact_aux=d.x, dact=N.ACT_ELU, addend=d.addend, tile=tile))
            torch.cuda.synchronize()
            routes = {kind: r.family for kind, r in log}
            assert [kind for kind, _ in log] == ["fwd", "wgrad", "dgrad"]
            assert routes == ({"fwd": N.IGEMM_FP32, "wgrad": N.WGRAD_FP32, "dgrad": N.IGEMM_FP32} if tile else
                              {"fwd": N.IGEMM_HALO, "wgrad": N.WGRAD_HALO, "dgrad": N.IGEMM_FP32}), (label, routes)
            name = "other (%s)" % label
            worst = judge("fwd " + name, c, y, pre, env)
            got = (dx, spec.weight.grad.detach().cpu(), spec.bias.grad.detach().cpu())
            worst = max(worst, check_bwd(name, c, got, ref, support, True, 1))
            diffs = [float((a - b).abs().max()) for a, b in zip((y,) + got, (stencil["y"],) + stencil[support])]
            for key, v in zip(("y", "dx", "dw", "db"), diffs):
                DIFF[(label, key)] = max(DIFF.get((label, key), 0.0), v)
            print("%s %-18s dy on %-5s: worst %.3f of the envelope; largest difference to the stencil: y %.3g, dx %.3g, dw %.3g, db %.3g" % (
                (K.case_id(c), label, support, worst) + tuple(diffs)))


def test_worst_ratios_table():
    """(prints what the tests above measured in this process: the largest |got - float64| / envelope per form)"""
    print("\nworst ratio to the envelope per form:")
    for name in sorted(WORST):
        print("  %-64s %.3f" % (name, WORST[name]))
    for key in sorted(DIFF):
        print("  largest |%s - stencil| of %s: %.3g" % (key[1], key[0], DIFF[key]))
    assert all(v <= 1.0 for v in WORST.values())
