"""GPU: every kernel of csrc/conv_halo.hip against float64, element by element, at every border alignment.

Cases and forms: tests/halo_cases.py (tests/test_halo_cpu.py shows that the planner takes each of them to the halo kernels and that every
alignment class, instantiation and grid residue is hit).  Definition and bound: tests/halo_ref.py -- |got - want64| <= envelope at EVERY
element, the envelope computed from the inputs alone.  Launches go through mcav.nn.conv_fwd / conv_dgrad / conv_wgrad into NaN-filled windows
between sentinel bands (tests/guarded.py): a tile a wrong workgroup remap never writes stays NaN, which is outside every envelope.  The route the
planner recorded for every launch is asserted, so no case silently runs on another kernel.

Also here: the same forward / adjoint cases on the general fp32 table kernel (tile bit 9), whose reflect-adjoint border path is the only
other fp32 implementation of these borders, held to the same envelope; the fused activations on a subset (the project's 2e-5 of the largest
entry: the device expm1f / expf error is not derived); dense weight gradients in the project's 5e-5 max-norm with the accumulate checked;
weight-gradient launches in which a workgroup walks two tiles.  Run with -s for the grids and the worst ratio to the envelope per form."""
import pytest
import torch
import torch.nn.functional as F

import halo_cases as K
import halo_ref as R
from conftest import rel_err
from conv_plan_cases import recorded_routes
from guarded import P, guard_allocations, guarded_spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}                                  # form -> the largest |got - want64| / envelope seen in this process
IDS = [K.case_id(c) for c in K.CASES]


@pytest.fixture(autouse=True)
def guarded_outputs():
    with guard_allocations() as guards:
        yield
        guards.check()


@pytest.fixture(scope="module")
def N():
    from mcav import nn
    return nn


def nhwc(t, cp=None):
    t = t.permute(0, 2, 3, 1)
    if cp is not None and cp != t.shape[3]:
        t = torch.cat([t, torch.zeros(*t.shape[:3], cp - t.shape[3])], 3)
    return t.contiguous().to(DEV)


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous()


def param(t):
    return None if t is None else torch.nn.Parameter(t.detach().clone().to(DEV))


def judge(what, c, got, want, env, pooled=False):
    """every element of got (NCHW on the CPU) inside the envelope of want; the failure names the worst element and where it lies"""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    r = R.ratio(got, want, env)
    worst = float(r.max())
    WORST[what] = max(WORST.get(what, 0.0), worst)
    bad = R.outside(got, want, env)
    if bool(bad.any()):
        n, ch, y, x = (int(v) for v in torch.unravel_index(torch.argmax(r), r.shape))
        cls = "/".join(sorted({K.pixel_class(c, yy, xx) for yy in ((2 * y, 2 * y + 1) if pooled else (y,)) for xx in ((2 * x, 2 * x + 1) if pooled else (x,))}))
        raise AssertionError("%s %s: %d of %d elements outside the envelope; worst (n=%d, y=%d, x=%d, channel=%d)%s [%s]: got %r, float64 %r, %.3g envelopes" % (
            what, K.case_id(c), int(bad.sum()), bad.numel(), n, y, x, ch, " of the pooled map" if pooled else "", cls,
            float(got[n, ch, y, x]), float(want[n, ch, y, x]), worst))
    return worst


def judge_filter(what, c, got, want, env, support=""):
    """the same for a weight gradient [Cout, C, 3, 3] or a bias gradient [Cout]"""
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


def routes_are(N, log, kind, n, family, variant=None, workgroups=None):
    assert len(log) == n and all(k == kind for k, _ in log), [(k, r.family) for k, r in log]
    for _, r in log:
        assert r.family == family, (kind, r.family, family)
        if variant is not None:
            assert (r.variant, r.workgroups) == (variant, workgroups), (kind, r.variant, r.workgroups, variant, workgroups)


def grid_note(form, c):
    return "grid %d x %d launch%s (%d x %d tiles x %d images, grid %% 8 = %d)" % (
        K.tiles(c), K.launches(form, c), "" if K.launches(form, c) == 1 else "es", K.tiles_y(c), K.tiles_x(c), c.B, K.tiles(c) % 8)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("ci", range(len(K.CASES)), ids=IDS)
def test_forward_inside_the_envelope(N, ci):
    c, i = K.CASES[ci], K.inputs(K.CASES[ci])
    got_by_form = {}
    for form in (f for f in K.FORMS if f.kind == "fwd" and K.applies(f, c)):
        x = i["xl"] if form.up else i["x"]
        want, env = R.forward(x, i["w"], i["b"], form.reflect, form.up)
        spec = N.ConvSpec(param(i["w"]), param(i["b"]), 1, 1, N.PAD_REFLECT if form.reflect else N.PAD_ZERO)
        xd = nhwc(x)
        for general in (False, True):
            with recorded_routes(N) as log:
                got = nchw(N.conv_fwd(spec, xd, up1=form.up, act=N.ACT_NONE, tile=form.tile | (K.T_GENERAL if general else 0)))
            if general:
                routes_are(N, log, "fwd", 1, N.IGEMM_FP32)
            else:
                family, variant, wgs = K.expected_igemm_route(N, form, c)
                routes_are(N, log, "fwd", 1, family, variant, wgs)
                got_by_form[form.name] = got
            name = form.name + (" [general fp32 kernel]" if general else "")
            print("%s %-34s %s %s: worst %.3f of the envelope" % (K.case_id(c), name, K.instantiation(form, c), grid_note(form, c), judge(name, c, got, want, env)))
    if "fwd up merged" in got_by_form:
        print("%s merged-tap against 9-tap on the same inputs: largest difference %.3g" % (
            K.case_id(c), float((got_by_form["fwd up merged"] - got_by_form["fwd up 9-tap"]).abs().max())))


# ------------------------------------------------------------------------------------------------ reflect-adjoint
@pytest.mark.parametrize("ci", range(len(K.CASES)), ids=IDS)
def test_adjoint_inside_the_envelope(N, ci):
    c, i = K.CASES[ci], K.inputs(K.CASES[ci])
    spec = N.ConvSpec(param(i["w"]), None, 1, 1, N.PAD_REFLECT)
    dyd = nhwc(i["dy"], K.up16(c.Cout))
    for form in (f for f in K.FORMS if f.kind == "adj" and K.applies(f, c)):
        pool = form.name.startswith("adj pool")
        want, env = R.adjoint(i["dy"], i["w"], **(dict(pool=True, aux=i["aux"], addend=i["add"]) if pool else {}))
        kw = dict(dact_aux=nhwc(i["aux"]), dact=N.ACT_ELU, addend=nhwc(i["add"]), pool=True) if pool else {}
        for general in (False, True):
            for n_begin in ((0, 16) if form.name == "adj n_begin 0|16" else (0,)):
                n_count = K.launch_shape(form, c)[1]
                with recorded_routes(N) as log:
                    got = nchw(N.conv_dgrad(spec, dyd, (c.H, c.W), n_begin=n_begin, n_count=n_count, tile=form.tile | (K.T_GENERAL if general else 0), **kw))
                if general:
                    routes_are(N, log, "dgrad", 1, N.IGEMM_FP32)
                else:
                    family, variant, wgs = K.expected_igemm_route(N, form, c)
                    routes_are(N, log, "dgrad", 1, family, variant, wgs)
                name = form.name + (" [general fp32 kernel]" if general else "")
                sl = slice(n_begin, n_begin + n_count)
                worst = judge(name, c, got, want[:, sl], env[:, sl], pooled=pool)
                print("%s %-34s n_begin %2d %s %s: worst %.3f of the envelope" % (K.case_id(c), name, n_begin, K.instantiation(form, c), grid_note(form, c), worst))


# ------------------------------------------------------------------------------------------------ fused activations
ACT_CASES = [ci for ci, c in enumerate(K.CASES) if (c.H, c.W) in ((2, 2), (10, 34), (3, 3), (9, 33), (17, 50), (9, 35), (16, 49))]


@pytest.mark.parametrize("ci", ACT_CASES, ids=[IDS[ci] for ci in ACT_CASES])
def test_forward_with_fused_activation(N, ci):
    """ELU as in the decoder, sigmoid as in a disparity head: the project's criterion, 2e-5 of the largest entry"""
    c, i = K.CASES[ci], K.inputs(K.CASES[ci])
    for form in (f for f in K.FORMS if f.kind == "fwd" and K.applies(f, c)):
        x = i["xl"] if form.up else i["x"]
        pre, _ = R.forward(x, i["w"], i["b"], form.reflect, form.up)
        spec = N.ConvSpec(param(i["w"]), param(i["b"]), 1, 1, N.PAD_REFLECT if form.reflect else N.PAD_ZERO)
        for act, fn in ((N.ACT_ELU, F.elu), (N.ACT_SIGMOID, torch.sigmoid)):
            with recorded_routes(N) as log:
                got = nchw(N.conv_fwd(spec, nhwc(x), up1=form.up, act=act, tile=form.tile))
            routes_are(N, log, "fwd", 1, *K.expected_igemm_route(N, form, c))
            err = rel_err(got, fn(pre))
            print("%s %-16s act %d: %.3g of the largest entry" % (K.case_id(c), form.name, act, err))
            assert err < 2e-5, (form.name, act, err)


# ------------------------------------------------------------------------------------------------ weight gradient
def run_wgrad(N, form, c, spec, xd, dy):
    """one weight-gradient launch of (form, case) accumulating into spec's gradients; dy NCHW on the CPU -> the recorded routes"""
    with recorded_routes(N) as log:
        if form.name == "wgrad dy_choff":      # mcav.nn has no caller for a channel window of a wider dy: conv_wgrad's descriptor with the window set
            wide = K.inputs(c)["wide"].clone()
            wide[:, K.CHOFF:K.CHOFF + c.Cout] = dy
            wd = nhwc(wide)
            d = K.wgrad_desc(N, form, c, x=P(xd), dy=P(wd), dw=P(N.grad_buffer(spec.weight)), db=P(N.grad_buffer(spec.bias)))
            N.launch_wgrad(d, (xd, wd))
        else:
            N.conv_wgrad(spec, xd, nhwc(dy), up1=form.up, tile=form.tile)
    routes_are(N, log, "wgrad", 1, *K.expected_wgrad_route(N, form, c)[:3])
    assert log[0][1].splits == K.expected_wgrad_route(N, form, c)[3]
    torch.cuda.synchronize()


def wgrad_spec(N, form, c):
    i = K.inputs(c)
    return guarded_spec(N.ConvSpec(param(i["w"]), None if form.name == "wgrad no bias" else param(i["b"]), 1, 1, N.PAD_REFLECT if form.reflect else N.PAD_ZERO))


def dense_wgrad(N, form, c, x, xd):
    """dense dy: the project's 5e-5 max-norm, and a second call accumulates to twice the gradient"""
    dy = K.inputs(c)["dy"]
    dw, _, db, _ = R.wgrad(x, dy, form.reflect, form.up)
    spec = wgrad_spec(N, form, c)
    for times in (1, 2):
        run_wgrad(N, form, c, spec, xd, dy)
        ew = rel_err(spec.weight.grad, times * dw)
        eb = rel_err(spec.bias.grad, times * db) if spec.bias is not None else 0.0
        print("%s %-16s dense x %d: dw %.3g, db %.3g of the largest entry" % (K.case_id(c), form.name, times, ew, eb))
        assert ew < 5e-5 and eb < 5e-5, (form.name, times, ew, eb)


def sparse_wgrad(N, form, c, x, xd, support, images=None):
    """dy on a support of at most 512 pixels: every element of dw and db inside the envelope.  images: the reference needs only these images
    (the others contribute exact zeros)"""
    dy = K.inputs(c)["dy"] * K.support_mask(c, support)
    assert R.support_pixels(dy) <= 512
    sl = slice(None) if images is None else images
    dw, ew, db, eb = R.wgrad(x[sl], dy[sl], form.reflect, form.up)
    spec = wgrad_spec(N, form, c)
    run_wgrad(N, form, c, spec, xd, dy)
    worst = judge_filter(form.name, c, spec.weight.grad.detach().cpu(), dw, ew, support)
    if spec.bias is not None:
        worst = max(worst, judge_filter(form.name + " (bias)", c, spec.bias.grad.detach().cpu(), db, eb, support))
    return worst


@pytest.mark.parametrize("ci", range(len(K.CASES)), ids=IDS)
def test_weight_gradient_inside_the_envelope(N, ci):
    c, i = K.CASES[ci], K.inputs(K.CASES[ci])
    for form in (f for f in K.FORMS if f.kind == "wgrad" and K.applies(f, c)):
        x = i["xl"] if form.up else i["x"]
        xd = nhwc(x)
        for support in K.supports(c)[:-1]:
            worst = sparse_wgrad(N, form, c, x, xd, support)
            print("%s %-16s %s dy on %-12s %d workgroups: worst %.3f of the envelope" % (
                K.case_id(c), form.name, K.instantiation(form, c), support, min(K.tiles(c), K.MAX_SPLITS), worst))
        dense_wgrad(N, form, c, x, xd)


WALKS = [(c, name) for c, names in K.WALK_CASES for name in names]


@pytest.mark.parametrize("c,name", WALKS, ids=["%s_%s" % (K.case_id(c), name.replace(" ", "_")) for c, name in WALKS])
def test_weight_gradient_where_a_workgroup_walks_two_tiles(N, c, name):
    """528 tiles on 512 workgroups: the tap accumulators and the dy column sums are carried from a workgroup's first tile to its second"""
    form, i = K.FORM[name], K.inputs(c)
    per = K.tiles_per_workgroup(c)
    print("%s %s %s: %d tiles on %d workgroups, %d of them walk 2 tiles, %d walk 1" % (
        K.case_id(c), name, K.instantiation(form, c), K.tiles(c), len(per), per.count(2), per.count(1)))
    x = i["xl"] if form.up else i["x"]
    xd = nhwc(x)
    for k in K.WALK_TILES:
        n = K.tile_origin(c, k)[0]
        worst = sparse_wgrad(N, form, c, x, xd, ("tile", k), images=slice(n, n + 1))
        print("  dy on tile %3d (walked %s by workgroup %d): worst %.3f of the envelope" % (k, "second" if k >= K.MAX_SPLITS else "first", k % K.MAX_SPLITS, worst))
    dense_wgrad(N, form, c, x, xd)


def test_worst_ratios_table():
    """(prints what the tests above measured in this process: the largest |got - float64| / envelope per form)"""
    print("\nworst ratio to the envelope per form:")
    for name in sorted(WORST):
        print("  %-44s %.3f" % (name, WORST[name]))
    assert all(v <= 1.0 for v in WORST.values())
