"""The cases of tests/test_conv_host_cpu.py and tests/golden/make_conv_host_golden.py: what mcav.nn, mcav.tape and the networks ask of the
library, taken with tests/conv_host_log.py (no GPU).  The cases call the public functions only, with the arguments the networks give them.

  layer cases    one per (layer of conv_plan_cases.LAYERS, image size, spec.mma, tile switch), full mode: conv_fwd, conv_dgrad and conv_wgrad in
                 every form the networks use on such a layer, once with mcav.nn.PROFILE off and once with it a list.
  deconv cases   mcav.tape.deconv forward + backward on two DispNetS shapes.
  network cases  DispResNet (18 and 50), PoseNet, DispNetS at 1x32x64 under three compute dtypes, sequence mode.

A case's canonical log is text; tests/golden/conv_host_parent.json holds its sha256 as the commit before the host layer was reworked wrote it."""
import torch

import conv_host_log as H
import conv_plan_cases as K

SIZES = ((2, 48, 64), (3, 9, 33), (1, 7, 21))
BIG = (12, 192, 640)
BIG_LAYERS = ("r18.conv1", "pose.conv1", "dec.1.0", "dec.1.1", "dec.0.0", "dec.0.1")      # where the halo and size predicates bite
MMAS = (0, 1, 2, 3)
TILES = (0, 1 << 9, 1 << 10, 1 << 11, 1 << 12)
DTYPES = (None, "bf16", "fp32-mfma")
NET_SIZE = (1, 32, 64)

# Profile records whose `executed` the commit before the rework guessed against its own planner: (case, index of the record among the case's
# profile records) -> (the parent's value, the route's family, the route's variant, the value derived from the route).  Everything else of
# such a case is compared as usual; tests/test_conv_host_cpu.py asserts the route-derived value for these records.
#
# All of them are the level-0 decoder convolution on the upsampled map (dec.0.1), where the earlier code took "3x3, reflection padding,
# upsampled 16-channel source" to mean the merged-tap halo kernels (4 taps of 9) without asking what the planner asks as well:
#   * conv_fwd with statistics: the halo kernel has no statistics epilogue; the planner gives the fp32 offset-table kernel, all 9 taps
#     (family IGEMM_FP32, variant RV_TABLE);
#   * conv_wgrad with tile bit 10 (TILE_HALO_9TAP): the halo weight-gradient kernel in its 9-tap form (family WGRAD_HALO, variant 0).
# Neither is a launch the networks make.  Rows: size, record indices, tile switches (under every spec.mma), parent's executed, family, variant,
# the route-derived executed (= the record's flops).
_CORRECTED_ROWS = (
    ("2x48x64", (2, 3), (0, 1 << 11, 1 << 12), "0x1.8000000000000p+23", 0, 0x400, "0x1.b000000000000p+24"),
    ("2x48x64", (10,), (1 << 10,), "0x1.8000000000000p+23", 1, 0, "0x1.b000000000000p+24"),
    ("3x9x33", (2,), (0, 1 << 11, 1 << 12), "0x1.fe00000000000p+20", 0, 0x400, "0x1.1ee0000000000p+22"),
    ("3x9x33", (9,), (1 << 10,), "0x1.fe00000000000p+20", 1, 0, "0x1.1ee0000000000p+22"),
    ("1x7x21", (2,), (0, 1 << 11, 1 << 12), "0x1.6000000000000p+18", 0, 0x400, "0x1.8c00000000000p+19"),
    ("1x7x21", (9,), (1 << 10,), "0x1.6000000000000p+18", 1, 0, "0x1.8c00000000000p+19"),
    ("12x192x640", (2, 3), (0, 1 << 11, 1 << 12), "0x1.6800000000000p+31", 0, 0x400, "0x1.9500000000000p+32"),
    ("12x192x640", (10,), (1 << 10,), "0x1.6800000000000p+31", 1, 0, "0x1.9500000000000p+32"),
)
EXECUTED_CORRECTED = {("layer dec.0.1 %s mma%d tile%#x" % (size, mma, tile), i): (parent, family, variant, value)
                      for size, records, tiles, parent, family, variant, value in _CORRECTED_ROWS
                      for mma in MMAS for tile in tiles for i in records}


def _t(*shape):
    return torch.empty(shape, dtype=torch.float32)


def _param(*shape):
    return torch.nn.Parameter(_t(*shape))


def make_spec(N, layer, mma):
    bias = _param(layer.cout) if (layer.reflect or layer.name.startswith("pose.")) else None
    spec = N.ConvSpec(_param(layer.cout, layer.cin, layer.k, layer.k), bias, layer.stride, layer.pad,
                      N.PAD_REFLECT if layer.reflect else N.PAD_ZERO, smallc=(layer.kind == "depth_stem"))
    spec.mma = mma
    return spec


def _bn_state(N, C, groups):
    st = N.BNState()
    st.scale, st.shift, st.mean, st.invstd, st.groups = _t(groups, C), _t(groups, C), _t(groups, C), _t(groups, C), groups
    return st


def _attempt(log, what, fn):
    """A refusal (the planner's, or the host layer's own) is part of the log."""
    from mcav import lib as L
    log.note("# " + what)
    try:
        fn()
    except L.MCAVError as e:
        log.note("MCAVError: %s" % e)


def layer_body(log, layer, size, mma, tile):
    from mcav import nn as N
    B, Hs, Ws = K.source_size(layer, size)
    Hd, Wd = K.out_size(Hs, layer.k, layer.stride, layer.pad), K.out_size(Ws, layer.k, layer.stride, layer.pad)
    c1 = layer.cin - layer.c2
    xc = 4 if layer.kind == "depth_stem" else 16 if layer.kind == "pose_stem" else c1
    x1 = _t(B, Hs // 2, Ws // 2, xc) if layer.up else _t(B, Hs, Ws, xc)
    x2 = _t(B, Hs, Ws, layer.c2) if layer.c2 else None
    up = bool(layer.up)
    act = N.ACT_ELU if layer.reflect else N.ACT_RELU
    spec = make_spec(N, layer, mma)
    go = lambda what, fn: _attempt(log, what, fn)

    go("fwd", lambda: N.conv_fwd(spec, x1, x2, up1=up, tile=tile))
    go("fwd act", lambda: N.conv_fwd(spec, x1, x2, up1=up, act=act, tile=tile))
    go("fwd stats", lambda: N.conv_fwd(spec, x1, x2, up1=up, stats=True, tile=tile))
    go("fwd stats groups=2", lambda: N.conv_fwd(spec, x1, x2, up1=up, stats=True, tile=tile, groups=2))
    planar = []
    if layer.kind == "depth_stem":
        planar = [("one image", lambda: N.PlanarImages([_t(B, 3, Hs, Ws)], N.PLANAR_BATCH, 4), 1)]
        if B % 2 == 0:
            planar.append(("pair", lambda: N.PlanarImages([_t(B // 2, 3, Hs, Ws), _t(B // 2, 3, Hs, Ws)], N.PLANAR_BATCH, 4), 2))
    elif layer.kind == "pose_stem":
        planar = [("three images", lambda: N.PlanarImages([_t(B, 3, Hs, Ws) for _ in range(3)], N.PLANAR_CHANNELS, 16), 1)]
    for name, make, groups in planar:
        go("fwd planar " + name, lambda: N.conv_fwd(spec, make(), act=act, tile=tile))
        go("fwd planar stats " + name, lambda: N.conv_fwd(spec, make(), stats=True, groups=groups, tile=tile))

    dy = _t(B, Hd, Wd, layer.cout)
    if layer.kind == "conv" and Hd >= 1 and Wd >= 1:
        xin = _t(B, Hs, Ws, layer.cin)
        go("dgrad whole", lambda: N.conv_dgrad(spec, dy, (Hs, Ws), tile=tile))
        go("dgrad addend", lambda: N.conv_dgrad(spec, dy, (Hs, Ws), addend=xin, tile=tile))
        go("dgrad dact addend", lambda: N.conv_dgrad(spec, dy, (Hs, Ws), dact_aux=xin, dact=act, addend=xin, tile=tile))
        if layer.up:
            a = _t(B, Hs // 2, Ws // 2, c1)
            go("dgrad pooled", lambda: N.conv_dgrad(spec, dy, (Hs, Ws), n_begin=0, n_count=c1, dact_aux=a, dact=N.ACT_ELU, pool=True, tile=tile))
            go("dgrad pooled addend", lambda: N.conv_dgrad(spec, dy, (Hs, Ws), n_begin=0, n_count=c1, dact_aux=a, dact=N.ACT_ELU, addend=a, pool=True, tile=tile))
        if layer.c2:
            go("dgrad skip", lambda: N.conv_dgrad(spec, dy, (Hs, Ws), n_begin=c1, n_count=layer.c2, tile=tile))
        if layer.stride == 1 and not layer.reflect:
            for groups in (1, 2):
                st = _bn_state(N, layer.cin, groups)
                go("dgrad bn_stats groups=%d" % groups,
                   lambda: N.conv_dgrad(spec, dy, (Hs, Ws), dact_aux=xin, dact=N.ACT_RELU, bn_stats=(xin, st), tile=tile))
                go("dgrad bn_stats after addend groups=%d" % groups,
                   lambda: N.conv_dgrad(spec, dy, (Hs, Ws), addend=xin, dact_aux=xin, dact=N.ACT_RELU | N.DACT_AFTER_ADDEND, bn_stats=(xin, st), tile=tile))
        go("dgrad after addend", lambda: N.conv_dgrad(spec, dy, (Hs, Ws), addend=xin, dact_aux=xin, dact=N.ACT_RELU | N.DACT_AFTER_ADDEND, tile=tile))

    go("wgrad", lambda: N.conv_wgrad(spec, x1, dy, x2=x2, up1=up, tile=tile))
    if layer.kind != "conv":
        st = _bn_state(N, layer.cout, 1)
        bn = N.DyBn(_t(B, Hd, Wd, layer.cout), _t(layer.cout), st.mean, st.invstd, _t(1, 2, layer.cout), 1)
        go("wgrad dy_bn", lambda: N.conv_wgrad(spec, x1, dy, tile=tile, dy_bn=bn))
        for name, make, groups in planar:
            go("wgrad planar " + name, lambda: N.conv_wgrad(spec, make(), dy, tile=tile))
            go("wgrad planar dy_bn " + name, lambda: N.conv_wgrad(spec, make(), dy, tile=tile, dy_bn=bn))


def deconv_body(log, cin, cout, in_shape, out_hw, mma):
    from mcav import nn as N
    from mcav import tape as T
    ds = T.DeconvSpec(_param(cin, cout, 3, 3), _param(cout))
    ds.as_conv.mma = mma
    tape = T.Tape()
    x = _t(*in_shape, cin)
    y = T.deconv(tape, ds, x, out_hw)
    log.note("# backward")
    tape.backward([(y, _t(*y.shape))])
    assert tape.grad(x) is not None and N.grad_buffer(ds.weight) is not None


def _images(n):
    B, H, W = NET_SIZE
    return [torch.zeros((B, 3, H, W), dtype=torch.float32) for _ in range(n)]


def _backward(outs):
    sum(o.sum() for o in outs).backward()


def network_body(log, net, dtype, mode):
    from mcav import nn as N
    from models.depth.disp_net import DispNetS
    from models.depth.resnet_dispnet import DispResNet
    from models.pose.pose_net import PoseNet
    model = {"r18": DispResNet, "r50": lambda: DispResNet(num_layers=50), "pose": PoseNet, "dispnets": DispNetS}[net]()
    if dtype is not None:
        N.set_compute_dtype(model, dtype)
    if mode == "eval":
        model.eval()
        with torch.no_grad():
            model(*_images(1)) if net != "pose" else model(_images(1)[0], _images(2))
        return
    model.train()
    if net in ("r18", "r50"):
        a, b = model.forward_pair(*_images(2))
        log.note("# backward")
        _backward(a + b)
    elif net == "pose":
        out = model(_images(1)[0], _images(2))
        log.note("# backward")
        _backward([out])
    else:
        outs = model(*_images(1))
        log.note("# backward")
        _backward(outs)


def _layer_sizes(layer):
    return SIZES + ((BIG,) if layer.name in BIG_LAYERS else ())


def all_cases():
    """-> {name: (mode, body(log))}, in a fixed order."""
    cases = {}
    for layer in K.LAYERS:
        for size in _layer_sizes(layer):
            for mma in MMAS:
                for tile in TILES:
                    cases["layer %s %dx%dx%d mma%d tile%#x" % (layer.name, *size, mma, tile)] = \
                        ("full", lambda log, a=(layer, size, mma, tile): layer_body(log, *a))
    for cin, cout, in_shape, out_hw in ((32, 16, (2, 24, 32), (48, 64)), (512, 512, (3, 1, 2), (1, 3))):
        for mma in MMAS:
            cases["deconv %d->%d %s->%s mma%d" % (cin, cout, "x".join(map(str, in_shape)), "x".join(map(str, out_hw)), mma)] = \
                ("full", lambda log, a=(cin, cout, in_shape, out_hw, mma): deconv_body(log, *a))
    for net in ("r18", "r50", "pose", "dispnets"):
        for dtype in DTYPES:
            for mode in ("train", "eval"):
                cases["net %s %s %s" % (net, dtype or "default", mode)] = ("sequence", lambda log, a=(net, dtype, mode): network_body(log, *a))
    return cases


def run(case, routes=False):
    """-> [(log, routes)] of the case's two runs: mcav.nn.PROFILE off, then a list.  routes: also the planned route of every conv launch of
    a run (mcav.nn.ROUTES), for reading a record against the planner -- the log itself does not depend on it."""
    from mcav import nn as N
    mode, body = case
    out = []
    for profile in (False, True):
        with H.recording(mode, profile) as log:
            N.ROUTES = [] if routes else None
            try:
                body(log)
            finally:
                planned, N.ROUTES = N.ROUTES, None
        out.append((log, planned))
    return out


def canonical(name, runs):
    """The text whose sha256 is recorded: both runs' calls, then the profiled run's records (without `executed` where EXECUTED_CORRECTED
    lists the record)."""
    text = []
    for (log, _), title in zip(runs, ("PROFILE = None", "PROFILE = []")):
        text.append("== %s\n%s" % (title, log.text()))
        for i, (rec, tag) in enumerate(log.profile):
            text.append(H.profile_line(rec, tag, "corrected" if (name, i) in EXECUTED_CORRECTED else None) + "\n")
    return "".join(text)


def dump(name, case):
    """canonical() with every profile record's `executed` and, beside each timed launch of the profiled run, the route the planner gave."""
    runs = run(case, routes=True)
    text = canonical(name, runs)
    log, planned = runs[1]
    lines = ["== planned routes of the profiled run, in launch order"]
    for kind, r in planned:
        lines.append("route %s family=%d variant=%#x tile=%d splits=%d" % (kind, r.family, r.variant, r.tile, r.splits))
    for i, (rec, tag) in enumerate(log.profile):
        lines.append("executed[%d] = %s (%r)" % (i, float(rec.executed).hex(), rec.executed / rec.flops if rec.flops else 0.0))
    return text + "\n".join(lines) + "\n"


def hashes(names=None):
    cases = all_cases()
    return {name: H.digest(canonical(name, run(cases[name]))) for name in (names or cases)}

