"""A deterministic sweep of convolution descriptors for the planner tests (tests/test_conv_plan_cpu.py, tests/golden/make_conv_plan_golden.py):
every layer of the R18 DispResNet encoder and decoder, the R50 bottleneck shapes and PoseNet, at four image sizes, as forward, data-gradient
and weight-gradient launches, crossed with the switches the planner reads (mma, tile ids and bits, statistics forms, merged-tap / stem / planar
sources).  No tensors: the planner entries never dereference a pointer, so small non-null constants stand in for device addresses.

The full cross product is thinned by fixed strides (every base descriptor is kept), so the sweep is the same list on every run; the recorded
answers in tests/golden/conv_plan_parent.npz are indexed by position in it."""
import contextlib
import ctypes
from collections import namedtuple

X1, X2, W, Y, W16, AUX, ADD, STATS, SX, SM, SI, WUP, WSTEM, DY, DW, DB, PL0, PL1, PL2, BN = (0x1000 * (i + 1) for i in range(20))

SIZES = ((12, 192, 640), (2, 48, 64), (3, 9, 33), (1, 7, 21))
MMAS = (0, 1, 2, 3)
TILES = (0, 1, 2, 7, 10, 12, 0x33) + tuple(1 << b for b in range(8, 17)) + (3 << 14,)
IGEMM_THIN, FORCED_THIN, WGRAD_THIN = 29, 5, 7
FORCED = (0x33, 1 << 13, 1 << 14, 1 << 15, 3 << 14)      # the opt-in kernels' switches: kept more densely (few descriptors qualify)

# cin, cout, k, stride, pad, reflect, div (the input is 1/div of the image), c2 (skip channels of a two-source layer), up (x1 is upsampled), kind
Layer = namedtuple("Layer", "name cin cout k stride pad reflect div c2 up kind")


def _enc(name, cin, cout, k, s, div):
    return Layer(name, cin, cout, k, s, k // 2, 0, div, 0, 0, "conv")


def _dec(name, c1, c2, cout, div, up):
    return Layer(name, c1 + c2, cout, 3, 1, 1, 1, div, c2, up, "conv")


LAYERS = (
    # R18 encoder
    Layer("r18.conv1", 3, 64, 7, 2, 3, 0, 1, 0, 0, "depth_stem"),
    _enc("r18.layer1", 64, 64, 3, 1, 4), _enc("r18.layer2.0", 64, 128, 3, 2, 4), _enc("r18.layer2", 128, 128, 3, 1, 8),
    _enc("r18.layer2.down", 64, 128, 1, 2, 4), _enc("r18.layer3.0", 128, 256, 3, 2, 8), _enc("r18.layer3", 256, 256, 3, 1, 16),
    _enc("r18.layer3.down", 128, 256, 1, 2, 8), _enc("r18.layer4.0", 256, 512, 3, 2, 16), _enc("r18.layer4", 512, 512, 3, 1, 32),
    _enc("r18.layer4.down", 256, 512, 1, 2, 16),
    # R18 decoder: upconv(i, 0) on the level's map, upconv(i, 1) on cat(up2(.), skip)
    _dec("dec.4.0", 512, 0, 256, 32, 0), _dec("dec.4.1", 256, 256, 256, 16, 1), _dec("dec.3.0", 256, 0, 128, 16, 0),
    _dec("dec.3.1", 128, 128, 128, 8, 1), _dec("dec.2.0", 128, 0, 64, 8, 0), _dec("dec.2.1", 64, 64, 64, 4, 1),
    _dec("dec.1.0", 64, 0, 32, 4, 0), _dec("dec.1.1", 32, 64, 32, 2, 1), _dec("dec.0.0", 32, 0, 16, 2, 0), _dec("dec.0.1", 16, 0, 16, 1, 1),
    # R50 bottlenecks and the decoder levels its wider skips change
    _enc("r50.l1.a", 64, 64, 1, 1, 4), _enc("r50.l1.c", 64, 256, 1, 1, 4), _enc("r50.l1.a2", 256, 64, 1, 1, 4),
    _enc("r50.l2.a", 256, 128, 1, 1, 4), _enc("r50.l2.b", 128, 128, 3, 2, 4), _enc("r50.l2.c", 128, 512, 1, 1, 8),
    _enc("r50.l2.down", 256, 512, 1, 2, 4), _enc("r50.l3.b", 256, 256, 3, 2, 8), _enc("r50.l3.c", 256, 1024, 1, 1, 16),
    _enc("r50.l4.a", 1024, 512, 1, 1, 16), _enc("r50.l4.b", 512, 512, 3, 2, 16), _enc("r50.l4.c", 512, 2048, 1, 1, 32),
    _dec("r50.dec.4.0", 2048, 0, 256, 32, 0), _dec("r50.dec.4.1", 256, 1024, 256, 16, 1), _dec("r50.dec.2.1", 64, 256, 64, 4, 1),
    # PoseNet
    Layer("pose.conv1", 9, 16, 7, 2, 3, 0, 1, 0, 0, "pose_stem"),
    _enc("pose.conv2", 16, 32, 5, 2, 2), _enc("pose.conv3", 32, 64, 3, 2, 4), _enc("pose.conv4", 64, 128, 3, 2, 8),
    _enc("pose.conv5", 128, 256, 3, 2, 16), _enc("pose.conv6", 256, 256, 3, 2, 32), _enc("pose.conv7", 256, 256, 3, 2, 64),
    _enc("pose.pred", 256, 12, 1, 1, 128),
)


def up16(v):
    return (v + 15) // 16 * 16


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def source_size(layer, size):
    """(B, Hs, Ws) of the layer's logical input at an image size; an upsampled source is twice its stored map (an odd size stays odd elsewhere)."""
    B, H, W = size
    if layer.up:
        return B, 2 * max(1, -(-H // (2 * layer.div))), 2 * max(1, -(-W // (2 * layer.div)))
    return B, max(1, -(-H // layer.div)), max(1, -(-W // layer.div))


def _stats_forms(direction):
    """name -> fields: off, on, on with two groups, the BatchNorm-backward (stats_x) form"""
    on = dict(stats=STATS)
    sx = dict(stats=STATS, stats_x=SX, stats_mean=SM, stats_invstd=SI)
    return (dict(), on, dict(on, groups=2), sx if direction != "fwd" else dict(sx, groups=2))


def _set(d, **kw):
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _copy(d):
    c = type(d)()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(d), ctypes.sizeof(d))
    return c


def igemm_forward(N, layer, size):
    B, Hs, Ws = source_size(layer, size)
    c1 = layer.cin - layer.c2
    d = N.IgemmDesc()
    smallc = layer.kind == "depth_stem"
    d.x1, d.x2 = X1, (X2 if layer.c2 else None)
    d.B, d.Hs, d.Ws, d.C1, d.C2, d.up1 = B, Hs, Ws, (4 if smallc else 16 if layer.kind == "pose_stem" else c1), layer.c2, layer.up
    d.w, d.kh, d.kw, d.Np, d.Kp = W, layer.k, layer.k, up16(layer.cout), (4 if smallc else up16(layer.cin))
    d.mode = N.G_SMALLC if smallc else N.G_DIRECT
    d.stride, d.sign, d.offset, d.pad_mode = layer.stride, 1, -layer.pad, (N.PAD_REFLECT if layer.reflect else N.PAD_ZERO)
    d.y, d.Hd, d.Wd = Y, out_size(Hs, layer.k, layer.stride, layer.pad), out_size(Ws, layer.k, layer.stride, layer.pad)
    d.Cd, d.n_begin, d.n_count, d.y_choff = layer.cout, 0, layer.cout, 0
    d.bias, d.act, d.groups = DB, N.ACT_ELU if layer.reflect else N.ACT_NONE, 1
    return d


def igemm_dgrads(N, layer, size):
    """The data-gradient launches of a layer: (name, descriptor) -- the three adjoint gathers, pooled, channel sub-ranges."""
    if layer.kind != "conv":
        return []
    B, Hs, Ws = source_size(layer, size)
    Hd, Wd = out_size(Hs, layer.k, layer.stride, layer.pad), out_size(Ws, layer.k, layer.stride, layer.pad)
    if Hd < 1 or Wd < 1:
        return []
    c1 = layer.cin - layer.c2
    d = N.IgemmDesc()
    d.x1, d.B, d.Hs, d.Ws, d.C1 = X1, B, Hd, Wd, up16(layer.cout)
    d.w, d.kh, d.kw, d.Np, d.Kp = W, layer.k, layer.k, up16(layer.cin), up16(layer.cout)
    if layer.stride == 1:
        d.mode, d.stride, d.sign, d.offset = (N.G_ADJ_REFLECT if layer.reflect else N.G_DIRECT), 1, -1, layer.pad
    else:
        d.mode, d.stride, d.sign, d.offset = N.G_ADJ_STRIDE2, 2, -1, layer.pad
    d.pad_mode = N.PAD_ZERO
    d.y, d.Hd, d.Wd, d.Cd, d.n_begin, d.n_count = Y, Hs, Ws, layer.cin, 0, layer.cin
    d.groups = 1
    out = [("whole", d)]
    if layer.up:                              # the upsampled source's share, 2x2 sum-pooled
        out.append(("pooled", _set(_copy(d), pool=1, n_count=c1, Cd=c1, dact_aux=AUX, dact=N.ACT_ELU)))
    if layer.c2:                              # the skip tensor's share: a filter-row sub-range, and the same into a wider pixel
        out.append(("skip", _set(_copy(d), n_begin=c1, n_count=layer.c2, Cd=layer.c2, addend=ADD)))
        out.append(("skip choff", _set(_copy(d), n_begin=c1, n_count=layer.c2, y_choff=c1)))
        m = N.IgemmDesc()                     # d / d(low-resolution map) as a 4x4 stride-2 conv of dy on the edge-replicated domain (mcav_conv.h)
        m.x1, m.B, m.Hs, m.Ws, m.C1 = X1, B, Hd, Wd, up16(layer.cout)
        m.w, m.kh, m.kw, m.Np, m.Kp = W, 4, 4, up16(c1), up16(layer.cout)
        m.mode, m.stride, m.sign, m.offset, m.pad_mode = N.G_DIRECT, 2, 1, -3, N.PAD_ZERO
        m.y, m.Hd, m.Wd, m.Cd, m.n_begin, m.n_count, m.groups = Y, Hs // 2 + 2, Ws // 2 + 2, c1, 0, c1, 1
        out.append(("merged 4x4", m))
    else:
        out.append(("after addend", _set(_copy(d), dact_aux=AUX, dact=N.ACT_RELU | N.DACT_AFTER_ADDEND, addend=ADD)))
    return out


def igemm_sweep(N):
    """-> (names, descriptors).  Position i of both is case i of the recorded answers."""
    names, descs = [], []
    count = 0
    for li, layer in enumerate(LAYERS):
        for size in SIZES:
            launches = [("fwd", "fwd", igemm_forward(N, layer, size))] + [("dgrad", n, d) for n, d in igemm_dgrads(N, layer, size)]
            for direction, what, base in launches:
                for mma in MMAS:
                    for tile in TILES:
                        for si, stats in enumerate(_stats_forms(direction)):
                            count += 1
                            if not (tile == 0 and si == 0) and count % IGEMM_THIN and (tile not in FORCED or count % FORCED_THIN):
                                continue
                            d = _set(_copy(base), mma=mma, tile=tile, w16=(W16 if mma else None), **stats)
                            extra = ""
                            if direction == "fwd" and layer.kind != "conv" and count % 4:      # the stems: w_stem mostly, planar sources sometimes
                                d.w_stem = WSTEM
                                if count % 3 == 0:
                                    depth = layer.kind == "depth_stem"
                                    d.x1 = None if count % 2 else X1
                                    d.x_planar[0], d.x_planar[1], d.x_planar[2] = PL0, (PL1 if not depth or size[0] % 2 == 0 else None), (None if depth else PL2)
                                    d.planar_B = size[0] // 2 if depth and size[0] % 2 == 0 else size[0]
                                    d.planar_stack = 1 if depth else 2
                                    extra = " planar"
                            if direction == "fwd" and layer.c2 and layer.up and count % 2:
                                d.w_upmerge = WUP
                                extra = " upmerge"
                            if direction == "fwd" and layer.kind == "conv" and not layer.c2 and count % 29 == 0:
                                d.x_planar[0], d.planar_B, d.planar_stack = PL0, size[0], 1      # planar sources on a launch that is no stem: refused
                                extra = " planar (no stem)"
                            names.append("%s %s %s%s %dx%dx%d mma%d tile%#x stats%d" % (layer.name, direction, what, extra, *size, mma, tile, si))
                            descs.append(d)
    # descriptors fill_params refuses, from a launchable one
    base = igemm_forward(N, LAYERS[1], SIZES[1])
    for name, change in (("Cd zero", dict(Cd=0)), ("y_choff past Cd", dict(y_choff=16)), ("n_count past Np", dict(n_count=80, Cd=80)),
                         ("kh zero", dict(kh=0)), ("64 < taps", dict(kh=9, kw=9)), ("Kp below C1", dict(Kp=48)), ("x1 null", dict(x1=None)),
                         ("pool with stats", dict(pool=1, stats=STATS)), ("stats_x without stats", dict(stats_x=SX)), ("B zero", dict(B=0))):
        names.append("refused: " + name)
        descs.append(_set(_copy(base), **change))
    return names, descs


def wgrad_launches(N, layer, size):
    """The weight-gradient launches of a layer: plain, a channel window of a wider dy, the two halves of a two-source filter (skip half with
    Cin_total / ci_offset, merged-tap upsampled half), each with and without the bias gradient."""
    B, Hs, Ws = source_size(layer, size)
    Hd, Wd = out_size(Hs, layer.k, layer.stride, layer.pad), out_size(Ws, layer.k, layer.stride, layer.pad)
    if Hd < 1 or Wd < 1:
        return []
    smallc = layer.kind == "depth_stem"
    c1 = layer.cin - layer.c2
    d = N.WgradDesc()
    d.x1, d.x2 = X1, (X2 if layer.c2 else None)
    d.B, d.Hs, d.Ws, d.C1, d.C2, d.up1 = B, Hs, Ws, (4 if smallc else 16 if layer.kind == "pose_stem" else c1), layer.c2, layer.up
    d.kh, d.kw, d.Kp = layer.k, layer.k, (4 if smallc else up16(layer.cin))
    d.mode = N.G_SMALLC if smallc else N.G_DIRECT
    d.stride, d.sign, d.offset, d.pad_mode = layer.stride, 1, -layer.pad, (N.PAD_REFLECT if layer.reflect else N.PAD_ZERO)
    d.dy, d.Hd, d.Wd, d.Cdy, d.dy_choff = DY, Hd, Wd, up16(layer.cout), 0
    d.Cout, d.Cin, d.dw_oihw, d.accumulate, d.dbias = layer.cout, layer.cin, DW, 1, DB
    out = [("plain", d), ("no dbias", _set(_copy(d), dbias=None)), ("dy_choff", _set(_copy(d), Cdy=up16(layer.cout) + 16, dy_choff=16))]
    if layer.c2:
        skip = _set(_copy(d), x1=X2, x2=None, C1=layer.c2, C2=0, up1=0, Kp=up16(layer.c2), Cin=layer.c2, Cin_total=layer.cin, ci_offset=c1)
        out.append(("skip half", skip))
        out.append(("upm half", _set(_copy(d), x2=None, C2=0, Kp=c1, Cin=c1, Cin_total=layer.cin, ci_offset=0, upm=1, dbias=None)))
        out.append(("upm half with dbias", _set(_copy(d), x2=None, C2=0, Kp=c1, Cin=c1, Cin_total=layer.cin, ci_offset=0, upm=1)))      # refused
        out.append(("skip half past Cin_total", _set(_copy(skip), ci_offset=c1 + 16)))                                                   # refused
    if layer.kind == "depth_stem":
        fold = dict(dy_bn_x=BN, dy_bn_gamma=BN, dy_bn_mean=BN, dy_bn_invstd=BN, dy_bn_sums=BN, dy_bn_groups=1, dy_bn_inv_count=1.0 / (B * Hd * Wd), dbias=None)
        out.append(("bn fold", _set(_copy(d), **fold)))
        out.append(("bn fold with dbias", _set(_copy(d), **dict(fold, dbias=DB))))                                                        # refused
    if layer.kind != "conv":
        depth = layer.kind == "depth_stem"
        p = _copy(d)
        p.x1 = None
        p.x_planar[0], p.x_planar[1], p.x_planar[2] = PL0, (None if depth else PL1), (None if depth else PL2)
        p.planar_B, p.planar_stack = B, (1 if depth else 2)
        out.append(("planar", p))
    return out


WGRAD_TILES = (0, 1, 2, 3, 4, 6, 7, 5, 1 << 8, 1 << 9, 1 << 10)


def wgrad_sweep(N):
    names, descs = [], []
    count = 0
    for layer in LAYERS:
        for size in SIZES:
            for what, base in wgrad_launches(N, layer, size):
                for mma in MMAS:
                    for tile in WGRAD_TILES:
                        count += 1
                        if tile and count % WGRAD_THIN:
                            continue
                        names.append("%s wgrad %s %dx%dx%d mma%d tile%#x" % (layer.name, what, *size, mma, tile))
                        descs.append(_set(_copy(base), mma=mma, tile=tile))
    return names, descs


def as_array(descs):
    return (type(descs[0]) * len(descs))(*descs)


# the fields _weights_for has not settled when it asks mcav_igemm_uses_bf16: every combination of them set / cleared
def unsettled_copies(d):
    for bits in range(8):
        c = _copy(d)
        c.stats = STATS if bits & 1 else None
        if not c.stats:
            c.stats_x = None
        c.groups = 2 if bits & 2 else 1
        c.w_stem = WSTEM if bits & 4 else None
        yield c


@contextlib.contextmanager
def recorded_routes(N):
    """GPU tests: the (kind, ConvRoute) of every conv_fwd / conv_dgrad / conv_wgrad launch inside the block, as mcav_igemm_route / mcav_wgrad_route planned it before the launch."""
    N.ROUTES = log = []
    try:
        yield log
    finally:
        N.ROUTES = None
