"""GPU: the pillar feature net's backward (include/mcav_depth.h: mcav_pillar_pseudo_image_bwd, pseudo_lidar.PillarFeatureNet.gradients, the
autograd node behind features / pseudo_image, PillarFeatureLayer) against its restatement (tests/pfn_bwd_ref.py): d_voxels bit for bit
(NaNs by class), the three sums within one float32 rounding of the restatement's float64 sums plus 2^-32 of their terms' magnitudes, on
the cases of tests/pfn_cases.py in both layouts and with both paddings; sentinels in every output; a capacity below the count; the
gradient sources; a grid-stride case; repeatability; graph capture and replay on new contents; autograd against the raw call; a short
training run; the C ABI's refusals."""
import numpy as np
import pytest
import torch

import pfn_bwd_ref as BR
import pfn_cases as C
import pfn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -7.0
SLACK = 5                                                    # rows of the buffers behind the pillars
CHUNK, GRID = 64, 1024                                       # csrc/pfn_bwd_math.h: rows a workgroup takes at a time, workgroups at most


def product_grid(nx, ny):
    from pseudo_lidar import PillarGrid
    g = PillarGrid(x=(0.0, float(nx)), y=(0.0, float(ny)), z=(-1.0, 1.0), size=(1.0, 1.0))
    assert (g.nx, g.ny) == (nx, ny)
    return g


def batch(a, capacity=None):
    """the case's pillars on the device in buffers of `capacity` rows (default: SLACK more than there are pillars), the rest sentinels"""
    from pseudo_lidar import PillarBatch
    P, N, Cc = a["voxels"].shape
    cap = P + SLACK if capacity is None else capacity
    pb = PillarBatch(len(a["offsets"]) - 1, cap, N, Cc, DEV)
    pb.voxels.fill_(SENTINEL); pb.coords.fill_(1 << 20); pb.num_points.fill_(1 << 20)
    k = min(P, cap)
    pb.voxels[:k], pb.coords[:k], pb.num_points[:k] = (torch.from_numpy(a[n][:k].copy()).to(DEV) for n in ("voxels", "coords", "num_points"))
    pb.offsets.copy_(torch.from_numpy(a["offsets"].copy()))
    pb.grid = product_grid(a["nx"], a["ny"])
    return pb


def tensor(v):
    return torch.from_numpy(np.array(v, F)).to(DEV)


def layer(a, pad="bias"):
    from pseudo_lidar import PillarFeatureNet
    return PillarFeatureNet(tensor(a["weight"]), tensor(a["bias"]), None if pad == "bias" else tensor(C.bias_pad(a, pad)))


def canvas_gradient(dc, layout):
    t = torch.from_numpy(np.array(dc, F)).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else t


def feature_gradient(df, cap):
    """the case's rows, and sentinels that must never be read behind them"""
    t = torch.full((cap, df.shape[1]), float("nan"), device=DEV)
    k = min(cap, len(df))
    t[:k] = torch.from_numpy(df[:k].copy()).to(DEV)
    return t


def sentinels(net, pb, voxels=True):
    shapes = [(net.c_out, net.columns), (net.c_out,), (net.c_out,)] + ([tuple(pb.voxels.shape)] if voxels else [])
    return [torch.full(s, SENTINEL, device=DEV) for s in shapes]


def check(got, want, P):
    """d_voxels bit for bit below the pillar count and +0.0 behind it; the sums within the bound"""
    dw, db, dp, dv = (None if t is None else t.cpu().numpy() for t in got)
    if dv is not None:
        C.same_bits(np.ascontiguousarray(dv[:P]), want["d_voxels"][:P])
        assert (dv[P:].view(np.uint32) == 0).all()
    BR.check_sums((dw, db, dp), want)


@pytest.mark.parametrize("pad", ["bias", "zero"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("case", C.CASES)
def test_kernel_matches_restatement(case, layout, pad):
    a, want = C.build(case), BR.reference(case, pad)
    dc, _ = BR.upstream_canvas(case)
    pb, net = batch(a), layer(a, pad)
    out = sentinels(net, pb)
    got = net.gradients(pb, grad_canvas=canvas_gradient(dc, layout), layout=layout, need_voxels=True, out=out)
    assert all(g is o for g, o in zip(got, out))
    check(got, want, len(want["slot"]))
    finite = np.isfinite(a["voxels"]).all(axis=(1, 2))
    assert (want["slot"][finite, 1] == BR.NO_FLOW).all()                                   # channel 1: +0.0 for finite points, no gradient
    assert float(got[1][1]) == 0.0 or not finite.all()
    if pad == "bias" and (a["num_points"] < a["voxels"].shape[1]).any():
        assert (want["slot"][:, 2] == BR.PADDING).any() and float(got[2][2]) != 0.0       # channel 2: the padding wins
    if pad == "zero":
        assert bool((got[2] == 0).all())


def test_real_grid_more_than_one_workgroup():
    """B = 2 on the 432 x 496 grid, 3 985 pillars: 63 workgroups leave a column in the slab"""
    a, want = C.build(C.REAL_CASE), BR.reference(C.REAL_CASE)
    dc, _ = BR.upstream_canvas(C.REAL_CASE)
    pb, net = batch(a), layer(a)
    assert 1 < -(-pb.voxels.shape[0] // CHUNK) < GRID
    for layout in ("nchw", "nhwc"):
        got = net.gradients(pb, grad_canvas=canvas_gradient(dc, layout), layout=layout, need_voxels=True, out=sentinels(net, pb))
        check(got, want, len(want["slot"]))


def test_grid_stride_second_round():
    """70 000 single-point pillars at C_out = 32, B = 1: 1 094 chunks on the 1 024 workgroups, so the first 70 take a second round"""
    P, nx, ny = 70000, 256, 280
    cells = np.arange(P)
    rows = [(0, int(c // nx), int(c % nx), 1) for c in cells]
    vox, coords, num, off = C.planted(rows, 1, 2, 4, 31)
    w, b = C.layer(32, 4, 1036)
    assert -(-(P + SLACK) // CHUNK) > GRID
    rng = np.random.RandomState(32)
    dc = rng.standard_normal((1, 32, ny, nx)).astype(F)
    a = dict(voxels=vox, coords=coords, num_points=num, offsets=off, nx=nx, ny=ny, weight=w, bias=b)
    want = BR.gradients(vox, coords, num, off, nx, ny, w, b, d_canvas=dc)
    assert (want["slot"] >= 0).any() and (want["slot"] == BR.PADDING).any()
    pb, net = batch(a), layer(a)
    for layout in ("nchw", "nhwc"):
        got = net.gradients(pb, grad_canvas=canvas_gradient(dc, layout), layout=layout, need_voxels=True, out=sentinels(net, pb))
        check(got, want, P)


def test_capacity_ends_inside_the_second_image():
    case = "wide-o128"
    a = C.build(case)
    cap = C.cut_capacity(case)
    want, full = BR.reference(case, "bias", "canvas", cap), BR.reference(case)
    assert len(want["slot"]) == cap < len(full["slot"]) and not np.array_equal(want["d_bias"], full["d_bias"])
    dc, _ = BR.upstream_canvas(case)
    pb, net = batch(a, capacity=cap), layer(a)
    for layout in ("nchw", "nhwc"):
        got = net.gradients(pb, grad_canvas=canvas_gradient(dc, layout), layout=layout, need_voxels=True, out=sentinels(net, pb))
        check(got, want, cap)
    roomy = batch(a, capacity=len(a["coords"]) + 70)         # more than a chunk of rows behind the last pillar: all +0.0
    got = net.gradients(roomy, grad_canvas=canvas_gradient(dc, "nchw"), need_voxels=True, out=sentinels(net, roomy))
    check(got, full, len(full["slot"]))


@pytest.mark.parametrize("case", ["wide-o128", "pair-N5-c9-o64"])
def test_gradient_sources(case):
    """d_features alone, both together, and need_voxels=False, which leaves a d_voxels buffer alone"""
    a = C.build(case)
    dc, df = BR.upstream_canvas(case)
    pb, net = batch(a), layer(a)
    P, cap = len(a["coords"]), pb.voxels.shape[0]
    gf = feature_gradient(df, cap)                                                        # NaNs behind the pillars: never read
    got = net.gradients(pb, grad_features=gf, need_voxels=True, out=sentinels(net, pb))
    check(got, BR.reference(case, "bias", "features"), P)
    for layout in ("nchw", "nhwc"):
        got = net.gradients(pb, grad_canvas=canvas_gradient(dc, layout), grad_features=gf, layout=layout, need_voxels=True, out=sentinels(net, pb))
        check(got, BR.reference(case, "bias", "both"), P)
    out = sentinels(net, pb)
    got = net.gradients(pb, grad_canvas=canvas_gradient(dc, "nchw"), out=out)
    assert got[3] is None and bool((out[3] == SENTINEL).all())
    check(got, BR.reference(case), P)
    fresh = net.gradients(pb, grad_canvas=canvas_gradient(dc, "nchw"), need_voxels=True)  # buffers of its own
    assert fresh[0].data_ptr() != out[0].data_ptr()
    check(fresh, BR.reference(case), P)


def test_rows_outside_the_canvas_get_no_canvas_gradient():
    a = dict(C.build("fullrow-o32"))
    coords = a["coords"].copy()
    coords[6, 3] = 7                                         # ix = nx
    coords[7, 2] = -1                                        # iy = -1
    a["coords"] = coords
    dc, df = BR.upstream_canvas("fullrow-o32")
    pb, net = batch(a), layer(a)
    gf = feature_gradient(df, pb.voxels.shape[0])
    for layout in ("nchw", "nhwc"):
        for kw, tkw in ((dict(d_canvas=dc), dict()), (dict(d_canvas=dc, d_features=df), dict(grad_features=gf))):
            want = BR.gradients(a["voxels"], coords, a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"], **kw)
            got = net.gradients(pb, grad_canvas=canvas_gradient(dc, layout), layout=layout, need_voxels=True, out=sentinels(net, pb), **tkw)
            check(got, want, len(coords))
    assert (want["g"][[6, 7]] == df[[6, 7]]).all()


def test_two_calls_give_the_same_bytes():
    case = C.REAL_CASE
    a = C.build(case)
    dc, df = BR.upstream_canvas(case)
    pb, net = batch(a), layer(a)
    g, gf = canvas_gradient(dc, "nchw"), feature_gradient(df, pb.voxels.shape[0])
    first = net.gradients(pb, grad_canvas=g, grad_features=gf, need_voxels=True)
    second = net.gradients(pb, grad_canvas=g, grad_features=gf, need_voxels=True)
    for x, y in zip(first, second):
        assert x.data_ptr() != y.data_ptr() and torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_capture_and_replay_on_new_contents():
    """gradients(out=...) captured and replayed after the pillars, their count, the layer and the upstream gradient changed in place"""
    a, b = C.build("pair-N5-c9-o64"), C.build("mixed-N5-c9-o64")
    assert len(b["coords"]) < len(a["coords"]) and a["voxels"].shape[1:] == b["voxels"].shape[1:] and (a["nx"], a["ny"]) == (b["nx"], b["ny"])
    pb, net = batch(a), layer(a)
    dca, _ = BR.upstream_canvas("pair-N5-c9-o64")
    g = canvas_gradient(dca, "nchw")
    out = sentinels(net, pb)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net.gradients(pb, grad_canvas=g, need_voxels=True, out=out)
    torch.cuda.current_stream().wait_stream(s)
    check(tuple(out), BR.reference("pair-N5-c9-o64"), len(a["coords"]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.gradients(pb, grad_canvas=g, need_voxels=True, out=out)
    rng = np.random.RandomState(8)
    for source, flip in ((b, False), (a, True)):
        P = len(source["coords"])
        w = (source["weight"] * F(-1.0)).astype(F) if flip else source["weight"]
        up = rng.standard_normal(dca.shape).astype(F)
        pb.voxels.fill_(SENTINEL); pb.coords.fill_(1 << 20); pb.num_points.fill_(1 << 20)
        pb.voxels[:P].copy_(torch.from_numpy(source["voxels"].copy())); pb.coords[:P].copy_(torch.from_numpy(source["coords"].copy()))
        pb.num_points[:P].copy_(torch.from_numpy(source["num_points"].copy())); pb.offsets.copy_(torch.from_numpy(source["offsets"].copy()))
        net.weight.copy_(torch.from_numpy(w.copy())); net.bias.copy_(torch.from_numpy(source["bias"].copy()))
        g.copy_(torch.from_numpy(up))
        for t in out:
            t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = BR.gradients(source["voxels"], source["coords"], source["num_points"], source["offsets"], source["nx"], source["ny"], w,
                            source["bias"], d_canvas=up)
        check(tuple(out), want, P)
    assert not np.array_equal(want["d_weight"], BR.reference("pair-N5-c9-o64")["d_weight"])


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_autograd_gives_what_the_raw_call_gives(layout, tied):
    from mcav import lib as L
    from pseudo_lidar import PillarFeatureNet
    case = "mixed-N5-c9-o64"
    a = C.build(case)
    dc, df = BR.upstream_canvas(case)
    pb = batch(a)
    P = len(a["coords"])
    w, b = tensor(a["weight"]).requires_grad_(True), tensor(a["bias"]).requires_grad_(True)
    bp = None if tied else (tensor(a["bias"]) * 0.5).requires_grad_(True)
    net = PillarFeatureNet(w, b, bp)
    assert (net.bias_pad is net.bias) == tied
    want_canvas = R.pseudo_image(a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"],
                                 bias_pad=None if tied else (a["bias"] * F(0.5)).astype(F))
    with torch.no_grad():                                                                  # today's path, today's bytes
        plain = net.pseudo_image(pb, layout=layout)
    assert not plain.requires_grad and plain.grad_fn is None
    C.same_bits(plain.cpu().contiguous().numpy(), want_canvas["canvas"])
    pb.voxels.requires_grad_(True)
    g, gf = canvas_gradient(dc, layout), feature_gradient(df, pb.voxels.shape[0])
    raw = net.gradients(pb, grad_canvas=g, layout=layout, need_voxels=True)
    raw_f = net.gradients(pb, grad_features=gf, need_voxels=True)
    for forward, upstream, ref in ((lambda: net.pseudo_image(pb, layout=layout), g, raw), (lambda: net.features(pb), gf, raw_f)):
        for t in (w, b, bp, pb.voxels):
            if t is not None:
                t.grad = None
        out = forward()
        assert out.requires_grad and out.grad_fn is not None
        if upstream is g:
            C.same_bits(out.detach().cpu().contiguous().numpy(), want_canvas["canvas"])
            assert out.is_contiguous(memory_format=torch.channels_last if layout == "nhwc" else torch.contiguous_format)
        out.backward(upstream)
        same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert same(w.grad, ref[0]) and same(pb.voxels.grad, ref[3])
        if tied:
            assert same(b.grad, ref[1] + ref[2])
        else:
            assert same(b.grad, ref[1]) and same(bp.grad, ref[2])
    check(raw, BR.gradients(a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"],
                            None if tied else (a["bias"] * F(0.5)).astype(F), d_canvas=dc), P)
    with pytest.raises(L.MCAVError, match="gradient"):
        net.pseudo_image(pb, layout=layout, out=plain)
    with pytest.raises(L.MCAVError, match="gradient"):
        net.pseudo_image(pb, layout=layout, features=torch.empty((pb.voxels.shape[0], 64), device=DEV))
    with pytest.raises(L.MCAVError, match="gradient"):
        net.features(pb, out=torch.empty((pb.voxels.shape[0], 64), device=DEV))
    pb.voxels.requires_grad_(False)
    w.requires_grad_(False); b.requires_grad_(False)
    if bp is not None:
        bp.requires_grad_(False)
    assert net.pseudo_image(pb, layout=layout, out=plain) is plain                         # nothing requires a gradient: out= is taken again


def test_only_the_voxels_require_a_gradient():
    """the first link of the chain to the depth network: a frozen layer, d_voxels alone"""
    case = "pair-N5-c9-o64"
    a, want = C.build(case), BR.reference(case)
    dc, _ = BR.upstream_canvas(case)
    pb, net = batch(a), layer(a)
    pb.voxels.requires_grad_(True)
    net.pseudo_image(pb).backward(canvas_gradient(dc, "nchw"))
    P = len(a["coords"])
    C.same_bits(pb.voxels.grad[:P].cpu().numpy(), want["d_voxels"])
    assert net.weight.grad is None and bool((pb.voxels.grad[P:] == 0).all())


def test_layer_trains_and_eval_net_is_its_forward():
    """PillarFeatureLayer on mixed-N5-c9-o64, thirty Adam steps towards the fixed canvas of another randomly drawn layer: the loss ends
    below half its start; for 9 columns the forward is from_state_dict's, bit for bit, before and after"""
    from pseudo_lidar import PillarFeatureLayer, PillarFeatureNet
    a = C.build("mixed-N5-c9-o64")
    pb = batch(a)
    torch.manual_seed(21)
    teacher = PillarFeatureLayer(9, 64).to(DEV)
    with torch.no_grad():
        teacher.linear.weight.normal_(0.0, 0.4); teacher.norm.weight.normal_().abs_().add_(0.5); teacher.norm.bias.normal_(0.0, 0.3)
        teacher.norm.running_mean.normal_(0.0, 0.2); teacher.norm.running_var.uniform_(0.1, 1.1)
        target = teacher(pb)
    assert not target.requires_grad and float(target.abs().sum()) > 0
    torch.manual_seed(22)
    student = PillarFeatureLayer(9, 64).to(DEV)
    student.train()
    opt = torch.optim.Adam(student.parameters(), lr=0.03)
    P = len(a["coords"])
    losses = []
    for step in range(31):
        out = student(pb)
        loss = ((out - target) ** 2).sum() / (P * 64)
        losses.append(loss.detach())
        if step < 30:
            opt.zero_grad()
            loss.backward()
            opt.step()
    losses = [float(v) for v in losses]
    print("loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], losses
    assert int(student.norm.num_batches_tracked) == 0 and bool((student.norm.running_var == 1).all())      # frozen statistics
    for layout in ("nchw", "nhwc"):
        with torch.no_grad():
            want = student(pb, layout=layout)
        got = student.eval_net().pseudo_image(pb, layout=layout)
        loaded = PillarFeatureNet.from_state_dict(student.state_dict(), prefix="").pseudo_image(pb, layout=layout)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(loaded.view(torch.int32), want.view(torch.int32))
    assert float((want - target).abs().max()) > 0


def test_layer_with_ten_columns_matches_from_state_dict():
    from pseudo_lidar import PillarFeatureLayer, PillarFeatureNet, PillarGrid
    a = C.build("pair-N5-c9-o64")
    pb = batch(a)
    pb.grid = PillarGrid(x=(0.0, float(a["nx"])), y=(0.0, float(a["ny"])), z=(-3.0, 1.0), size=(1.0, 1.0))      # zc = -1
    torch.manual_seed(5)
    m = PillarFeatureLayer(10, 64, grid=pb.grid).to(DEV)
    with torch.no_grad():
        m.norm.running_mean.normal_(0.0, 0.2); m.norm.running_var.uniform_(0.1, 1.1); m.norm.bias.normal_(0.0, 0.3)
    out = m(pb)
    loaded = PillarFeatureNet.from_state_dict(m.state_dict(), prefix="", grid=pb.grid)
    assert loaded.bias_pad is not loaded.bias
    assert torch.equal(out.detach().view(torch.int32), loaded.pseudo_image(pb).view(torch.int32))
    out.sum().backward()
    assert m.linear.weight.grad.shape == (64, 10) and bool(m.linear.weight.grad[:, 9].abs().sum() > 0) and m.norm.bias.grad is not None


def test_c_abi_refuses_bad_arguments_untouched():
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401  (registers the signatures)
    h = L.lib()
    case = "mixed-N5-c9-o64"
    a = C.build(case)
    dc, df = BR.upstream_canvas(case)
    pb, net = batch(a), layer(a)
    cap = pb.voxels.shape[0]
    g, gf = canvas_gradient(dc, "nchw"), feature_gradient(df, cap)
    out = sentinels(net, pb)
    nbytes = h.mcav_pillar_pseudo_image_bwd_workspace_bytes(cap, 9, 64)
    assert nbytes >= 8 * 64 * 11 and nbytes % 256 == 0
    for bad in ((-1, 9, 64), (cap, 5, 64), (cap, 10, 64), (cap, 9, 48), (cap, 9, 0), (cap, 9, 160)):
        assert h.mcav_pillar_pseudo_image_bwd_workspace_bytes(*bad) == 0, bad
    ws = torch.full((nbytes + 8,), 0x55, dtype=torch.uint8, device=DEV)
    good = dict(voxels=L.ptr(pb.voxels), coords=L.ptr(pb.coords), num=L.ptr(pb.num_points), poff=L.ptr(pb.offsets), B=len(pb), cap=cap, N=5,
                C=9, nx=a["nx"], ny=a["ny"], w=L.ptr(net.weight), b=L.ptr(net.bias), bp=L.ptr(net.bias_pad), c_out=64, flags=0, dc=L.ptr(g),
                df=L.ptr(gf), dw=L.ptr(out[0]), db=L.ptr(out[1]), dbp=L.ptr(out[2]), dv=L.ptr(out[3]), ws=L.ptr(ws), bytes=nbytes)
    call = lambda **kw: h.mcav_pillar_pseudo_image_bwd(*[dict(good, **kw)[k] for k in good], L.stream())
    bad = [dict(voxels=L.c_p(0)), dict(coords=L.c_p(0)), dict(num=L.c_p(0)), dict(poff=L.c_p(0)), dict(w=L.c_p(0)), dict(b=L.c_p(0)),
           dict(bp=L.c_p(0)), dict(dc=L.c_p(0), df=L.c_p(0)), dict(dw=L.c_p(0)), dict(db=L.c_p(0)), dict(dbp=L.c_p(0)), dict(ws=L.c_p(0)),
           dict(B=0), dict(B=-1), dict(B=65536), dict(cap=-1), dict(N=0), dict(N=65), dict(C=0), dict(C=5), dict(C=10), dict(c_out=0),
           dict(c_out=16), dict(c_out=48), dict(c_out=160), dict(c_out=-64), dict(flags=2), dict(flags=1 << 30), dict(nx=0), dict(ny=0),
           dict(nx=-7), dict(nx=1 << 16, ny=1 << 14), dict(B=4, nx=1 << 15, ny=1 << 14), dict(dc=L.c_p(g.data_ptr() + 2)),
           dict(dv=L.c_p(out[3].data_ptr() + 1)), dict(ws=L.c_p(ws.data_ptr() + 4))]
    for kw in bad:
        assert call(**kw) == -1, kw
    for short in (0, nbytes - 1):
        assert call(bytes=short) == -2, short
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in out) and bool((ws == 0x55).all())
    assert call() == 0
    check(tuple(out), BR.reference(case, "bias", "both"), len(a["coords"]))
    assert call(dv=L.c_p(0), df=L.c_p(0)) == 0 and call(dc=L.c_p(0)) == 0                  # each optional pointer on its own
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_canvas=g.contiguous(memory_format=torch.channels_last))     # nchw asked for, channels_last given
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_canvas=g, layout="nhwc")
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_canvas=g[:, :32])
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_canvas=g.double())
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_features=gf[:-1])
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_canvas=g, out=out[:2])
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_canvas=g, need_voxels=True, out=out[:3])
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_canvas=g, out=[out[0], out[1], out[2].double()])
    with pytest.raises(L.MCAVError):
        net.gradients(pb, grad_canvas=g.cpu())
