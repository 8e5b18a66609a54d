"""GPU: the pillar feature net and its pseudo-image (include/mcav_depth.h: mcav_pillar_pseudo_image, pseudo_lidar.PillarFeatureNet,
PillarBatch.pseudo_image) against its restatement (tests/pfn_ref.py), bit for bit (NaNs by class), on the cases of tests/pfn_cases.py in
both layouts; sentinels in the canvas, which must be written everywhere, and in the feature rows that must stay unwritten; a capacity
below the count; the padding variants; repeatability; graph capture and replay on new contents; the path behind pillarize; the C ABI's
refusals."""
import numpy as np
import pytest
import torch

import pfn_cases as C
import pfn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -7.0
SLACK = 5                                                    # rows of the buffers behind the pillars: they keep the sentinel


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


def layer(a, pad="bias"):
    from pseudo_lidar import PillarFeatureNet
    t = lambda v: torch.from_numpy(np.array(v, F)).to(DEV)
    return PillarFeatureNet(t(a["weight"]), t(a["bias"]), None if pad == "bias" else t(C.bias_pad(a, pad)))


def sentinels(a, pb, layout):
    shape = (len(pb), a["weight"].shape[0], a["ny"], a["nx"])
    canvas = torch.empty(shape, device=DEV, memory_format=torch.channels_last if layout == "nhwc" else torch.contiguous_format).fill_(SENTINEL)
    return canvas, torch.full((pb.voxels.shape[0], shape[1]), SENTINEL, device=DEV)


def check(canvas, feat, want, layout):
    """the canvas everywhere, the feature rows below the pillar count, the sentinel in the rows behind them"""
    assert canvas.dtype == torch.float32 and canvas.shape == want["canvas"].shape
    assert canvas.is_contiguous(memory_format=torch.channels_last if layout == "nhwc" else torch.contiguous_format)
    C.same_bits(canvas.cpu().contiguous().numpy(), want["canvas"])
    if feat is not None:
        P = len(want["features"])
        host = feat.cpu().numpy()
        C.same_bits(host[:P], want["features"])
        assert len(host) > P and (host[P:] == SENTINEL).all()


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("case", C.CASES)
def test_kernel_matches_restatement(case, layout):
    C.check_non_trivial(case)
    a = C.build(case)
    pb, net = batch(a), layer(a)
    canvas, feat = sentinels(a, pb, layout)
    got = net.pseudo_image(pb, layout=layout, out=canvas, features=feat)
    assert got is canvas
    check(canvas, feat, C.reference(case), layout)


def test_real_grid():
    """B = 2 on the 432 x 496 grid: four column tiles a row, the last of 48 columns; 16-byte stores; 110 MB written"""
    C.check_non_trivial(C.REAL_CASE)
    a = C.build(C.REAL_CASE)
    pb, net = batch(a), layer(a)
    want = C.reference(C.REAL_CASE)
    for layout in ("nchw", "nhwc"):
        canvas, feat = sentinels(a, pb, layout)
        pb.pseudo_image(net, layout=layout, out=canvas, features=feat)                     # the PillarBatch shortcut
        check(canvas, feat, want, layout)


def test_unaligned_canvas_takes_the_narrow_stores():
    """a canvas that starts 4 bytes into its allocation: dword stores, the same values, nothing in front of it or behind it touched"""
    case = "wide-o128"
    a = C.build(case)
    pb, net = batch(a), layer(a)
    shape = C.reference(case)["canvas"].shape
    n = int(np.prod(shape))
    for layout in ("nchw", "nhwc"):
        raw = torch.full((n + 8,), SENTINEL, device=DEV)
        view = raw[1:n + 1].view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2) if layout == "nhwc" else raw[1:n + 1].view(shape)
        assert view.data_ptr() % 16 == 4
        net.pseudo_image(pb, layout=layout, out=view)
        C.same_bits(view.cpu().contiguous().numpy(), C.reference(case)["canvas"])
        assert float(raw[0]) == SENTINEL and bool((raw[n + 1:] == SENTINEL).all())


@pytest.mark.parametrize("case", ["pair-N5-c9-o64", "wide-o128"])
def test_capacity_ends_inside_the_second_image(case):
    """the pillars behind the capacity are never read: their cells are +0.0, their feature rows do not exist"""
    a = C.build(case)
    cap = C.cut_capacity(case)
    want = C.reference(case, "bias", cap)
    dropped = a["coords"][cap:]
    assert len(dropped) and (want["canvas"][dropped[:, 0], :, dropped[:, 2], dropped[:, 3]].view(np.uint32) == 0).all()
    pb, net = batch(a, capacity=cap), layer(a)
    for layout in ("nchw", "nhwc"):
        canvas, _ = sentinels(a, pb, layout)
        feat = torch.full((cap, net.c_out), SENTINEL, device=DEV)
        net.pseudo_image(pb, layout=layout, out=canvas, features=feat)
        check(canvas, None, want, layout)
        C.same_bits(feat.cpu().numpy(), want["features"])


def test_without_features_and_features_alone():
    case = "mixed-N32-c9-o128"
    a, want = C.build(case), C.reference(case)
    pb, net = batch(a), layer(a)
    canvas, feat = sentinels(a, pb, "nchw")
    net.pseudo_image(pb, out=canvas)
    check(canvas, None, want, "nchw")
    assert net.features(pb, out=feat) is feat
    check(canvas, feat, want, "nchw")
    fresh = net.features(pb)
    assert fresh.shape == feat.shape and fresh.data_ptr() != feat.data_ptr()
    C.same_bits(fresh[:len(want["features"])].cpu().numpy(), want["features"])
    made = net.pseudo_image(pb, layout="nhwc")                                             # a canvas of its own
    check(made, None, want, "nhwc")


@pytest.mark.parametrize("pad", ["zero", "negative", "other"])
def test_bias_pad_variants(pad):
    from pseudo_lidar import PillarFeatureNet
    case = "pair-N5-c9-o64"
    a = C.build(case)
    value = {"zero": np.zeros_like(a["bias"]), "negative": np.full_like(a["bias"], -2.5), "other": (a["bias"] * F(-1.5)).astype(F)}[pad]
    want = R.pseudo_image(a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"], bias_pad=value)
    if pad != "other":
        C.same_bits(want["canvas"], C.reference(case, "zero")["canvas"])                   # any bias_pad <= 0 ignores the padding
    assert not np.array_equal(want["canvas"], C.reference(case)["canvas"])
    t = lambda v: torch.from_numpy(np.array(v, F)).to(DEV)
    net = PillarFeatureNet(t(a["weight"]), t(a["bias"]), t(value))
    pb = batch(a)
    canvas, feat = sentinels(a, pb, "nchw")
    net.pseudo_image(pb, out=canvas, features=feat)
    check(canvas, feat, want, "nchw")


def test_two_calls_give_the_same_bytes():
    case = "wide-o128"
    a = C.build(case)
    pb, net = batch(a), layer(a)
    first, second = net.pseudo_image(pb), net.pseudo_image(pb)
    assert first.data_ptr() != second.data_ptr()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))                  # the NaNs' bits too
    f1, f2 = net.features(pb), net.features(pb)
    P = len(a["coords"])
    assert torch.equal(f1[:P].view(torch.int32), f2[:P].view(torch.int32))


def test_capture_and_replay_on_new_contents():
    """pseudo_image(out=, features=) captured on one stream and replayed twice after the pillars, their count and the layer changed in
    place: every replay writes the whole canvas again"""
    a, b = C.build("pair-N5-c9-o64"), C.build("mixed-N5-c9-o64")
    Pa, Pb = len(a["coords"]), len(b["coords"])
    assert Pb < Pa and a["voxels"].shape[1:] == b["voxels"].shape[1:] and (a["nx"], a["ny"]) == (b["nx"], b["ny"])
    pb, net = batch(a), layer(a)
    canvas, feat = sentinels(a, pb, "nchw")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net.pseudo_image(pb, out=canvas, features=feat)
    torch.cuda.current_stream().wait_stream(s)
    check(canvas, feat, C.reference("pair-N5-c9-o64"), "nchw")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        net.pseudo_image(pb, out=canvas, features=feat)
    for source, flip in ((b, False), (a, True)):
        P = len(source["coords"])
        w = (source["weight"] * F(-1.0)).astype(F) if flip else source["weight"]
        pb.voxels.fill_(SENTINEL); pb.coords.fill_(1 << 20); pb.num_points.fill_(1 << 20)
        pb.voxels[:P].copy_(torch.from_numpy(source["voxels"].copy())); pb.coords[:P].copy_(torch.from_numpy(source["coords"].copy()))
        pb.num_points[:P].copy_(torch.from_numpy(source["num_points"].copy())); pb.offsets.copy_(torch.from_numpy(source["offsets"].copy()))
        net.weight.copy_(torch.from_numpy(w)); net.bias.copy_(torch.from_numpy(source["bias"].copy()))
        canvas.fill_(SENTINEL); feat.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        want = R.pseudo_image(source["voxels"], source["coords"], source["num_points"], source["offsets"], source["nx"], source["ny"], w,
                              source["bias"])
        check(canvas, feat, want, "nchw")
    assert not np.array_equal(want["canvas"], C.reference("pair-N5-c9-o64")["canvas"])


def test_rows_outside_the_canvas_are_skipped():
    """rows whose (b, iy, ix) name no cell, sorted where they belong: no cell, no feature row, nothing else disturbed"""
    a = dict(C.build("fullrow-o32"))
    coords = a["coords"].copy()
    coords[6, 3] = 7                                         # ix = nx
    coords[7, 2] = -1                                        # iy = -1
    a["coords"] = coords
    want = R.pseudo_image(a["voxels"], coords, a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"])
    pb, net = batch(a), layer(a)
    for layout in ("nchw", "nhwc"):
        canvas, feat = sentinels(a, pb, layout)
        net.pseudo_image(pb, layout=layout, out=canvas, features=feat)
        C.same_bits(canvas.cpu().contiguous().numpy(), want["canvas"])
        host = feat.cpu().numpy()
        keep = np.ones(len(coords), bool)
        keep[[6, 7]] = False
        C.same_bits(host[:len(coords)][keep], want["features"][keep])
        assert (host[[6, 7]] == SENTINEL).all() and (host[len(coords):] == SENTINEL).all()
    C.same_bits(net.features(pb)[:len(coords)].cpu().numpy(), want["features"])            # features alone: every row, whatever its coords


def test_end_to_end_behind_pillarize():
    """pseudo_lidar.pillarize on the device, then the layer: the pseudo-image of the restatement's pillars of the same cloud"""
    import pillar_cases as PC
    import pillar_ref as PR
    from pseudo_lidar import PillarGrid, pillarize
    case = "pair-N5-c9"
    p, pillars = PC.build(case), PC.reference(case)
    g = p["grid"]
    grid = PillarGrid(x=(float(g.x0), float(g.x0) + float(g.vx) * g.nx), y=(float(g.y0), float(g.y0) + float(g.vy) * g.ny),
                      z=(float(g.z0), float(g.z1)), size=(float(g.vx), float(g.vy)))
    pb = pillarize(torch.from_numpy(np.ascontiguousarray(p["points"])).to(DEV), torch.from_numpy(np.ascontiguousarray(p["offsets"])).to(DEV),
                   grid=grid, max_points=p["max_points"], decorate=p["decorate"])
    a = C.build(case + "-o64")
    assert a["voxels"] is not None and np.array_equal(a["coords"], pillars["coords"])
    net = layer(a)
    canvas = pb.pseudo_image(net)
    feat = net.features(pb)
    want = C.reference(case + "-o64")
    assert pb.voxels.shape[0] > len(want["features"])
    C.same_bits(canvas.cpu().numpy(), want["canvas"])
    C.same_bits(feat[:len(want["features"])].cpu().numpy(), want["features"])
    assert PR.make_grid().nx == 432


def test_c_abi_refuses_bad_arguments_untouched():
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401  (registers the signatures)
    h = L.lib()
    case = "mixed-N5-c9-o64"
    a = C.build(case)
    pb, net = batch(a), layer(a)
    canvas, feat = sentinels(a, pb, "nchw")
    good = dict(voxels=L.ptr(pb.voxels), coords=L.ptr(pb.coords), num=L.ptr(pb.num_points), poff=L.ptr(pb.offsets), B=len(pb),
                cap=pb.voxels.shape[0], N=5, C=9, nx=a["nx"], ny=a["ny"], w=L.ptr(net.weight), b=L.ptr(net.bias), bp=L.ptr(net.bias_pad),
                c_out=64, flags=0, canvas=L.ptr(canvas), feat=L.ptr(feat))
    call = lambda **kw: h.mcav_pillar_pseudo_image(*[dict(good, **kw)[k] for k in good], L.stream())
    bad = [dict(voxels=L.c_p(0)), dict(coords=L.c_p(0)), dict(num=L.c_p(0)), dict(poff=L.c_p(0)), dict(w=L.c_p(0)), dict(b=L.c_p(0)),
           dict(bp=L.c_p(0)), dict(canvas=L.c_p(0), feat=L.c_p(0)), dict(B=0), dict(B=-1), dict(B=65536), dict(cap=-1), dict(N=0), dict(N=65),
           dict(C=0), dict(C=5), dict(C=10), dict(c_out=0), dict(c_out=16), dict(c_out=48), dict(c_out=160), dict(c_out=-64), dict(flags=2),
           dict(flags=1 << 30), dict(nx=0), dict(ny=0), dict(nx=-7), dict(nx=1 << 16, ny=1 << 14), dict(B=4, nx=1 << 15, ny=1 << 14),
           dict(canvas=L.c_p(canvas.data_ptr() + 2)), dict(voxels=L.c_p(pb.voxels.data_ptr() + 1))]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((canvas == SENTINEL).all()) and bool((feat == SENTINEL).all())
    assert call() == 0
    check(canvas, feat, C.reference(case), "nchw")
    with pytest.raises(L.MCAVError):
        net.pseudo_image(pb, out=canvas.contiguous(memory_format=torch.channels_last))     # nchw asked for, a channels_last canvas given
    with pytest.raises(L.MCAVError):
        net.pseudo_image(pb, layout="nhwc", out=canvas)
    with pytest.raises(L.MCAVError):
        net.pseudo_image(pb, out=canvas[:, :32])
    with pytest.raises(L.MCAVError):
        net.pseudo_image(pb, out=canvas.double())
    with pytest.raises(L.MCAVError):
        net.pseudo_image(pb, features=feat[:-1])
    with pytest.raises(L.MCAVError):
        net.pseudo_image(pb, out=canvas.cpu())
