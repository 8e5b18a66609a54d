"""CPU: the pillar feature net's backward (include/mcav_depth.h: mcav_pillar_pseudo_image_bwd, pseudo_lidar.PillarFeatureNet.gradients,
PillarFeatureLayer).  The restatement (tests/pfn_bwd_ref.py) against float64 autograd through the stock formulation outside near-ties;
the header csrc/pfn_bwd_math.h compiled for the host against the restatement -- winners and d_voxels bit for bit, the sums within one
float32 rounding -- on the cases the GPU tests run (tests/pfn_cases.py), once more as a stand-alone program under the address and
undefined-behaviour sanitizers; what the Python side refuses without a GPU; PillarFeatureLayer's state dict and fold."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import pfn_bwd_ref as BR
import pfn_cases as C
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "pfn_bwd_hostcheck", "pfn_bwd_hostcheck.cpp")
F = np.float32
ALL = C.CASES + [C.REAL_CASE]
PADS = ["bias", "zero"]
CAP = 0.05                                                   # of a case's live (p, o) may be near-ties


# ---------------------------------------------------------------------------------------------- restatement vs float64 autograd
def finite_copy(a):
    """the case with the pillars that hold a NaN or an infinity emptied (float64 autograd turns 0 x inf into NaNs all over the sums;
    what the definition does with such pillars is held by the host check and the direct test below): no points, so only the padding
    term competes there, and no upstream gradient on either side -> case, finite [P]"""
    finite = np.isfinite(a["voxels"]).all(axis=(1, 2))
    b = dict(a)
    b["voxels"] = np.where(finite[:, None, None], a["voxels"], F(0))
    b["num_points"] = np.where(finite, a["num_points"], 0).astype(np.int32)
    return b, finite


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("case", ALL)
def test_restatement_matches_float64_autograd(case, pad):
    """Outside the near-ties (a (p, o) whose two best competitors lie within 1e-5 relative in float64; at most 5 % of a case's live
    (p, o)): the same winners; d_voxels within C_out 2^-24 sum_o |g w|; the three sums within 2^-24 |ref| + 2^-32 sum |terms|.  The
    upstream gradient of the near-ties is zero on both sides, so every output is compared whole."""
    a, finite = finite_copy(C.build(case))
    bp = C.bias_pad(a, pad)
    dc, _ = BR.upstream_canvas(case)
    probe = BR.torch_autograd(a, bp, dc)
    near = probe["near"]
    live = near.size
    print("%s %s: %d of %d (p, o) are near-ties: %.2f %%" % (case, pad, near.sum(), live, 100.0 * near.sum() / live))
    assert near.sum() <= CAP * live, "%d of %d (p, o) are near-ties: %.2f %%" % (near.sum(), live, 100.0 * near.sum() / live)
    keep = ~near & finite[:, None]
    want = BR.torch_autograd(a, bp, dc, keep=keep.astype(np.float64))
    mask = np.zeros(dc.shape, F)
    mask[a["coords"][:, 0], :, a["coords"][:, 2], a["coords"][:, 3]] = keep
    got = BR.gradients(a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"], bp, d_canvas=dc * mask)
    assert np.array_equal(got["slot"][keep], want["slot"][keep])
    assert (got["slot"][keep] >= 0).sum() >= 4
    # d_voxels: a chain of at most C_out fmas, each within 2^-24 of the running magnitude
    w64, g64 = a["weight"].astype(np.float64), got["g"].astype(np.float64)
    N = a["voxels"].shape[1]
    mag = np.zeros(a["voxels"].shape)
    for k in range(N):
        mag[:, k, :] = (np.abs(g64) * (got["slot"] == k)) @ np.abs(w64)
    err = np.abs(got["d_voxels"].astype(np.float64) - want["d_voxels"])
    assert (err <= w64.shape[0] * 2.0 ** -24 * mag).all(), (err - w64.shape[0] * 2.0 ** -24 * mag).max()
    assert (got["d_voxels"][mag == 0].view(np.uint32) == 0).all()                          # +0.0 where nothing won
    for k, t in (("d_weight", "abs_weight"), ("d_bias", "abs_bias"), ("d_bias_pad", "abs_bias_pad")):
        err = np.abs(got[k].astype(np.float64) - want[k])
        assert (err <= BR.sum_bound(want[k], got[t])).all(), (k, (err - BR.sum_bound(want[k], got[t])).max())
    if pad == "zero":
        assert (got["slot"] != BR.PADDING).all() and (got["d_bias_pad"] == 0).all()
    elif (a["num_points"] < N).any():
        won = (got["slot"][:, 2] == BR.PADDING) & keep[:, 2]                              # channel 2: the padding wins partly filled pillars
        assert won.any() or case == "special-o32"                                          # (whose partly filled pillars hold the NaNs)
        assert (got["d_bias_pad"][2] != 0) == won.any()
    assert (got["slot"][:, 1] == BR.NO_FLOW).all() and got["d_bias"][1] == 0 and (got["d_weight"][1] == 0).all()      # channel 1: +0.0


def test_definition_on_special_values_and_ties():
    """a NaN feature gets no gradient, +inf does; the lowest of equal slots wins; a slot that ties the padding takes it; feat = 0 gets
    nothing; rows outside the canvas get no canvas gradient; d_features is added in float32"""
    ref = BR.reference("special-o32")
    feat, slot = ref["features"], ref["slot"]
    assert np.isnan(feat).any() and (slot[np.isnan(feat)] == BR.NO_FLOW).all()
    assert (slot[feat == np.inf] >= 0).all() and (feat == np.inf).any()
    assert (slot[feat == 0] == BR.NO_FLOW).all() and ((feat > 0) == (slot != BR.NO_FLOW)).all()
    w = np.zeros((32, 4), F)
    w[:, 0] = 1.0
    vox = np.zeros((2, 3, 4), F)
    vox[0, :, 0] = [2.0, 2.0, 1.0]                           # slots 0 and 1 tie: 0 wins
    vox[1, :2, 0] = [0.25, 0.5]                              # n = 2 of 3: the padding (0.5) ties slot 1: the slot wins
    coords = np.array([[0, 0, 0, 0], [0, 0, 5, 0]], np.int32)                              # the second row lies outside a 2 x 2 canvas
    num, off = np.array([3, 2], np.int32), np.array([0, 2], np.int32)
    dc = np.full((1, 32, 2, 2), 3.0, F)
    df = np.full((2, 32), 0.5, F)
    out = BR.gradients(vox, coords, num, off, 2, 2, w, np.zeros(32, F), np.full(32, 0.5, F), d_canvas=dc, d_features=df)
    assert (out["slot"][0] == 0).all() and (out["slot"][1] == 1).all()
    assert (out["g"][0] == 3.5).all() and (out["g"][1] == 0.5).all()
    assert (out["d_bias"] == 4.0).all() and (out["d_bias_pad"] == 0).all() and (out["d_weight"][:, 0] == 3.5 * 2.0 + 0.5 * 0.5).all()
    assert out["d_voxels"][0, 0, 0] == 32 * 3.5 and (out["d_voxels"][0, 1:] == 0).all() and out["d_voxels"][1, 1, 0] == 16.0
    pad_wins = BR.gradients(vox, coords, num, off, 2, 2, w, np.zeros(32, F), np.full(32, 0.75, F), d_features=df)
    assert (pad_wins["slot"][1] == BR.PADDING).all() and (pad_wins["d_bias_pad"] == 0.5).all() and (pad_wins["d_voxels"][1] == 0).all()
    assert (pad_wins["slot"][0] == 0).all()                  # a full pillar has no padding term


# ---------------------------------------------------------------------------------------------- csrc/pfn_bwd_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pfn_bwd_hostcheck") / "libpfn_bwd_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.pfn_bwd_host.argtypes = [p, p, p, p, i, ll, i, i, i, i, p, p, p, i, i, p, p, p, p, p, p, p]
    return lib


def host_run(host, a, pad="bias", capacity=None, nhwc=False, d_canvas=None, d_features=None, want_voxels=True, **kw):
    """-> status, dict(d_weight, d_bias, d_bias_pad, d_voxels [capacity, N, C], slot [capacity, C_out]), all pre-filled with -7"""
    B, (cap, N, Cc), c_out = len(a["offsets"]) - 1, a["voxels"].shape, a["weight"].shape[0]
    cap = cap if capacity is None else capacity
    out = dict(d_weight=np.full((c_out, Cc), -7.0, F), d_bias=np.full(c_out, -7.0, F), d_bias_pad=np.full(c_out, -7.0, F),
               d_voxels=np.full((max(cap, 1), N, Cc), -7.0, F), slot=np.full((max(cap, 1), c_out), -7, np.int32))
    if d_canvas is not None and nhwc:
        d_canvas = np.ascontiguousarray(d_canvas.transpose(0, 2, 3, 1))
    arrays = dict(voxels=a["voxels"], coords=a["coords"], num_points=a["num_points"], offsets=a["offsets"], weight=a["weight"],
                  bias=a["bias"], bias_pad=C.bias_pad(a, pad), d_canvas=d_canvas, d_features=d_features)
    held = {k: np.ascontiguousarray(v) for k, v in arrays.items() if v is not None}
    arg = dict(B=B, capacity=cap, N=N, C=Cc, nx=a["nx"], ny=a["ny"], c_out=c_out, flags=1 if nhwc else 0, d_canvas=None, d_features=None,
               d_weight=out["d_weight"].ctypes.data, d_bias=out["d_bias"].ctypes.data, d_bias_pad=out["d_bias_pad"].ctypes.data,
               d_voxels=out["d_voxels"].ctypes.data if want_voxels else None, slot=out["slot"].ctypes.data)
    arg.update({k: v.ctypes.data for k, v in held.items()})
    arg.update(kw)
    rc = host.pfn_bwd_host(*[arg[k] for k in ("voxels", "coords", "num_points", "offsets", "B", "capacity", "N", "C", "nx", "ny", "weight", "bias",
                                              "bias_pad", "c_out", "flags", "d_canvas", "d_features", "d_weight", "d_bias", "d_bias_pad",
                                              "d_voxels", "slot")])
    return rc, out


def check_host(out, want, P):
    C.same_bits(out["d_voxels"], want["d_voxels"])
    assert np.array_equal(out["slot"][:P], want["slot"]) and (out["slot"][P:] == -7).all()
    BR.check_sums(out, want)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("case", ALL)
def test_header_matches_restatement(host, case, pad):
    a, want = C.build(case), BR.reference(case, pad)
    dc, _ = BR.upstream_canvas(case)
    P = len(want["slot"])
    for nhwc in ((False, True) if case != C.REAL_CASE else (False,)):
        rc, out = host_run(host, a, pad=pad, nhwc=nhwc, d_canvas=dc)
        assert rc == 0
        check_host(out, want, P)
    assert (want["slot"] >= 0).any() and (want["slot"] == BR.NO_FLOW).any()


def test_header_gradient_sources_capacity_and_optional_output(host):
    case = C.HARDEST
    a = C.build(case)
    dc, df = BR.upstream_canvas(case)
    P = len(a["coords"])
    for source, kw in (("features", dict(d_features=df)), ("both", dict(d_canvas=dc, d_features=df))):
        rc, out = host_run(host, a, **kw)
        assert rc == 0
        check_host(out, BR.reference(case, "bias", source), P)
    cap = C.cut_capacity(case)
    cut = BR.reference(case, "bias", "canvas", cap)
    rc, out = host_run(host, a, capacity=cap, d_canvas=dc)
    assert rc == 0 and len(cut["slot"]) == cap and cut["d_voxels"].shape[0] == cap
    check_host(out, cut, cap)
    assert not np.array_equal(cut["d_bias"], BR.reference(case)["d_bias"])
    rc, out = host_run(host, a, d_canvas=dc, want_voxels=False)
    assert rc == 0 and (out["d_voxels"] == -7).all()
    BR.check_sums(out, BR.reference(case))


def test_header_rows_outside_the_canvas_get_no_canvas_gradient(host):
    a = dict(C.build("fullrow-o32"))
    coords = a["coords"].copy()
    coords[6, 3] = 7                                         # ix = nx
    coords[7, 2] = -1                                        # iy = -1
    a["coords"] = coords
    dc, df = BR.upstream_canvas("fullrow-o32")
    for kw in (dict(d_canvas=dc), dict(d_canvas=dc, d_features=df)):
        want = BR.gradients(a["voxels"], coords, a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"], **kw)
        rc, out = host_run(host, a, **kw)
        assert rc == 0
        check_host(out, want, len(coords))
        if "d_features" not in kw:
            assert (want["g"][[6, 7]] == 0).all() and (want["d_voxels"][[6, 7]] == 0).all() and (want["g"][:6] != 0).all()


def test_header_refusals(host):
    a = C.build("mixed-N5-c9-o64")
    dc, df = BR.upstream_canvas("mixed-N5-c9-o64")
    assert host_run(host, a, d_canvas=dc)[0] == 0
    bad = [dict(voxels=None), dict(coords=None), dict(num_points=None), dict(offsets=None), dict(weight=None), dict(bias=None),
           dict(bias_pad=None), dict(d_canvas=None), dict(d_weight=None), dict(d_bias=None), dict(d_bias_pad=None), dict(B=0), dict(B=65536),
           dict(capacity=-1), dict(N=0), dict(N=65), dict(C=5), dict(C=10), dict(c_out=0), dict(c_out=48), dict(c_out=160), dict(flags=2),
           dict(nx=0), dict(ny=0), dict(nx=1 << 16, ny=1 << 14)]
    for kw in bad:
        rc, out = host_run(host, a, **dict(dict(d_canvas=dc), **kw))
        assert rc == -1 and all((v == -7).all() for v in out.values()), kw


def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the hardest case (NaN rows, partly filled
    pillars, 128 channels) at full capacity under the canvas gradient and with a capacity that ends inside the second image under both
    gradients, NHWC: a finding ends the program with a non-zero status."""
    exe = str(tmp_path / "pfn_bwd_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPFN_BWD_STANDALONE"]) +
                          ["-o", exe])
    a = C.build(C.HARDEST)
    dc, df = BR.upstream_canvas(C.HARDEST)
    B, (P, N, Cc), c_out = len(a["offsets"]) - 1, a["voxels"].shape, a["weight"].shape[0]
    for cap, nhwc, source in ((P, 0, "canvas"), (C.cut_capacity(C.HARDEST), 1, "both")):
        want = BR.reference(C.HARDEST, "bias", source, cap)
        head = np.array([B, cap, N, Cc, a["nx"], a["ny"], c_out, nhwc, 1, source == "both", 1, 0], np.int64)
        canvas = dc.transpose(0, 2, 3, 1) if nhwc else dc
        parts = [head, a["offsets"], a["num_points"][:cap], a["coords"][:cap], a["voxels"][:cap], a["weight"], a["bias"], a["bias"], canvas]
        parts += [df[:cap]] if source == "both" else []
        with open(str(tmp_path / "in.bin"), "wb") as f:
            for part in parts:
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        raw = open(str(tmp_path / "out.bin"), "rb").read()
        assert np.frombuffer(raw, np.int32, 1)[0] == 0
        at, out = 4, {}
        for k, shape, dt in (("d_weight", (c_out, Cc), F), ("d_bias", (c_out,), F), ("d_bias_pad", (c_out,), F), ("d_voxels", (cap, N, Cc), F),
                             ("slot", (cap, c_out), np.int32)):
            out[k] = np.frombuffer(raw, dt, int(np.prod(shape)), at).reshape(shape)
            at += out[k].nbytes
        assert at == len(raw)
        C.same_bits(out["d_voxels"], want["d_voxels"])
        assert np.array_equal(out["slot"], want["slot"])
        BR.check_sums(out, want)


# ---------------------------------------------------------------------------------------------- the Python side without a GPU
def cpu_layer(c_out=64, columns=9):
    from pseudo_lidar import PillarFeatureNet
    net = PillarFeatureNet.__new__(PillarFeatureNet)
    net.weight, net.bias, net.bias_pad = torch.zeros(c_out, columns), torch.zeros(c_out), torch.zeros(c_out)
    net.c_out, net.columns = c_out, columns
    return net


def test_python_side_refuses_without_a_gpu():
    import mcav.lib as L
    from pseudo_lidar import PillarBatch, PillarFeatureLayer, PillarGrid
    net = cpu_layer()
    pb = PillarBatch(2, 10, 5, 9, "cpu")
    pb.grid = PillarGrid()
    g = torch.zeros(2, 64, pb.grid.ny, pb.grid.nx)
    with pytest.raises(L.MCAVError, match="layout"):
        net.gradients(pb, grad_canvas=g, layout="chwn")
    with pytest.raises(L.MCAVError, match="grad_canvas or grad_features"):
        net.gradients(pb)
    with pytest.raises(L.MCAVError, match="PillarBatch"):
        net.gradients(pb.voxels, grad_canvas=g)
    with pytest.raises(L.MCAVError, match="GPU"):
        net.gradients(pb, grad_canvas=g)                                                   # CPU buffers
    four = PillarBatch(2, 10, 5, 4, "cpu")
    four.grid = PillarGrid()
    with pytest.raises(L.MCAVError, match="columns"):
        net.gradients(four, grad_features=torch.zeros(10, 64))
    pb.grid = None
    with pytest.raises(L.MCAVError, match="grid"):
        net.gradients(pb, grad_canvas=g)
    for kw in (dict(in_columns=8), dict(out_channels=48), dict(in_columns=10)):            # 10 columns without a grid
        with pytest.raises(L.MCAVError):
            PillarFeatureLayer(**kw)
    with pytest.raises(L.MCAVError, match="GPU"):
        PillarFeatureLayer()(pb)                                                           # a layer on the CPU has no path
    net.weight.requires_grad_(True)
    pb.grid = PillarGrid()
    with pytest.raises(L.MCAVError, match="GPU"):
        net.pseudo_image(pb)


# ---------------------------------------------------------------------------------------------- PillarFeatureLayer
PFN_KEYS = ["linear.weight", "norm.weight", "norm.bias", "norm.running_mean", "norm.running_var", "norm.num_batches_tracked"]


def randomise(layer, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.linear.weight.copy_(torch.randn(layer.linear.weight.shape, generator=g) * 0.4)
        layer.norm.weight.copy_(torch.randn(layer.out_channels, generator=g).abs() + 0.5)
        layer.norm.bias.copy_(torch.randn(layer.out_channels, generator=g) * 0.3)
        layer.norm.running_mean.copy_(torch.randn(layer.out_channels, generator=g) * 0.2)
        layer.norm.running_var.copy_(torch.rand(layer.out_channels, generator=g) + 0.1)


@pytest.mark.parametrize("columns", [4, 9, 10])
def test_layer_state_dict_and_fold(columns):
    """the keys are a PFNLayer's, a checkpoint round-trips, and the differentiable float64 fold gives fold_state_dict's bits"""
    from pseudo_lidar import PillarFeatureLayer, PillarFeatureNet, PillarGrid
    grid = PillarGrid(x=(-1.0, 2.5), y=(-1.0, 1.25), z=(-3.0, 1.0), size=(0.5, 0.25))
    layer = PillarFeatureLayer(columns, 64, grid=grid if columns == 10 else None)
    assert list(layer.state_dict().keys()) == PFN_KEYS
    assert isinstance(layer.linear, torch.nn.Linear) and layer.linear.bias is None and isinstance(layer.norm, torch.nn.BatchNorm1d)
    assert layer.norm.eps == 1e-3
    randomise(layer, columns)
    sd = {"vfe.pfn_layers.0." + k: v.clone() for k, v in layer.state_dict().items()}        # as a detector checkpoint names them
    other = PillarFeatureLayer(columns, 64, grid=grid if columns == 10 else None)
    other.load_state_dict({k[len("vfe.pfn_layers.0."):]: v for k, v in sd.items()})
    w, b, bp = PillarFeatureNet.fold_state_dict(sd, grid=grid if columns == 10 else None)
    for m in (layer, other):
        fw, fb, fbp = m.folded()
        assert fw.dtype == fb.dtype == torch.float32 and fw.is_contiguous() and fw.requires_grad and fb.requires_grad
        assert np.array_equal(fw.detach().numpy().view(np.uint32), w.view(np.uint32))
        assert np.array_equal(fb.detach().numpy().view(np.uint32), b.view(np.uint32))
        assert (fbp is None) == (columns != 10)
        assert np.array_equal((fb if fbp is None else fbp).detach().numpy().view(np.uint32), bp.view(np.uint32))
    fw, fb, _ = layer.folded()
    (fw.sum() + fb.sum()).backward()                         # the fold is differentiable down to the parameters
    assert layer.linear.weight.grad is not None and layer.norm.weight.grad is not None and layer.norm.bias.grad is not None
    mean = layer.norm.running_mean.clone()
    layer.train()
    layer.folded()
    assert torch.equal(layer.norm.running_mean, mean) and int(layer.norm.num_batches_tracked) == 0      # frozen statistics
