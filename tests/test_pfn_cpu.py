"""CPU: the pillar feature net and its pseudo-image (include/mcav_depth.h: mcav_pillar_pseudo_image, pseudo_lidar.PillarFeatureNet).  The
restatement (tests/pfn_ref.py) against a float64 torch composition of the stock formulation within the bound of a float32 chain; its fma32
against C's fmaf; the header csrc/pfn_math.h compiled for the host against the restatement, bit for bit, on the cases the GPU tests run
(tests/pfn_cases.py), once more as a stand-alone program under the address and undefined-behaviour sanitizers; the BatchNorm fold of
from_state_dict; what the Python side refuses without a GPU; the new inference flags."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import pfn_cases as C
import pfn_ref as R
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "pfn_hostcheck", "pfn_hostcheck.cpp")
F = np.float32
ALL = C.CASES + [C.REAL_CASE]


# ---------------------------------------------------------------------------------------------- restatement vs stock torch in float64
def torch_float64(a, bias_pad):
    """Linear -> affine (folded) -> relu -> max over the slots with zero-masked padding rows -> zeros canvas -> indexed assignment, all
    float64.  -> canvas, features, and per feature the magnitude sum_c |w x| + |b| of the slot that won (the largest over the slots)"""
    vox = torch.from_numpy(a["voxels"].astype(np.float64))
    w, b, bp = (torch.from_numpy(np.asarray(v, np.float64)) for v in (a["weight"], a["bias"], bias_pad))
    P, N, _ = vox.shape
    used = (torch.arange(N)[None, :] < torch.from_numpy(a["num_points"].astype(np.int64)).clamp(0, N)[:, None])
    masked = vox * used[:, :, None]                                                       # the padding rows are zero rows
    pre = torch.nn.functional.linear(masked, w)                                           # [P, N, C_out]
    pre = pre + torch.where(used[:, :, None], b[None, None, :], bp[None, None, :])        # bias_pad = bias: the plain layer
    feat = torch.relu(pre).max(dim=1).values
    mag = (torch.nn.functional.linear(masked.abs(), w.abs()) + b.abs().maximum(bp.abs())[None, None, :]).max(dim=1).values
    B = len(a["offsets"]) - 1
    canvas = torch.zeros((B, w.shape[0], a["ny"], a["nx"]), dtype=torch.float64)
    c = torch.from_numpy(a["coords"].astype(np.int64))
    canvas[c[:, 0], :, c[:, 2], c[:, 3]] = feat
    return canvas.numpy(), feat.numpy(), mag.numpy()


@pytest.mark.parametrize("pad", ["bias", "zero"])
@pytest.mark.parametrize("case", C.CASES)
def test_restatement_matches_float64_torch(case, pad):
    """|restatement - float64| <= (C + 3) 2^-24 (sum_c |w x| + |b|) per element: the bound of a length-C float32 chain"""
    C.check_non_trivial(case)
    a, want = C.build(case), C.reference(case, pad)
    with np.errstate(invalid="ignore"):
        canvas, feat, mag = torch_float64(a, C.bias_pad(a, pad))
    Cc = a["voxels"].shape[2]
    bound = (Cc + 3) * 2.0 ** -24 * mag
    got = want["features"].astype(np.float64)
    finite = np.isfinite(feat)
    assert np.array_equal(np.isnan(got), np.isnan(feat)) and np.array_equal(got[~finite & ~np.isnan(feat)], feat[~finite & ~np.isnan(feat)])
    with np.errstate(invalid="ignore"):                      # NaN - NaN and inf - inf on elements the masks leave out
        assert finite.sum() >= 32 and (np.abs(got - feat)[finite] <= bound[finite]).all()
    cf = np.isfinite(canvas)
    assert np.array_equal(np.isnan(want["canvas"]), np.isnan(canvas))
    big = np.zeros_like(canvas)
    big[a["coords"][:, 0], :, a["coords"][:, 2], a["coords"][:, 3]] = bound
    with np.errstate(invalid="ignore"):
        assert (np.abs(want["canvas"].astype(np.float64) - canvas)[cf] <= big[cf]).all()
    assert (want["canvas"][canvas == 0].view(np.uint32) == 0).all()                        # +0.0, never -0.0


def test_padding_variants_of_the_definition():
    """bias_pad = bias is the zero-masked padding row through the layer: a partly filled pillar's feature is at least relu(bias);
    any bias_pad <= 0 gives what ignoring the padding gives"""
    a = C.build("pair-N5-c9-o64")
    args = (a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"])
    zero = C.reference("pair-N5-c9-o64", "zero")["features"]
    neg = R.pseudo_image(*args, bias_pad=np.full_like(a["bias"], -3.0))["features"]
    assert np.array_equal(zero.view(np.uint32), neg.view(np.uint32))
    full = C.reference("pair-N5-c9-o64")["features"]
    partly = a["num_points"] < a["voxels"].shape[1]
    relu_b = np.maximum(a["bias"], 0)
    assert np.array_equal(full[partly], np.maximum(zero[partly], relu_b[None, :])) and np.array_equal(full[~partly], zero[~partly])
    assert (full[partly] != zero[partly]).any()
    none = R.pseudo_image(*args[:2], np.zeros_like(a["num_points"]), *args[3:])["features"]            # n = 0: the padding alone
    assert np.array_equal(none, np.broadcast_to(relu_b, none.shape))
    over = R.pseudo_image(*args[:2], a["num_points"] + 100 * (~partly), *args[3:])["features"]         # n above N is N
    assert np.array_equal(over.view(np.uint32), full.view(np.uint32))


# ---------------------------------------------------------------------------------------------- csrc/pfn_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pfn_hostcheck") / "libpfn_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.pfn_host_pseudo_image.argtypes = [p, p, p, p, i, ll, i, i, i, i, p, p, p, i, i, p, p]
    lib.pfn_host_fmaf.argtypes = [p, p, p, p, ll]
    lib.pfn_host_first_at_or_after.argtypes = [p, ll, ll, i, i]
    lib.pfn_host_first_at_or_after.restype = ll
    return lib


def host_run(host, a, pad="bias", capacity=None, nhwc=False, canvas=True, features=True, **kw):
    """-> status, canvas (as [B, C_out, ny, nx]) and features [capacity, C_out], both pre-filled with -7"""
    B, (cap, N, Cc), c_out = len(a["offsets"]) - 1, a["voxels"].shape, a["weight"].shape[0]
    cap = cap if capacity is None else capacity
    shape = (B, a["ny"], a["nx"], c_out) if nhwc else (B, c_out, a["ny"], a["nx"])
    cv, ft = np.full(shape, -7.0, F), np.full((max(cap, 1), c_out), -7.0, F)
    arrays = dict(voxels=a["voxels"], coords=a["coords"], num_points=a["num_points"], offsets=a["offsets"], weight=a["weight"],
                  bias=a["bias"], bias_pad=C.bias_pad(a, pad))
    ptr = {k: np.ascontiguousarray(v).ctypes.data for k, v in arrays.items()}
    arg = dict(B=B, capacity=cap, N=N, C=Cc, nx=a["nx"], ny=a["ny"], c_out=c_out, flags=1 if nhwc else 0,
               canvas=cv.ctypes.data if canvas else None, features=ft.ctypes.data if features else None)
    arg.update(ptr)
    arg.update(kw)
    rc = host.pfn_host_pseudo_image(arg["voxels"], arg["coords"], arg["num_points"], arg["offsets"], arg["B"], arg["capacity"], arg["N"],
                                    arg["C"], arg["nx"], arg["ny"], arg["weight"], arg["bias"], arg["bias_pad"], arg["c_out"], arg["flags"],
                                    arg["canvas"], arg["features"])
    return rc, (cv.transpose(0, 3, 1, 2) if nhwc else cv), ft


def test_fma32_is_c_fmaf(host):
    """the restatement's fused multiply-add against C's, bit for bit: random triples over many exponents, sums that nearly cancel, ties of
    the float32 rounding that only the exact sum decides, subnormal results, zeros of both signs, infinities and NaNs"""
    rng = np.random.RandomState(3)
    n = 400000
    a = (rng.randn(n) * 2.0 ** rng.randint(-20, 20, n)).astype(F)
    b = (rng.randn(n) * 2.0 ** rng.randint(-20, 20, n)).astype(F)
    c = (rng.randn(n) * 2.0 ** rng.randint(-30, 30, n)).astype(F)
    near = (-(a.astype(np.float64) * b.astype(np.float64))).astype(F)                      # a b + c cancels to the product's rounding error
    c[::4] = near[::4]
    c[1::8] = np.nextafter(near[1::8], F(0))
    odd = rng.randint(1 << 22, 5592405, n // 10) * 2 + 1                                   # odd, in [2^23, 2^24 / 1.5)
    a[:n // 10], b[:n // 10] = odd.astype(F), F(1.5)                                       # odd * 1.5 = x.5 below 2^24: a float32 tie ...
    c[:n // 10] = (2.0 ** -40 * rng.choice([-1.0, 1.0], n // 10)).astype(F)                # ... that an addend below float64's reach breaks
    a[n // 10:n // 5] *= F(2.0 ** -70)
    b[n // 10:n // 5] *= F(2.0 ** -70)                                                     # subnormal and underflowing products
    c[n // 10:n // 5:2] = 0.0
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.4e38, 1e-45], F)
    sa, sb, sc = (v.reshape(-1) for v in np.meshgrid(special, special, special))
    a, b, c = np.concatenate([a, sa]), np.concatenate([b, sb]), np.concatenate([c, sc])
    want = np.empty_like(a)
    host.pfn_host_fmaf(a.ctypes.data, b.ctypes.data, c.ctypes.data, want.ctypes.data, len(a))
    got = R.fma32(a, b, c)
    C.same_bits(got, want)
    with np.errstate(invalid="ignore", over="ignore"):
        plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    ok = ~np.isnan(want)
    assert (plain[ok].view(np.uint32) != want[ok].view(np.uint32)).sum() > 10              # a double rounding would have shown


@pytest.mark.parametrize("case", ALL)
def test_header_matches_restatement(host, case):
    a, want = C.build(case), C.reference(case)
    P = len(want["features"])
    for nhwc in ((False, True) if case != C.REAL_CASE else (False,)):
        rc, canvas, feat = host_run(host, a, nhwc=nhwc)
        assert rc == 0
        C.same_bits(np.ascontiguousarray(canvas), want["canvas"])
        C.same_bits(feat[:P], want["features"])


def test_header_padding_capacity_and_optional_outputs(host):
    case = C.HARDEST
    a = C.build(case)
    rc, canvas, feat = host_run(host, a, pad="zero")
    assert rc == 0
    C.same_bits(np.ascontiguousarray(canvas), C.reference(case, "zero")["canvas"])
    cap = C.cut_capacity(case)
    cut = C.reference(case, "bias", cap)
    rc, canvas, feat = host_run(host, a, capacity=cap)
    assert rc == 0 and len(cut["features"]) == cap
    C.same_bits(np.ascontiguousarray(canvas), cut["canvas"])
    C.same_bits(feat, cut["features"])
    full = C.reference(case)["canvas"]
    dropped = a["coords"][cap:]
    assert np.isnan(full).sum() > np.isnan(cut["canvas"]).sum() > 0                        # a NaN pillar on each side of the cut
    assert (cut["canvas"][dropped[:, 0], :, dropped[:, 2], dropped[:, 3]].view(np.uint32) == 0).all()
    rc, canvas, feat = host_run(host, a, features=False)
    assert rc == 0 and (feat == -7).all()
    C.same_bits(np.ascontiguousarray(canvas), full)
    rc, canvas, feat = host_run(host, a, canvas=False)
    assert rc == 0 and (canvas == -7).all()
    C.same_bits(feat, C.reference(case)["features"])


def test_header_skips_rows_outside_the_canvas(host):
    """rows whose (b, iy, ix) name no cell, sorted where they belong, leave the canvas as it is without them"""
    a = dict(C.build("fullrow-o32"))
    coords = a["coords"].copy()
    coords[6, 3] = 7                                         # ix = nx: behind the last cell of its row
    coords[7, 2] = -1                                        # iy = -1: in front of the second image's first row
    a["coords"] = coords
    rc, canvas, feat = host_run(host, a)
    assert rc == 0
    want = R.pseudo_image(a["voxels"], coords, a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"])
    C.same_bits(np.ascontiguousarray(canvas), want["canvas"])
    assert (want["canvas"][0, :, 3, 6] == 0).all() and (want["canvas"][1, :, 0, 0] == 0).all() and (feat[[6, 7]] == -7).all()
    keep = np.ones(len(coords), bool)
    keep[[6, 7]] = False
    C.same_bits(feat[keep], want["features"][keep])


def test_header_row_search(host):
    coords = np.array([[0, 0, 1, 2], [0, 0, 1, 5], [0, 0, 3, 0], [0, 0, 3, 127], [0, 0, 3, 128], [0, 0, 8, 1]], np.int32)
    for (y, x), r in (((0, 0), 0), ((1, 2), 0), ((1, 3), 1), ((1, 6), 2), ((3, 0), 2), ((3, 128), 4), ((3, 129), 5), ((9, 0), 6), ((8, 2), 6)):
        assert host.pfn_host_first_at_or_after(coords.ctypes.data, 0, 6, y, x) == r
    assert host.pfn_host_first_at_or_after(coords.ctypes.data, 2, 2, 0, 0) == 2


def test_header_refusals(host):
    a = C.build("mixed-N5-c9-o64")
    assert host_run(host, a)[0] == 0
    bad = [dict(voxels=None), dict(coords=None), dict(num_points=None), dict(offsets=None), dict(weight=None), dict(bias=None),
           dict(bias_pad=None), dict(canvas=None, features=None), dict(B=0), dict(B=65536), dict(capacity=-1), dict(N=0), dict(N=65), dict(C=5),
           dict(C=10), dict(c_out=0), dict(c_out=48), dict(c_out=160), dict(flags=2), dict(nx=0), dict(ny=0), dict(nx=1 << 16, ny=1 << 14)]
    for kw in bad:
        rc, canvas, feat = host_run(host, a, **kw)
        assert rc == -1 and (canvas == -7).all() and (feat == -7).all(), kw


def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the hardest case (the wide grid with its
    partial last column tile, NaN rows) at full capacity and with a capacity that ends inside the second image, in both layouts: a
    finding ends the program with a non-zero status."""
    exe = str(tmp_path / "pfn_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPFN_STANDALONE"]) +
                          ["-o", exe])
    a = C.build(C.HARDEST)
    B, (P, N, Cc), c_out = len(a["offsets"]) - 1, a["voxels"].shape, a["weight"].shape[0]
    for cap, nhwc in ((P, 0), (C.cut_capacity(C.HARDEST), 1)):
        want = C.reference(C.HARDEST, "bias", cap)
        head = np.array([B, cap, N, Cc, a["nx"], a["ny"], c_out, nhwc, 1, 0], np.int64)
        with open(str(tmp_path / "in.bin"), "wb") as f:
            for part in (head, a["offsets"], a["num_points"][:cap], a["coords"][:cap], a["voxels"][:cap], a["weight"], a["bias"], a["bias"]):
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        raw = open(str(tmp_path / "out.bin"), "rb").read()
        assert np.frombuffer(raw, np.int32, 1)[0] == 0
        n = want["canvas"].size
        canvas = np.frombuffer(raw, F, n, 4)
        canvas = canvas.reshape(B, a["ny"], a["nx"], c_out).transpose(0, 3, 1, 2) if nhwc else canvas.reshape(want["canvas"].shape)
        feat = np.frombuffer(raw, F, cap * c_out, 4 + 4 * n).reshape(cap, c_out)
        assert 4 + 4 * n + 4 * feat.size == len(raw)
        C.same_bits(np.ascontiguousarray(canvas), want["canvas"])
        C.same_bits(feat, want["features"])


# ---------------------------------------------------------------------------------------------- from_state_dict
class Unfolded(torch.nn.Module):
    """second.pytorch's PFNLayer in evaluation mode, float64"""

    def __init__(self, c_in, c_out, bias):
        super().__init__()
        self.linear = torch.nn.Linear(c_in, c_out, bias=bias)
        self.norm = torch.nn.BatchNorm1d(c_out, eps=1e-3)

    def forward(self, x):                                    # [P, N, c_in] -> [P, c_out]
        y = self.norm(self.linear(x).permute(0, 2, 1)).permute(0, 2, 1)
        return torch.relu(y).max(dim=1).values


@pytest.mark.parametrize("columns,linear_bias", [(9, False), (10, False), (4, True)])
def test_from_state_dict_folds_the_batchnorm(columns, linear_bias):
    """the folded float32 layer, evaluated in float64, against the unfolded float64 module on zero-masked pillars: within one rounding of
    w' and b' -- 2^-24 (sum_c |w' x| + |b'|) per element; the 10th column is z - zc on used slots and 0 on padding rows"""
    from pseudo_lidar import PillarFeatureNet, PillarGrid
    torch.manual_seed(columns)
    m = Unfolded(columns, 64, linear_bias).double().eval()
    with torch.no_grad():
        m.norm.weight.copy_(torch.randn(64).double().abs() + 0.5)
        m.norm.bias.copy_(torch.randn(64).double() * 0.3)
        m.norm.running_mean.copy_(torch.randn(64).double() * 0.2)
        m.norm.running_var.copy_(torch.rand(64).double() + 0.1)
    sd = {"vfe.pfn_layers.0." + k: v for k, v in m.state_dict().items()}
    grid = PillarGrid(x=(-1.0, 2.5), y=(-1.0, 1.25), z=(-3.0, 1.0), size=(0.5, 0.25))
    w, b, bp = PillarFeatureNet.fold_state_dict(sd, grid=grid if columns == 10 else None)
    Cc = 9 if columns == 10 else columns
    assert w.shape == (64, Cc) and b.shape == bp.shape == (64,) and w.dtype == b.dtype == bp.dtype == F
    assert (columns == 10) == (not np.array_equal(b, bp))
    rw, rb, rbp = R.fold_batchnorm(m.linear.weight.detach().numpy(), m.norm.weight.detach().numpy(), m.norm.bias.detach().numpy(),
                                   m.norm.running_mean.numpy(), m.norm.running_var.numpy(), 1e-3,
                                   m.linear.bias.detach().numpy() if linear_bias else None, zc=-1.0)
    assert np.array_equal(w, rw) and np.array_equal(b, rb) and np.array_equal(bp, rbp)
    a = C.build("pair-N5-c9-o64")
    vox = a["voxels"][:, :, :Cc].astype(np.float64)
    N = vox.shape[1]
    used = np.arange(N)[None, :] < a["num_points"][:, None]
    x = vox * used[:, :, None]
    if columns == 10:
        x = np.concatenate([x, ((vox[:, :, 2] - (-1.0)) * used)[:, :, None]], axis=2)      # zc = (-3 + 1) / 2
    with torch.no_grad():
        want = m(torch.from_numpy(x)).numpy()
    got = R.features(np.ascontiguousarray(a["voxels"][:, :, :Cc]), a["num_points"], len(vox), w, b, bp).astype(np.float64)
    w64, b64, bp64 = w.astype(np.float64), b.astype(np.float64), bp.astype(np.float64)
    mag = (np.abs(vox * used[:, :, None]) @ np.abs(w64).T + np.maximum(np.abs(b64), np.abs(bp64))).max(axis=1)
    assert (np.abs(got - want) <= (Cc + 3 + 1) * 2.0 ** -24 * mag).all()                   # the chain's bound and one rounding of w', b'
    assert np.abs(got - want).max() > 0                      # the fold rounds: equality would mean nothing was compared


def test_from_state_dict_refusals():
    import mcav.lib as L
    from pseudo_lidar import PillarFeatureNet, PillarGrid
    good = {"p.linear.weight": torch.zeros(64, 9), "p.norm.weight": torch.ones(64), "p.norm.bias": torch.zeros(64),
            "p.norm.running_mean": torch.zeros(64), "p.norm.running_var": torch.ones(64)}
    assert PillarFeatureNet.fold_state_dict(good, prefix="p.")[0].shape == (64, 9)
    bad = [dict(good, **{"p.linear.weight": torch.zeros(64, 8)}), dict(good, **{"p.linear.weight": torch.zeros(48, 9)}),
           dict(good, **{"p.linear.weight": torch.zeros(64, 10)}),                         # 10 columns without a grid
           dict(good, **{"p.linear.weight": torch.zeros(64)}), dict(good, **{"p.norm.bias": torch.zeros(32)}),
           dict(good, **{"p.norm.running_var": -torch.ones(64)}), dict(good, **{"p.linear.bias": torch.zeros(63)}),
           {k: v for k, v in good.items() if k != "p.norm.running_mean"}]
    for sd in bad:
        with pytest.raises(L.MCAVError):
            PillarFeatureNet.fold_state_dict(sd, prefix="p.")
    with pytest.raises(L.MCAVError):
        PillarFeatureNet.fold_state_dict(good)                                             # nothing under the default prefix
    ten = dict(good, **{"p.linear.weight": torch.zeros(64, 10)})
    assert PillarFeatureNet.fold_state_dict(ten, prefix="p.", grid=PillarGrid())[0].shape == (64, 9)


# ---------------------------------------------------------------------------------------------- the Python side without a GPU
def cpu_layer(c_out=64, columns=9):
    """a layer that never reaches a device: the constructor refuses CPU tensors, the checks of a call come before any device is needed"""
    from pseudo_lidar import PillarFeatureNet
    net = PillarFeatureNet.__new__(PillarFeatureNet)
    net.weight, net.bias, net.bias_pad = torch.zeros(c_out, columns), torch.zeros(c_out), torch.zeros(c_out)
    net.c_out, net.columns = c_out, columns
    return net


def test_python_side_refuses_without_a_gpu():
    import mcav.lib as L
    from pseudo_lidar import PillarBatch, PillarFeatureNet, PillarGrid
    for args in ((torch.zeros(64, 9), torch.zeros(64)),                                   # CPU tensors
                 (np.zeros((64, 9), F), np.zeros(64, F)), (torch.zeros(64, 8), torch.zeros(64)), (torch.zeros(48, 9), torch.zeros(48)),
                 (torch.zeros(64, 9), torch.zeros(32)), (torch.zeros(64, 9), torch.zeros(64), torch.zeros(1, 64)), (torch.zeros(9), torch.zeros(64)),
                 (torch.zeros(64, 9, dtype=torch.float64), torch.zeros(64, dtype=torch.float64))):
        with pytest.raises(L.MCAVError):
            PillarFeatureNet(*args)
    net = cpu_layer()
    pb = PillarBatch(2, 10, 5, 9, "cpu")
    pb.grid = PillarGrid()
    with pytest.raises(L.MCAVError, match="GPU"):
        net.pseudo_image(pb)                                                               # CPU buffers
    with pytest.raises(L.MCAVError, match="GPU"):
        net.features(pb)
    with pytest.raises(L.MCAVError, match="layout"):
        net.pseudo_image(pb, layout="chwn")
    with pytest.raises(L.MCAVError, match="PillarBatch"):
        net.pseudo_image(pb.voxels)
    pb.grid = None
    with pytest.raises(L.MCAVError, match="grid"):
        net.pseudo_image(pb)
    with pytest.raises(L.MCAVError, match="grid"):
        pb.pseudo_image(net)                                                               # the shortcut is the same call
    four = PillarBatch(2, 10, 5, 4, "cpu")
    four.grid = PillarGrid()
    with pytest.raises(L.MCAVError, match="columns"):
        net.pseudo_image(four)
    with pytest.raises(L.MCAVError, match="columns"):
        net.features(four)
    for spoil in (lambda o: setattr(o, "coords", o.coords[:, :3]), lambda o: setattr(o, "num_points", o.num_points[:5]),
                  lambda o: setattr(o, "offsets", o.offsets.reshape(1, 3)), lambda o: setattr(o, "voxels", torch.zeros(10, 65, 9))):
        out = PillarBatch(2, 10, 5, 9, "cpu")
        out.grid = PillarGrid()
        spoil(out)
        with pytest.raises(L.MCAVError) as e:
            net.pseudo_image(out)
        assert "GPU" not in str(e.value)                                                   # refused for its shape, before any device check


def test_inference_pfn_flags():
    import inference
    assert callable(inference.Inference.pseudo_images)
    base = ["--config", "c.yaml", "--checkpoint", "x.pth", "--out", "o"]
    parse = lambda argv: inference.build_parser().parse_args(argv)
    assert inference.pfn_arguments(parse(base)) is None and inference.pfn_arguments(parse(base + ["--pillars"])) is None
    assert inference.pfn_arguments(parse(base + ["--pillars", "--pfn", "det.pth"])) == ("det.pth", "vfe.pfn_layers.0.")
    assert inference.pfn_arguments(parse(base + ["--pillars", "--pfn", "det.pth", "--pfn-prefix", "m."])) == ("det.pth", "m.")
    with pytest.raises(ValueError):
        inference.main(base + ["--pfn", "det.pth"])                                        # refused before the config is read
    kw = inference.pillar_arguments(parse(base + ["--pillars", "--pfn", "det.pth"]))
    assert sorted(kw) == ["grid", "max_points"]                                            # what --pillars gives is what it gave


def test_save_npz_takes_features(tmp_path):
    """without features the .npz holds what it held; with them one more array, the image's rows"""
    from pseudo_lidar import PillarBatch
    a = C.build("pair-N5-c9-o64")
    P = len(a["coords"])
    pb = PillarBatch(3, P + 4, 5, 9, "cpu")
    pb.voxels[:P], pb.coords[:P], pb.num_points[:P] = (torch.from_numpy(a[n].copy()) for n in ("voxels", "coords", "num_points"))
    pb.offsets.copy_(torch.from_numpy(a["offsets"].copy()))
    feat = torch.arange((P + 4) * 64, dtype=torch.float32).reshape(P + 4, 64)
    plain, with_f = [str(tmp_path / ("p%d.npz" % b)) for b in range(3)], [str(tmp_path / ("f%d.npz" % b)) for b in range(3)]
    pb.save_npz(plain)
    pb.save_npz(with_f, features=feat)
    for b in range(3):
        lo, hi = a["offsets"][b], a["offsets"][b + 1]
        z, zf = np.load(plain[b]), np.load(with_f[b])
        assert sorted(z.files) == ["coords", "num_points", "voxels"] and sorted(zf.files) == ["coords", "features", "num_points", "voxels"]
        assert np.array_equal(zf["features"], feat[lo:hi].numpy()) and np.array_equal(zf["voxels"].view(np.uint32), z["voxels"].view(np.uint32))
