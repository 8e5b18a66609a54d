"""CPU: training-mode BatchNorm statistics of the pillar feature layer from the voxels' moments (include/mcav_depth.h: mcav_pillar_moments,
mcav_pillar_moments_bwd; pseudo_lidar.pillar_moments, fold_batch, PillarFeatureLayer(batch_stats=True)).  The identity -- the fold of the
moments against F.linear -> BatchNorm1d(train) -> relu -> max in float64 through autograd -- on the cases of tests/pfn_stats_cases.py;
fold_batch against PillarFeatureNet.fold_state_dict, its 10-column extension, its fallback and the buffers' update against BatchNorm1d;
the header csrc/pfn_stats_math.h compiled for the host against the restatement (tests/pfn_stats_ref.py), once more as a stand-alone
program under the address and undefined-behaviour sanitizers; what the Python side refuses without a GPU; the defaults."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import pfn_ref as R
import pfn_stats_cases as SC
import pfn_stats_ref as SR
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "pfn_stats_hostcheck", "pfn_stats_hostcheck.cpp")
F = np.float32
TOL = 2.0 ** -30                                             # of a tensor's maximum: the float64 slack of the identity
CAP = 0.05                                                   # of a case's (p, o) may be near-ties (tests/test_pfn_bwd_cpu.py)
EPS = 1e-3
IDENTITY = [n for n in SC.ALL if n not in SC.FALLBACK]


def t64(v):
    return torch.from_numpy(np.asarray(v, np.float64).copy())


def close(got, want, what):
    got, want = got.detach(), want.detach()
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print("    %-14s max err %.3g of max %.3g (%.3g)" % (what, err, scale, err / scale if scale else 0.0))
    assert err <= TOL * scale, (what, err, scale)


def live_finite(name):
    """the case's live rows with the pillars that hold a NaN or an infinity emptied (as tests/test_pfn_bwd_cpu.py's finite_copy does)
    -> voxels [P, N, C], num_points [P]"""
    a = SC.build(name)
    P = R.live_pillars(a["offsets"], min(a["capacity"], len(a["voxels"])))
    vox, num = a["voxels"][:P], a["num_points"][:P]
    finite = np.isfinite(vox).all(axis=(1, 2))
    return np.where(finite[:, None, None], vox, F(0)), np.where(finite, num, 0).astype(np.int32)


def moments_of(x, used):
    """differentiable float64 moments of the zero-masked rows x [P, N, C]"""
    flat = x.reshape(-1, x.shape[2])
    head = torch.tensor([float(x.shape[0] * x.shape[1]), float(used.sum())], dtype=torch.float64)
    return torch.cat([head, flat.sum(dim=0), (flat.T @ flat).reshape(-1)])


def folded_features(vox, num, weight, gamma, beta, rm, rv, grid=None):
    """the moments, fold_batch without a rounding, relu and the maximum -> features, mean, var, rows"""
    from pseudo_lidar import fold_batch
    x, used = SR.padded_rows(vox, num)
    wf, bias, bias_pad, mean, var, rows = fold_batch(weight, gamma, beta, moments_of(x, used), EPS, rm, rv, grid, dtype=torch.float64)
    bias_pad = bias if bias_pad is None else bias_pad
    pre = x @ wf.T + torch.where(used[:, :, None], bias[None, None, :], bias_pad[None, None, :])
    return torch.relu(pre).max(dim=1).values, mean, var, rows


def identity(name, weight, grid=None, momentum=0.1):
    from pseudo_lidar.PillarFeatureNet import update_running_stats
    vox, num = live_finite(name)
    c_out = weight.shape[0]
    gamma, beta, rm, rv = SC.norm_parameters(c_out, 40 + c_out)
    zc = None if grid is None else (grid.z[0] + grid.z[1]) / 2.0
    sides = []
    for side in ("stock", "folded"):
        leaves = [t64(v).requires_grad_(True) for v in (vox, weight, gamma, beta)]
        v, w, g, b = leaves
        if side == "stock":
            out = SR.stock(v, num, w, g, b, EPS, t64(rm), t64(rv), momentum, zc)
            feat, near = out["features"], out["near"]
            share = float(near.sum()) / near.numel()
            print("%s: %d of %d (p, o) are near-ties: %.2f %%" % (name, int(near.sum()), near.numel(), 100.0 * share))
            assert share <= CAP
            up = torch.from_numpy(np.random.RandomState(90 + len(name)).standard_normal(tuple(feat.shape))) * ~near
            running = (out["norm"].running_mean, out["norm"].running_var)
        else:
            feat, mean, var, rows = folded_features(v, num, w, g, b, t64(rm), t64(rv), grid)
            norm = torch.nn.BatchNorm1d(c_out, eps=EPS, momentum=momentum).double()
            with torch.no_grad():
                norm.running_mean.copy_(t64(rm)); norm.running_var.copy_(t64(rv))
            update_running_stats(norm, mean, var, rows)
            assert int(norm.num_batches_tracked) == 1
            running = (norm.running_mean, norm.running_var)
        (feat * up).sum().backward()
        sides.append([feat] + [t.grad for t in leaves] + list(running))
    for got, want, what in zip(sides[1], sides[0], ("features", "d_voxels", "d_weight", "d_gamma", "d_beta", "running_mean", "running_var")):
        close(got, want, what)
    assert float(sides[0][1].abs().max()) > 0 and float(sides[0][3].abs().max()) > 0


# ---------------------------------------------------------------------------------------------- 1. the identity
def test_cases_hold_what_they_promise():
    SC.check_non_trivial()


@pytest.mark.parametrize("name", IDENTITY)
def test_fold_of_the_moments_is_batchnorm_behind_the_linear_layer(name):
    """features, the gradients of W, gamma, beta and the voxels, and the running statistics within 2^-30 of each tensor's maximum; the
    upstream gradient of the near-ties (at most 5 % of a case's (p, o)) is zero on both sides"""
    identity(name, SC.build(name)["weight"])


@pytest.mark.parametrize("momentum", [0.01, None])
def test_identity_with_ten_columns(momentum):
    from pseudo_lidar import PillarGrid
    grid = PillarGrid(x=(0.0, 7.0), y=(0.0, 9.0), z=(-3.0, 1.0), size=(1.0, 1.0))
    weight = 0.4 * np.random.RandomState(3).randn(64, 10)
    identity("pair-N5-c9-o64", weight, grid, momentum)


# ---------------------------------------------------------------------------------------------- 2. fold_batch
def random_layer(c_out, columns, seed):
    rng = np.random.RandomState(seed)
    return (0.4 * rng.randn(c_out, columns),) + SC.norm_parameters(c_out, seed + 1)


@pytest.mark.parametrize("columns,name", [(4, "over-N64-c4-o64"), (9, "mixed-N5-c9-o64"), (10, "mixed-N5-c9-o64"), (4, "real-o64")])
def test_fold_batch_gives_fold_state_dicts_bits(columns, name):
    """fold_batch's layer is PillarFeatureNet.fold_state_dict's under the batch statistics as running ones, bit for bit"""
    from pseudo_lidar import PillarFeatureNet, PillarGrid, fold_batch
    grid = PillarGrid(x=(-1.0, 2.5), y=(-1.0, 1.25), z=(-3.0, 1.0), size=(0.5, 0.25)) if columns == 10 else None
    w, gamma, beta, rm, rv = random_layer(64, columns, 7 + columns)
    m = t64(SC.moments(name)["moments"])
    leaves = [t64(v).float().requires_grad_(True) for v in (w, gamma, beta)]
    wf, bias, bias_pad, mean, var, rows = fold_batch(*leaves, m, EPS, t64(rm).float(), t64(rv).float(), grid)
    assert wf.dtype == bias.dtype == torch.float32 and wf.is_contiguous() and wf.requires_grad and mean.dtype == var.dtype == torch.float64
    assert (bias_pad is None) == (columns != 10) and float(rows) == SC.moments(name)["moments"][0] >= 2
    assert not torch.equal(mean, t64(rm).float().double()) and bool((var > 0).all())
    sd = {"linear.weight": leaves[0].detach(), "norm.weight": leaves[1].detach(), "norm.bias": leaves[2].detach(),
          "norm.running_mean": mean.detach(), "norm.running_var": var.detach()}
    want = PillarFeatureNet.fold_state_dict(sd, prefix="", eps=EPS, grid=grid)
    for got, ref in zip((wf, bias, bias if bias_pad is None else bias_pad), want):
        assert np.array_equal(got.detach().numpy().view(np.uint32), ref.view(np.uint32))
    (wf.sum() + bias.sum()).backward()
    assert all(t.grad is not None and float(t.grad.abs().sum()) > 0 for t in leaves)


def test_ten_column_extension_against_ten_explicit_columns():
    """the mean and variance fold_batch takes from nine-column moments under a 10-column weight against the moments of ten explicit
    columns (z - zc in the used slots), float64"""
    from pseudo_lidar import PillarGrid, fold_batch
    grid = PillarGrid(x=(0.0, 7.0), y=(0.0, 9.0), z=(-3.0, 1.0), size=(1.0, 1.0))
    w, gamma, beta, rm, rv = random_layer(64, 10, 21)
    for name in ("mixed-N5-c9-o64", "mixed-N32-c9-o128"):
        vox, num = live_finite(name)
        x9, used = SR.padded_rows(t64(vox), num)
        x10, _ = SR.padded_rows(t64(vox), num, zc=-1.0)
        assert x10.shape[2] == 10 and float(x10[:, :, 9].abs().max()) > 0
        _, _, _, mean, var, rows = fold_batch(t64(w), t64(gamma), t64(beta), moments_of(x9, used), EPS, t64(rm), t64(rv), grid)
        y = (x10 @ t64(w).T).reshape(-1, 64)
        close(mean, y.mean(dim=0), "mean")
        close(var, y.var(dim=0, unbiased=False), "var")


@pytest.mark.parametrize("name", SC.FALLBACK)
def test_fewer_than_two_rows_fold_the_running_statistics(name):
    from pseudo_lidar import PillarFeatureNet, fold_batch
    from pseudo_lidar.PillarFeatureNet import update_running_stats
    w, gamma, beta, rm, rv = random_layer(32, 4, 5)
    m = t64(SC.moments(name)["moments"])
    assert float(m[0]) < 2
    wf, bias, bias_pad, mean, var, rows = fold_batch(t64(w), t64(gamma), t64(beta), m, EPS, t64(rm), t64(rv))
    sd = {"linear.weight": w, "norm.weight": gamma, "norm.bias": beta, "norm.running_mean": rm, "norm.running_var": rv}
    for got, ref in zip((wf, bias), PillarFeatureNet.fold_state_dict(sd, prefix="", eps=EPS)):
        assert np.array_equal(got.numpy().view(np.uint32), ref.view(np.uint32))
    norm = torch.nn.BatchNorm1d(32, eps=EPS)
    with torch.no_grad():
        norm.running_mean.copy_(t64(rm)); norm.running_var.copy_(t64(rv))
    before = [norm.running_mean.clone(), norm.running_var.clone()]
    update_running_stats(norm, mean, var, rows)
    assert int(norm.num_batches_tracked) == 0 and torch.equal(norm.running_mean, before[0]) and torch.equal(norm.running_var, before[1])


@pytest.mark.parametrize("momentum", [0.1, 0.01, None])
def test_buffer_update_is_batchnorms(momentum):
    from pseudo_lidar.PillarFeatureNet import update_running_stats
    gen = torch.Generator().manual_seed(17)
    stock, ours = (torch.nn.BatchNorm1d(32, eps=EPS, momentum=momentum).double() for _ in range(2))
    for step, rows in enumerate((37, 2, 400)):
        y = torch.randn(rows, 32, generator=gen, dtype=torch.float64) * 3.0 + 1.5
        stock.train()(y)
        update_running_stats(ours, y.mean(dim=0), y.var(dim=0, unbiased=False), torch.tensor(float(rows), dtype=torch.float64))
        assert int(ours.num_batches_tracked) == int(stock.num_batches_tracked) == step + 1
        for got, want in ((ours.running_mean, stock.running_mean), (ours.running_var, stock.running_var)):
            assert float(((got - want).abs() / want.abs()).max()) <= 1e-12


# ---------------------------------------------------------------------------------------------- 3. csrc/pfn_stats_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pfn_stats_hostcheck") / "libpfn_stats_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.pfn_stats_host.argtypes = [p, p, p, i, ll, i, i, p]
    lib.pfn_stats_bwd_host.argtypes = [p, p, p, i, ll, i, i, p, p, p]
    return lib


def host_run(host, a, vox, num, grad):
    cap, (_, N, Cc), B = a["capacity"], vox.shape, len(a["offsets"]) - 1
    vox, num, off, grad = (np.ascontiguousarray(v) for v in (vox, num, a["offsets"], grad))
    m, dv = np.full(SR.size(Cc), -7.0), np.full((cap, N, Cc), -7.0, F)
    assert host.pfn_stats_host(vox.ctypes.data, num.ctypes.data, off.ctypes.data, B, cap, N, Cc, m.ctypes.data) == 0
    assert host.pfn_stats_bwd_host(vox.ctypes.data, num.ctypes.data, off.ctypes.data, B, cap, N, Cc, grad[2:].ctypes.data,
                                   grad[2 + Cc:].ctypes.data, dv.ctypes.data) == 0
    return m, dv


@pytest.mark.parametrize("name", SC.ALL)
def test_header_matches_restatement(host, name):
    a = SC.build(name)
    vox, _, num = SC.padded(a, -7.0)
    grad = SC.gradient(name)
    m, dv = host_run(host, a, vox, num, grad)
    SR.check_moments(m, SC.moments(name), name)
    SR.check_backward(dv, SC.backward(name), name)
    m2, dv2 = host_run(host, a, SC.nan_filled(a), num, grad)                               # NaNs wherever the definition does not read
    assert m.tobytes() == m2.tobytes() and dv.tobytes() == dv2.tobytes()


def test_header_refusals(host):
    a = SC.build("mixed-N5-c9-o64")
    vox, _, num = SC.padded(a, 0.0)
    m = np.full(SR.size(9), -7.0)
    good = dict(v=vox.ctypes.data, n=num.ctypes.data, o=a["offsets"].ctypes.data, B=3, cap=a["capacity"], N=5, C=9, m=m.ctypes.data)
    call = lambda **kw: host.pfn_stats_host(*[dict(good, **kw)[k] for k in good])
    assert call() == 0
    m[:] = -7.0
    for kw in (dict(v=None), dict(n=None), dict(o=None), dict(m=None), dict(B=0), dict(B=65536), dict(cap=-1), dict(N=0), dict(N=65), dict(C=5),
               dict(C=10)):
        assert call(**kw) == -1 and (m == -7.0).all(), kw


def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the capacity cut, the clipped counts and
    the real grid's case: a finding ends the program with a non-zero status."""
    exe = str(tmp_path / "pfn_stats_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPFN_STATS_STANDALONE"]) +
                          ["-o", exe])
    for name in ("cut", "clipped", "no-pillars", "real-o64"):
        a = SC.build(name)
        vox, _, num = SC.padded(a, -7.0)
        cap, (_, N, Cc), B = a["capacity"], vox.shape, len(a["offsets"]) - 1
        grad = SC.gradient(name)
        with open(str(tmp_path / "in.bin"), "wb") as f:
            for part in (np.array([B, cap, N, Cc], np.int64), a["offsets"], num, vox, grad[2:]):
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        raw = open(str(tmp_path / "out.bin"), "rb").read()
        assert np.frombuffer(raw, np.int32, 2).tolist() == [0, 0] and len(raw) == 8 + 8 * SR.size(Cc) + 4 * cap * N * Cc
        SR.check_moments(np.frombuffer(raw, np.float64, SR.size(Cc), 8), SC.moments(name), name)
        SR.check_backward(np.frombuffer(raw, F, cap * N * Cc, 8 + 8 * SR.size(Cc)).reshape(cap, N, Cc), SC.backward(name), name)


# ---------------------------------------------------------------------------------------------- 4. refusals without a GPU
def test_python_side_refuses_without_a_gpu():
    import mcav.lib as L
    from pseudo_lidar import PillarBatch, PillarFeatureLayer, PillarGrid, pillar_moments, pillar_moments_backward
    pb = PillarBatch(2, 10, 5, 9, "cpu")
    pb.grid = PillarGrid()
    with pytest.raises(L.MCAVError, match="PillarBatch"):
        pillar_moments(pb.voxels)
    with pytest.raises(L.MCAVError, match="GPU"):
        pillar_moments(pb)                                                                 # CPU buffers
    with pytest.raises(L.MCAVError, match="GPU"):
        pillar_moments_backward(pb, torch.zeros(92, dtype=torch.float64))
    seven = PillarBatch(2, 10, 5, 9, "cpu")
    seven.voxels = torch.zeros(10, 5, 7)
    with pytest.raises(L.MCAVError, match="columns"):
        pillar_moments(seven)
    with pytest.raises(L.MCAVError, match="columns"):
        pillar_moments_backward(seven, torch.zeros(58, dtype=torch.float64))
    pb.voxels.requires_grad_(True)
    with pytest.raises(L.MCAVError, match="gradient"):
        pillar_moments(pb, out=torch.zeros(92, dtype=torch.float64))
    pb.voxels.requires_grad_(False)
    layer = PillarFeatureLayer(batch_stats=True)
    assert layer.training and layer.batch_stats
    for call in (layer, layer.features, layer.folded):
        with pytest.raises(L.MCAVError, match="GPU"):
            call(pb)                                                                       # a layer on the CPU has no path


# ---------------------------------------------------------------------------------------------- 5. the defaults
def test_default_layer_is_frozen_and_the_state_dict_is_unchanged():
    from pseudo_lidar import PillarBatch, PillarFeatureLayer
    default, batch = PillarFeatureLayer(), PillarFeatureLayer(batch_stats=True)
    assert default.batch_stats is False and list(default.state_dict().keys()) == list(batch.state_dict().keys())
    assert not any("batch_stats" in k for k in batch.state_dict())
    default.load_state_dict(batch.state_dict())
    default.train()
    mean, var = default.norm.running_mean.clone(), default.norm.running_var.clone()
    pb = PillarBatch(2, 10, 5, 9, "cpu")
    default.folded(pb)                                       # the pillars are not looked at: today's fold, today's buffers
    for got, want in zip(default.folded(pb), default.folded()):
        assert (got is None and want is None) or torch.equal(got, want)
    assert torch.equal(default.norm.running_mean, mean) and torch.equal(default.norm.running_var, var) and int(default.norm.num_batches_tracked) == 0
    batch.eval()
    for got, want in zip(batch.folded(pb), batch.folded()):  # eval(): the frozen path, no moments
        assert (got is None and want is None) or torch.equal(got, want)
