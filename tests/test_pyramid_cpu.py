"""CPU: csrc/pyramid_math.h -- the taps, the adjoint window and both orders of the depth pyramid -- compiled for the host
(tests/pyramid_hostcheck) without fma contraction, against brute force, tests/pyramid_ref.py and float64 autograd."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pyramid_ref as R
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "pyramid_hostcheck", "pyramid_hostcheck.cpp")
PAIRS = [(h, H) for h in range(1, 13) for H in range(h, 4 * h + 4)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pyramid_hostcheck") / "libpyramid_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), SRC, "-o", so])
    lib = ctypes.CDLL(so)
    lib.pyr_weight.restype = ctypes.c_float
    return lib


def header_taps(host, h, H):
    i0, i1, lam = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    rows = []
    for o in range(H):
        host.pyr_taps(o, h, H, ctypes.byref(i0), ctypes.byref(i1), ctypes.byref(lam))
        rows.append((i0.value, i1.value, lam.value))
    return rows


def header_window(host, i, h, H):
    lo, hi = ctypes.c_int(), ctypes.c_int()
    host.pyr_window(i, h, H, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def test_taps_equal_the_numpy_restatement(host):
    """tests/pyramid_ref.py's float32 taps ARE the header's as this build rounds them (no contraction), bit for bit.  The fma form, which the
    device code compiles to and the GPU tests' references use, moves the tap position by at most one rounding of the product: the lower tap
    by at most one index, and where it agrees lam by at most one ulp of n_in."""
    for h, H in PAIRS:
        i0, i1, lam = R.taps(h, H)
        got = header_taps(host, h, H)
        assert [g[0] for g in got] == list(i0) and [g[1] for g in got] == list(i1), (h, H)
        assert np.array_equal(np.array([g[2] for g in got], np.float32), lam), (h, H)
        f0, _, flam = R.taps(h, H, fma=True)
        assert np.abs(f0 - i0).max() <= 1, (h, H)
        same = f0 == i0
        assert np.abs(flam[same].astype(np.float64) - lam[same]).max(initial=0.0) <= h * 2.0 ** -23, (h, H)


def test_adjoint_window_is_exactly_the_touching_outputs(host):
    """Brute force over all outputs: the window of source i holds every output one of whose taps is i, and no other.  Source 0 collects the
    clamped leading run, the last source the trailing one; non-dyadic ratios included."""
    for h, H in PAIRS:
        taps = header_taps(host, h, H)
        for i in range(h):
            touching = [o for o, (i0, i1, _) in enumerate(taps) if i0 == i or i1 == i]
            lo, hi = header_window(host, i, h, H)
            assert touching == list(range(lo, hi + 1)), (h, H, i, lo, hi, touching)
            assert all(host.pyr_weight(o, i, h, H) == 0.0 for o in range(H) if o < lo or o > hi)
        assert header_window(host, 0, h, H)[0] == 0 and header_window(host, h - 1, h, H)[1] == H - 1


def test_adjoint_identity_with_the_headers_weights(host):
    """<A x, y> = <x, A^T y> to float64 rounding, A from the header's weights and A^T y summed over the header's windows only."""
    rng = np.random.default_rng(7)
    for h, H in PAIRS:
        A = np.array([[host.pyr_weight(o, i, h, H) for i in range(h)] for o in range(H)], dtype=np.float64)
        assert np.array_equal(A, R.axis_matrix(h, H).numpy()), (h, H)
        x, y = rng.standard_normal(h), rng.standard_normal(H)
        Aty = np.zeros(h)
        for i in range(h):
            lo, hi = header_window(host, i, h, H)
            Aty[i] = sum(A[o, i] * y[o] for o in range(lo, hi + 1))
        lhs, rhs = float((A @ x) @ y), float(x @ Aty)
        assert abs(lhs - rhs) <= 1e-13 * (np.abs(A) @ np.abs(x)) @ np.abs(y), (h, H, lhs, rhs)


def test_dyadic_weights_equal_interpolate_in_float64(host):
    """For H = h * 2^k the float32 weights are exact: the matrix equals F.interpolate's in float64, bit for bit."""
    seen = 0
    for h, H in PAIRS:
        if H % h or (H // h) & (H // h - 1):
            continue
        seen += 1
        eye = torch.eye(h, dtype=torch.float64).reshape(h, 1, h, 1)            # source k = the k-th unit vector along y
        want = F.interpolate(eye, size=(H, 1), mode="bilinear", align_corners=False)[:, 0, :, 0].T
        assert torch.equal(R.axis_matrix(h, H), want), (h, H)
    assert seen >= 30


def run_host(host, disp, H, W, rtd, d_out):
    B, h, w = disp.shape
    d = np.ascontiguousarray(disp.numpy(), np.float32)
    out = np.zeros((B, H, W), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    host.pyr_fwd(p(d), B, h, w, H, W, int(rtd), p(out))
    g = np.ascontiguousarray(d_out.numpy(), np.float32)
    dd = np.zeros_like(d)
    host.pyr_bwd(p(d), p(out), p(g), B, h, w, H, W, int(rtd), p(dd))
    return torch.from_numpy(out), torch.from_numpy(dd)


@pytest.mark.parametrize("rtd", [False, True], ids=["depth", "disparity"])
@pytest.mark.parametrize("h,w,H,W", [(13, 21, 30, 50), (4, 8, 32, 64)])
def test_both_orders_vs_float64_autograd(host, h, w, H, W, rtd):
    """The header's forward and separable adjoint (x, then y) against float64 autograd through F.interpolate.  Dyadic: the weights are exact,
    so the bounds are pure float32 rounding -- 1e-6 of the largest contributing depth forward (8 operations of 2^-24 each, with margin),
    (N + 8) 2^-24 S backward.  13x21 -> 30x50: autograd is run through the float32 weights widened to float64 (tests/pyramid_ref.py), under
    the same bounds; against F.interpolate's own float64 weights the tap position s <= n_in carries up to 4 n_in 2^-24 of error per axis
    (scale, product, two sums), which bounds the forward distance by (4 (h + w) + 8) 2^-24 of the largest contributing depth."""
    g = torch.Generator().manual_seed(11)
    disp = torch.rand(3, h, w, generator=g)
    d_out = torch.randn(3, H, W, generator=g)
    out, dd = run_host(host, disp, H, W, rtd, d_out)
    want, scale = R.forward64(disp, H, W, rtd)
    assert bool(((out.double() - want).abs() <= 1e-6 * scale).all()), float(((out.double() - want).abs() / scale).max())
    grad, S, N = R.backward64(disp, d_out, rtd)
    assert bool(((dd.double() - grad).abs() <= R.backward_bound(S, N)).all()), float(((dd.double() - grad).abs() / R.backward_bound(S, N)).max())
    # the same through torch's own float64 interpolate and autograd
    x = disp.double().requires_grad_()
    up = lambda t: F.interpolate(t[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    ref = R.depth_of(up(x)) if rtd else up(R.depth_of(x))
    ref.backward(d_out.double())
    dyadic = H % h == 0 and W % w == 0
    if dyadic:
        assert bool(((ref.detach() - want).abs() <= 1e-12 * scale).all())
        assert bool(((x.grad - grad).abs() <= 1e-12 * S + 1e-300).all())
        assert bool(((dd.double() - x.grad).abs() <= R.backward_bound(S, N)).all())
    fwd_tol = (1e-6 if dyadic else (4 * (h + w) + 8) * R.EPS) * scale
    assert bool(((out.double() - ref.detach()).abs() <= fwd_tol).all()), float(((out.double() - ref.detach()).abs() / scale).max())
