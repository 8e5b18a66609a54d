"""CPU: the edge-aware smoothness on mean-normalised disparity (include/mcav_depth.h: mcav_edge_smooth_fwd / _bwd).  The float64 restatement
(tests/edge_smooth_ref.py) against a literal transcription of the definition and against the closed-form gradient, its edge shapes and
invariances; the per-pixel header csrc/edge_math.h compiled for the host against the restatement; the C ABI's symbols; the kernels in the
compiled gfx950 ISA."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import edge_smooth_ref as R
from conftest import PKG, REPO


def literal(disp, img):
    """The definition transcribed with Python scalars and loops: E for one scale."""
    d, I = disp.tolist(), img.tolist()
    B, _, h, w = disp.shape
    f = img.shape[-2] // h

    def Is(b, c, y, x):
        return sum(I[b][c][y * f + i][x * f + j] for i in range(f) for j in range(f)) / (f * f)
    sx = sy = 0.0
    for b in range(B):
        m = sum(d[b][0][y][x] for y in range(h) for x in range(w)) / (h * w)
        n = [[d[b][0][y][x] / (m + 1e-7) for x in range(w)] for y in range(h)]
        for y in range(h):
            for x in range(w):
                if x < w - 1:
                    wx = math.exp(-(1 / 3) * sum(abs(Is(b, c, y, x) - Is(b, c, y, x + 1)) for c in range(3)))
                    sx += abs(n[y][x] - n[y][x + 1]) * wx
                if y < h - 1:
                    wy = math.exp(-(1 / 3) * sum(abs(Is(b, c, y, x) - Is(b, c, y + 1, x)) for c in range(3)))
                    sy += abs(n[y][x] - n[y + 1][x]) * wy
    return (sx / (B * h * (w - 1)) if w > 1 else 0.0) + (sy / (B * (h - 1) * w) if h > 1 else 0.0)


def inputs(B, H, W, n_scales, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, H, W, generator=g, dtype=dtype)
    disps = [torch.rand(B, 1, H >> s, W >> s, generator=g, dtype=dtype) * 0.8 + 0.1 for s in range(n_scales)]
    return img, disps


@pytest.mark.parametrize("n_scales", [1, 2, 3, 4])
def test_restatement_is_the_definition(n_scales):
    img, disps = inputs(2, 16, 24, n_scales, 10 + n_scales)
    got, _ = R.run(disps, img, weight=1e-3)
    want = 1e-3 / n_scales * sum(2.0 ** -s * literal(d, img) for s, d in enumerate(disps))
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


@pytest.mark.parametrize("B,h,w,f", [(2, 5, 7, 1), (1, 4, 6, 2), (3, 3, 5, 4), (2, 1, 5, 1), (2, 5, 1, 2), (1, 1, 1, 1)])
def test_autograd_gradient_is_the_closed_form(B, h, w, f):
    g = torch.Generator().manual_seed(B * 100 + h * 10 + w)
    img = torch.randn(B, 3, h * f, w * f, generator=g, dtype=torch.float64)
    d = torch.rand(B, 1, h, w, generator=g, dtype=torch.float64) + 0.05
    E, grad = R.run(d, img, weight=1.0)
    want, E_cf = R.closed_form_grad(d, img)
    assert abs(E - E_cf) <= 1e-12 * max(abs(E_cf), 1e-300)
    assert float((grad - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300)
    if h > 1 or w > 1:
        assert abs(E - literal(d, img)) <= 1e-12 * abs(E)


@pytest.mark.parametrize("h,w", [(1, 6), (6, 1), (1, 1)])
def test_edge_shapes_are_finite(h, w):
    img = torch.randn(2, 3, h, w, dtype=torch.float64)
    d = torch.rand(2, 1, h, w, dtype=torch.float64) + 0.1
    E, grad = R.run(d, img, weight=1.0)
    assert math.isfinite(E) and bool(torch.isfinite(grad).all())
    if h == 1 and w == 1:
        assert E == 0.0 and float(grad.abs().max()) == 0.0
    else:
        assert E > 0


def test_constant_disparity_is_exactly_zero():
    img, _ = inputs(2, 16, 24, 1, 3)
    for s in range(3):
        d = torch.full((2, 1, 16 >> s, 24 >> s), 0.37, dtype=torch.float64)
        E, grad = R.run(d, img, weight=1.0)
        assert E == 0.0 and float(grad.abs().max()) == 0.0


def test_scale_invariance_in_float64():
    img, (d,) = inputs(3, 12, 20, 1, 5)
    E1, g = R.run(d, img, weight=1.0)
    E2, _ = R.run(0.5 * d, img, weight=1.0)
    assert abs(E2 - E1) <= 1e-6 * E1                  # only eps breaks the invariance: ~eps / m
    for b in range(3):
        s = float((g[b] * d[b]).sum())
        assert abs(s) <= 1e-6 * float((g[b].abs() * d[b].abs()).sum()), s


# ---------------------------------------------------------------------------------------------- csrc/edge_math.h on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("edge_hostcheck") / "libedge_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(REPO, "tests", "edge_hostcheck", "edge_hostcheck.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.edge_hostcheck.restype = ctypes.c_int
    lib.edge_hostcheck.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_float,
                                                                                               ctypes.c_void_p, ctypes.c_void_p]
    return lib


def host_run(lib, d, img, weight, upstream=1.0):
    B, _, h, w = d.shape
    H, W = img.shape[-2:]
    d32 = np.ascontiguousarray(d.numpy(), dtype=np.float32)
    i32 = np.ascontiguousarray(img.numpy(), dtype=np.float32)
    loss = np.zeros(1, np.float64)
    grad = np.zeros_like(d32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.edge_hostcheck(p(d32), p(i32), B, H, W, h, w, weight, upstream, p(loss), p(grad)) == 0
    return float(loss[0]), torch.from_numpy(grad)


@pytest.mark.parametrize("B,h,w,f", [(2, 5, 7, 1), (2, 33, 65, 1), (2, 16, 32, 2), (1, 8, 16, 4), (2, 4, 8, 8), (1, 1, 5, 1), (2, 5, 1, 1)])
def test_header_on_the_host_matches_the_restatement(host, B, h, w, f):
    g = torch.Generator().manual_seed(7 * h + w)
    img = torch.randn(B, 3, h * f, w * f, generator=g, dtype=torch.float64).float().double()
    d = (torch.rand(B, 1, h, w, generator=g, dtype=torch.float64) * 0.8 + 0.1).float().double()
    loss, grad = host_run(host, d, img, 1e-3, 1.5)
    want, gw = R.run(d, img, weight=1e-3, upstream=1.5)
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
    # fp32 per pixel: a pair whose |delta d| rounds to 0 in one evaluation flips a sign term; none at these sizes
    assert float((grad.double() - gw).norm() / gw.norm()) <= 1e-5
    const = torch.full_like(d, 0.3)
    loss, grad = host_run(host, const, img, 1e-3)
    assert loss == 0.0 and float(grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- the C ABI and the compiled kernels
ENTRIES = ("mcav_edge_smooth_workspace_bytes", "mcav_edge_smooth_fwd", "mcav_edge_smooth_bwd")


def test_library_exports_and_header_declares_the_entries():
    lib_path = os.path.join(PKG, "mcav", "libmcav_depth.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    handle = ctypes.CDLL(lib_path)
    text = open(os.path.join(REPO, "include", "mcav_depth.h")).read()
    import mcav.lib as L
    for name in ENTRIES:
        assert hasattr(handle, name), name
        assert name + "(" in text, name
        assert name in L._SIGNATURES, name
    handle.mcav_edge_smooth_workspace_bytes.restype = ctypes.c_size_t
    assert handle.mcav_edge_smooth_workspace_bytes(12, 192, 640) > 0
    assert handle.mcav_edge_smooth_workspace_bytes(0, 192, 640) == 0


def test_entries_reject_bad_arguments_without_a_device():
    """Every rejection happens before anything touches the device: null pointers, non-positive sizes, shapes that are not an integer
    f x f multiple, B above the ticket capacity, a small workspace."""
    import mcav.lib as L
    h = L.lib()
    fake = ctypes.c_void_p(0x1000)            # never dereferenced: the checks fail first
    ok = dict(B=2, H=8, W=16, h=4, w=8)

    def fwd(ws_bytes=1 << 20, **kw):
        a = dict(ok, **kw)
        return h.mcav_edge_smooth_fwd(fake, fake, a["B"], a["H"], a["W"], a["h"], a["w"], 1e-3, fake, fake, fake, ws_bytes, None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return h.mcav_edge_smooth_bwd(fake, fake, a["B"], a["H"], a["W"], a["h"], a["w"], 1e-3, fake, fake, fake, 0, None)
    for kw in (dict(H=9), dict(W=17), dict(h=3), dict(H=16, W=16), dict(B=0), dict(h=0), dict(w=-1), dict(B=4096)):
        assert fwd(**kw) == -1, kw
        assert bwd(**kw) == -1, kw
    assert fwd(ws_bytes=h.mcav_edge_smooth_workspace_bytes(2, 4, 8) - 1) == -2
    assert h.mcav_edge_smooth_fwd(None, fake, 2, 8, 16, 4, 8, 1e-3, fake, fake, fake, 1 << 20, None) == -1
    assert h.mcav_edge_smooth_bwd(fake, fake, 2, 8, 16, 4, 8, 1e-3, None, fake, fake, 0, None) == -1


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import test_isa_handoff as T
    return T._device_functions(tmp_path_factory, "edge_smooth.hip")


def test_kernels_exist_without_scratch(kernels):
    for kern in ("edge_smooth_fwd_kernel", "edge_smooth_bwd_kernel"):
        names = [n for n in kernels if kern in n]
        assert len(names) == 2, (kern, list(kernels))          # <f == 1 | box-averaged taps>
        for n in names:
            assert not any(i.startswith("scratch_") for i in kernels[n]), n


def test_forward_keeps_the_ticket_hand_off(kernels):
    import test_isa_handoff as T
    tk = T._ticket_kernels(kernels)
    assert [n for n in tk if "edge_smooth_fwd_kernel" in n] and not [n for n in tk if "edge_smooth_bwd_kernel" in n], list(tk)
    T.test_stores_are_acknowledged_before_every_ticket(tk)
    T.test_published_words_and_finisher_reads_are_agent_scope(tk)
