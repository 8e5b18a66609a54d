"""CPU: the depth geometry-consistency term (include/mcav_depth.h: mcav_geom_consistency_fwd / _bwd).  The float64 definition
(tests/geom_consistency_ref.py) under gradcheck and on its closed forms; the per-pixel header csrc/geom_math.h compiled for the host
(fp32, no FMA contraction, the fixed-point scatter, single-threaded) against the definition on the GPU tests' inputs -- its measured
deviation is the basis of the GPU tolerances -- and as a stand-alone program under the address and undefined-behaviour sanitizers; the C
ABI's symbols and argument checks; the kernels in the compiled gfx950 ISA."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import geom_consistency_ref as R
from conftest import PKG, REPO

# The inputs shared with tests/test_geom_consistency_gpu.py: name -> (B, H, W, seed, extra inputs() arguments, min_valid).  Seeds are
# chosen so that the definition itself flags at most 0.5 % of the pixels as ties, and none of them at a validity border: no pixel can
# change n_d, so the scalars need no allowance beyond the kernel tolerance (check_case_ties asserts both).
CASES = {
    "24x40": (2, 24, 40, 11, {}, 100),
    "23x37": (2, 23, 37, 4, {}, 100),              # odd sizes: ragged tiles, the halo
    "8x16": (1, 8, 16, 3, {}, 0),
    "many_to_one": (2, 24, 40, 3, {"forward": 20.0}, 100),      # a (direction 0) shrinks into a few dozen texels of b
}
MAX_FLAGGED = 0.005

# MEASURED: the host check's (fp32, no FMA) maximum deviation from the float64 definition on those inputs, as a fraction of the
# reference tensor's maximum, over the pixels the definition does not flag (for the gradients: nor the texels a flagged pixel reaches).
# The GPU tests allow the kernels 4x these (FMA contraction, v_rcp + Newton) plus 1e-7 of the tensor's maximum.  This file asserts that
# the host check stays within them, so they cannot go stale.
HOST_DEV = {
    "24x40": dict(diff=6.1e-07, d_disp_t=3.1e-06, d_disp_r=1.9e-06, loss=2.5e-09, d_poses=5.9e-07),
    "23x37": dict(diff=7.3e-07, d_disp_t=5.3e-06, d_disp_r=2.3e-06, loss=2.9e-08, d_poses=4.1e-07),
    "8x16": dict(diff=2.2e-07, d_disp_t=1.1e-06, d_disp_r=1.7e-06, loss=4.5e-08, d_poses=1.4e-07),
    "many_to_one": dict(diff=1.7e-07, d_disp_t=5.8e-07, d_disp_r=1.4e-06, loss=1.4e-09, d_poses=1.7e-07),
}

_REF = {}


def case_inputs(name):
    B, H, W, seed, kw, min_valid = CASES[name]
    return R.inputs(B, H, W, seed, **kw) + (min_valid,)


def reference(name, weight=1.0):
    """The float64 definition on a case's inputs: computed once, shared, never modified."""
    if name not in _REF:
        dt, dr, poses, K, mv = case_inputs(name)
        _REF[name] = R.run(dt, dr, poses, K, min_valid=mv)
    return _REF[name]


def deviations(got, ref):
    """got: dict(loss, diff, d_disp_t, d_disp_r, d_poses) of an fp32 evaluation.  -> the figures HOST_DEV records, and the scalar
    allowances for the flagged pixels."""
    keep = ~ref["flagged"]
    out = {}
    d = (got["diff"].double() - ref["diff"]).abs()
    out["diff"] = float(d[keep].max() / ref["diff"].abs().max())
    for k, plane in (("d_disp_t", 0), ("d_disp_r", 1)):
        ok = keep[:, plane] & ~ref["touched"][:, plane]
        g = (got[k].double()[:, 0] - ref[k][:, 0]).abs()
        out[k] = float(g[ok].max() / ref[k].abs().max())
    out["loss"] = abs(got["loss"] - ref["loss"]) / max(abs(ref["loss"]), 1e-300)
    out["d_poses"] = float((got["d_poses"].double() - ref["d_poses"]).abs().max() / ref["d_poses"].abs().max())
    return out


# ---------------------------------------------------------------------------------------------- the definition
def test_definition_passes_gradcheck():
    dt, dr, poses, K = R.inputs(1, 6, 9, 9)
    res = R.run(dt, dr, poses, K, min_valid=0)
    assert int(res["flagged"].sum()) == 0 and min(res["n"]) > 5, (res["n"], int(res["flagged"].sum()))
    fn = lambda a, b, p: R.geom_consistency(a, b, p, K, min_valid=0)[0]
    args = [t.clone().requires_grad_() for t in (dt, dr, poses)]
    assert torch.autograd.gradcheck(fn, args, eps=1e-7, atol=1e-6, rtol=1e-5)


def closed_form_inputs(B=2, H=6, W=9, ratio=1.0):
    """Zero pose, constant depths D_t = 0.75 and D_r = ratio * D_t; focal lengths that are powers of two, so that K K^-1 = I exactly and a
    border pixel projects onto itself (it stays valid in float32 as in float64)."""
    K = torch.tensor([[16.0, 0, (W - 1) / 2], [0, 32.0, (H - 1) / 2], [0, 0, 1]], dtype=torch.float64).repeat(B, 1, 1)
    Dt = torch.full((B, 1, H, W), 0.75, dtype=torch.float64)
    return Dt, ratio * Dt, torch.zeros(B, 2, 6, dtype=torch.float64), K


def check_closed_forms(evaluate):
    """evaluate(Dt, Dr, poses, K, min_valid) -> dict(loss, n, diff, d_disp_t, d_disp_r, d_poses) on DEPTH inputs."""
    Dt, Dr, poses, K = closed_form_inputs(ratio=1.0)
    r = evaluate(Dt, Dr, poses, K, 0)
    assert r["loss"] == 0.0 and list(r["n"]) == [108, 108]
    for k in ("d_disp_t", "d_disp_r", "d_poses"):
        assert float(r[k].abs().max()) == 0.0, k
    Dt, Dr, poses, K = closed_form_inputs(ratio=2.0)
    r = evaluate(Dt, Dr, poses, K, 100)
    assert list(r["n"]) == [108, 108]                      # every pixel is valid: n_d = B H W
    assert abs(r["loss"] - 1 / 3) < 1e-4                   # up to the + 1e-5 of the projection
    assert float((r["diff"].double() - 1 / 3).abs().max()) < 1e-4
    r = evaluate(Dt, Dr, poses, K, 108)                    # n_d <= min_valid: nothing
    assert r["loss"] == 0.0
    for k in ("d_disp_t", "d_disp_r", "d_poses"):
        assert float(r[k].abs().max()) == 0.0, k


def test_definition_closed_forms():
    check_closed_forms(lambda Dt, Dr, p, K, mv: R.run(Dt, Dr, p, K, min_valid=mv, inputs_are_depth=True))


def check_case_ties(name, ref):
    """What the choice of seeds promises about a case, by the definition itself."""
    assert ref["flagged_share"] <= MAX_FLAGGED, ref["flagged_share"]
    assert ref["border"] == [0, 0], ref["border"]
    if name != "many_to_one":
        assert 0.07 <= ref["valid_share"] <= 0.93, ref["valid_share"]
    else:                                                  # direction 0 lands in a few dozen texels, direction 1 is behind the camera
        assert ref["n"][1] == 0 and ref["n"][0] > 1000 and int((ref["d_disp_r"] != 0).sum()) < 100, ref["n"]


def scalar_allowance(ref):
    """What pixels at a validity border may do to the loss on top of the kernel tolerance, as a fraction of the loss: such a pixel moves
    n_d by one and E_d by at most 1 / n_d (diff <= 1), each direction weighing 0.5.  Zero for the seeds in use."""
    return sum(0.5 * b / n for b, n in zip(ref["border"], ref["n"]) if n > 0) / max(abs(ref["loss"]), 1e-300)


# ---------------------------------------------------------------------------------------------- csrc/geom_math.h on the host
SRC = os.path.join(REPO, "tests", "geom_hostcheck", "geom_hostcheck.cpp")
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("geom_hostcheck") / "libgeom_hostcheck.so")
    subprocess.check_call(GXX + ["-shared", "-fPIC", SRC, "-o", so])
    lib = ctypes.CDLL(so)
    lib.geom_hostcheck.restype = ctypes.c_int
    lib.geom_hostcheck.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_uint, ctypes.c_int, ctypes.c_float,
                                                                                 ctypes.c_float] + [ctypes.c_void_p] * 6
    return lib


def host_run(lib, dt, dr, poses, K, min_valid, weight=1.0, upstream=1.0, inputs_are_depth=False):
    B, _, H, W = dt.shape
    f32 = lambda t: np.ascontiguousarray(t.numpy(), dtype=np.float32)
    a, b, p = f32(dt), f32(dr), f32(poses)
    k = np.ascontiguousarray(K.numpy(), dtype=np.float64)
    loss, n = np.zeros(1, np.float64), np.zeros(2, np.float64)
    diff = np.zeros((B, 2, H, W), np.float32)
    gt, gr, gp = np.zeros_like(a), np.zeros_like(b), np.zeros_like(p)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = lib.geom_hostcheck(ptr(a), ptr(b), ptr(p), ptr(k), B, H, W, 8 if inputs_are_depth else 0, min_valid, weight, upstream, ptr(loss),
                            ptr(n), ptr(diff), ptr(gt), ptr(gr), ptr(gp))
    assert rc == 0, rc
    return dict(loss=float(loss[0]), n=[int(n[0]), int(n[1])], diff=torch.from_numpy(diff), d_disp_t=torch.from_numpy(gt),
                d_disp_r=torch.from_numpy(gr), d_poses=torch.from_numpy(gp))


def test_header_on_the_host_closed_forms(host):
    check_closed_forms(lambda Dt, Dr, p, K, mv: host_run(host, Dt, Dr, p, K, mv, inputs_are_depth=True))


@pytest.mark.parametrize("name", list(CASES))
def test_header_on_the_host_matches_the_definition(host, name):
    dt, dr, poses, K, mv = case_inputs(name)
    ref = reference(name)
    got = host_run(host, dt, dr, poses, K, mv)
    dev = deviations(got, ref)
    print(name, "n", got["n"], ref["n"], {k: "%.3g" % v for k, v in dev.items()})
    check_case_ties(name, ref)
    assert got["n"] == ref["n"]                            # no pixel sits at a validity border
    assert bool(((got["diff"] >= 0) == (ref["diff"] >= 0)).all())
    for k, v in dev.items():
        allow = HOST_DEV[name][k] + (scalar_allowance(ref) if k == "loss" else 0.0)
        assert v <= allow, (k, v, allow)


def test_scaled_upstream_and_weight_on_the_host(host):
    dt, dr, poses, K, mv = case_inputs("23x37")
    a = host_run(host, dt, dr, poses, K, mv)
    b = host_run(host, dt, dr, poses, K, mv, weight=0.5, upstream=3.0)
    assert abs(b["loss"] - 0.5 * a["loss"]) <= 1e-12
    for k in ("d_disp_t", "d_disp_r", "d_poses"):
        assert float((b[k] - 1.5 * a[k]).abs().max()) <= 2e-6 * float(a[k].abs().max()), k


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same source with its own main(), built with -fsanitize=address,undefined and run as a program of its own: out-of-bounds taps,
    signed overflow in the fixed-point sums and float -> integer conversions outside the range would all stop it."""
    exe = str(tmp_path / "geom_hostcheck_san")
    cmd = GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGEOM_HOSTCHECK_MAIN", SRC, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("g++ has no sanitizer runtime here")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "geom_hostcheck: ok" in run.stdout, (run.stdout, run.stderr)


# ---------------------------------------------------------------------------------------------- the C ABI and the compiled kernels
ENTRIES = ("mcav_geom_consistency_workspace_bytes", "mcav_geom_consistency_fwd", "mcav_geom_consistency_bwd")


def test_library_exports_and_header_declares_the_entries():
    lib_path = os.path.join(PKG, "mcav", "libmcav_depth.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    handle = ctypes.CDLL(lib_path)
    text = open(os.path.join(REPO, "include", "mcav_depth.h")).read()
    import losses  # noqa: F401  (registers the signatures)
    import mcav.lib as L
    for name in ENTRIES:
        assert hasattr(handle, name), name
        assert name + "(" in text, name
        assert name in L._SIGNATURES, name
    handle.mcav_geom_consistency_workspace_bytes.restype = ctypes.c_size_t
    assert handle.mcav_geom_consistency_workspace_bytes(12, 192, 640) >= 24 * 12 * 192 * 640
    for bad in ((0, 192, 640), (2, 1, 640), (2, 192, 1), (2, 4097, 4096), (4096, 8, 8)):
        assert handle.mcav_geom_consistency_workspace_bytes(*bad) == 0, bad


def test_entries_reject_bad_arguments_without_a_device():
    """Every rejection happens before anything touches the device: null pointers, unknown flag bits, non-positive sizes, H < 2, W < 2,
    H W > 2^24, a negative min_valid, a small workspace."""
    import losses  # noqa: F401
    import mcav.lib as L
    h = L.lib()
    fake = ctypes.c_void_p(0x1000)            # never dereferenced: the checks fail first
    ok = dict(B=2, H=8, W=16, flags=1, min_valid=100)

    def fwd(ws_bytes=1 << 30, null=None, **kw):
        a = dict(ok, **kw)
        p = [None if null == i else fake for i in range(7)]
        return h.mcav_geom_consistency_fwd(p[0], p[1], p[2], p[3], a["B"], a["H"], a["W"], a["flags"], a["min_valid"], 0.5, p[4], p[5],
                                           fake, p[6], ws_bytes, None)

    def bwd(ws_bytes=1 << 30, null=None, **kw):
        a = dict(ok, **kw)
        p = [None if null == i else fake for i in range(9)]
        return h.mcav_geom_consistency_bwd(p[0], p[1], p[2], p[3], a["B"], a["H"], a["W"], a["flags"], a["min_valid"], 0.5, p[4], fake,
                                           p[5], p[6], p[7], 0, p[8], ws_bytes, None)
    for kw in (dict(B=0), dict(B=4096), dict(H=1), dict(W=1), dict(H=-3), dict(H=4097, W=4096), dict(flags=2), dict(flags=16),
               dict(flags=1 << 31), dict(min_valid=-1)):
        assert fwd(**kw) == -1, kw
        assert bwd(**kw) == -1, kw
    for i in range(7):
        assert fwd(null=i) == -1, i
    for i in range(9):
        assert bwd(null=i) == -1, i
    need = h.mcav_geom_consistency_workspace_bytes(2, 8, 16)
    assert fwd(ws_bytes=need - 1) == -2 and bwd(ws_bytes=need - 1) == -2


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import test_isa_handoff as T
    return T._device_functions(tmp_path_factory, "geom_consistency.hip")


def test_kernels_exist_without_scratch(kernels):
    for kern, count in (("geom_consistency_fwd_kernel", 1), ("geom_consistency_scatter_kernel", 2), ("geom_consistency_combine_kernel", 1)):
        names = [n for n in kernels if kern in n]
        assert len(names) == count, (kern, list(kernels))
        for n in names:
            assert not any(i.startswith("scratch_") for i in kernels[n]), n


def test_sums_are_integer_or_fixed_order(kernels):
    """No float atomics anywhere; the scatter adds 64-bit integers (global, and in LDS in the tile form); the forward's only atomic is
    the ticket."""
    for n, body in kernels.items():
        assert not any("atomic" in i and ("_f32" in i or "_f64" in i or "pk_" in i) for i in body), n
    for n in (n for n in kernels if "scatter_kernel" in n):
        assert any(i.startswith("global_atomic_add_x2") for i in kernels[n]), n
    tile = [n for n in kernels if "scatter_kernelILb1" in n]
    assert tile and any(i.startswith("ds_add_u64") or i.startswith("ds_add_rtn_u64") for i in kernels[tile[0]]), tile
    fwd = [n for n in kernels if "fwd_kernel" in n][0]
    atomics = [i for i in kernels[fwd] if "atomic" in i]
    assert atomics and all(i.startswith("global_atomic_add ") and " sc0" in i for i in atomics), atomics


def test_forward_keeps_the_ticket_hand_off(kernels):
    import test_isa_handoff as T
    fwd = {n: b for n, b in kernels.items() if "fwd_kernel" in n}
    T.test_stores_are_acknowledged_before_every_ticket(fwd)
    for name, body in fwd.items():
        first = next(i for i, ins in enumerate(body) if ins.startswith("global_atomic_add "))
        assert [i for i in body[:first] if i.startswith("global_store") and " sc1" in i], name      # the slab entry
        assert len([i for i in body[first:] if i.startswith("global_load") and " sc1" in i]) >= 2, name      # the finisher's reads
        assert not any(i.startswith(("buffer_wbl2", "buffer_inv")) for i in body), name
