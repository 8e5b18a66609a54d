"""CPU: the backwards from pillar voxels to the network's plane (include/mcav_depth.h: mcav_pillarize_bwd, mcav_pl_batch_project_bwd;
pseudo_lidar.pillarize_backward, project_batch_backward).  The restatement (tests/pl_bwd_ref.py) against float64 autograd through the stock
formulations within the bounds its docstring derives; the header csrc/pl_bwd_math.h compiled for the host against the restatement bit for
bit on the cases the GPU tests run (tests/pl_bwd_cases.py), once more as a stand-alone program under the address and undefined-behaviour
sanitizers; the adjoint window against brute force; what the Python side refuses without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import pillar_ref as PR
import pl_batch_ref as R
import pl_bwd_cases as C
import pl_bwd_ref as BR
from conftest import PKG, REPO
from pfn_bwd_ref import sum_bound

SRC = os.path.join(REPO, "tests", "pl_bwd_hostcheck", "pl_bwd_hostcheck.cpp")
F = np.float32


# ---------------------------------------------------------------------------------------------- restatement vs float64 autograd
ILL = "odd-negatives"                                          # the one case whose plane keeps negative disparities


def plane_against_autograd(case):
    a, fwd, ref = C.project_build(case), C.project_forward(case), C.project_reference(case)
    C.project_non_trivial(case)
    n = len(fwd["pixels"])
    want = BR.project_autograd(C.project_upstream(case)[:n], fwd, **a)
    err = np.abs(ref["d_m"].astype(np.float64) - want)
    assert (ref["d_m"][ref["abs_terms"] == 0].view(np.uint32) == 0).all()                  # +0.0 where nothing arrives
    return a, ref, want, err


@pytest.mark.parametrize("case", [c for c in C.PROJECT_CASES if c != ILL])
def test_plane_restatement_matches_float64_autograd(case):
    """every element of d_m within the derived constant bound, which never exceeds 2^-20 sum |terms|: 8 x 2^-24 of it"""
    a, ref, want, err = plane_against_autograd(case)
    assert (a["m"] > 0).all() and ref["kappa"].max() <= 1.0, ref["kappa"].max()            # what the constant rests on
    bound = BR.plane_bound(want, ref)
    print("%s: largest error / bound %.3f, largest kappa %.3f" % (case, (err / np.maximum(bound, 1e-300)).max(), ref["kappa"].max()))
    assert (err <= bound).all(), (case, (err - bound).max())
    assert (bound <= 8.0 * 2.0 ** -24 * ref["abs_terms"] * (1 + 2.0 ** -15)).all()
    assert (bound <= 2.0 ** -20 * ref["abs_terms"]).all()


def test_ill_conditioned_demonstration_beside_the_bound():
    """NOT the required bound: the scene's negative disparities kept.  Their resized neighbours land just in front of the camera with
    10 v + 0.01 nearly cancelled; the constant bound is not claimed there, the kappa-weighted one holds, and every pixel with kappa > 1
    blends a negative entry.  (The kernels are held bit for bit on this case like on any other.)"""
    a, ref, want, err = plane_against_autograd(ILL)
    kap = ref["kappa"]
    hot = np.argwhere(kap > 1.0)
    print("%s: %d pixels with kappa > 1, largest %.1f" % (ILL, len(hot), kap.max()))
    assert len(hot) >= 10 and kap.max() > 10.0
    h, w = a["m"].shape[1:]
    for b, r, c in hot:
        Hb, Wb = a["sizes"][b]
        (y0, y1, _), (x0, x1, _) = R.axis_taps(h, Hb), R.axis_taps(w, Wb)
        assert a["m"][b][[y0[r], y0[r], y1[r], y1[r]], [x0[c], x1[c], x0[c], x1[c]]].min() < 0, (b, r, c)
    assert (err <= BR.plane_bound_conditioned(want, ref)).all()


@pytest.mark.parametrize("case", C.PILLAR_CASES)
def test_pillar_restatement_matches_float64_autograd(case):
    a, fwd, ref = C.pillar_build(case), C.pillar_forward(case), C.pillar_reference(case)
    C.pillar_non_trivial(case)
    g = C.pillar_upstream(case)
    P = len(fwd["coords"])
    cen = np.stack([PR.centre(fwd["coords"][:, 3], a["grid"].x0, a["grid"].vx), PR.centre(fwd["coords"][:, 2], a["grid"].y0, a["grid"].vy)],
                   axis=1).astype(np.float64)
    want = BR.pillar_autograd(a["points"], fwd["slot_points"], fwd["num_points"], cen, g[:P], g.shape[2])
    err = np.abs(ref["d_points"].astype(np.float64) - want)
    assert (err <= sum_bound(want, ref["abs_terms"])).all(), err.max()
    np.testing.assert_allclose(ref["d_points64"], want, rtol=0, atol=2.0 ** -40 * max(ref["abs_terms"].max(), 1.0))
    if a["decorate"]:                                              # the mean's derivative is there: a plain pass-through differs
        held = fwd["slot_points"][fwd["slot_points"] >= 0]
        plain = g[:P][fwd["slot_points"] >= 0]
        assert not np.array_equal(ref["d_points"][held, 0], (plain[:, 0] + plain[:, 4] + plain[:, 7]).astype(F))


def test_provenance_restates_the_forwards():
    """pl_bwd_ref's forwards with the selection kept give pl_batch_ref's and pillar_ref's results, and the selection reproduces them"""
    import pl_batch_cases as PC
    for case in ("odd-dense", "odd-sparse3", "odd-beams8x16", "direct-depth"):
        a = C.project_build(case)
        fwd = C.project_forward(case)
        kw = {k: v for k, v in a.items() if k not in ("scales", "capacity")}
        cloud, offsets = R.project_batch(**kw)
        C.same_bits(fwd["cloud"], cloud)
        assert np.array_equal(fwd["offsets"], offsets)
        for b, (Hb, Wb) in enumerate(a["sizes"]):                   # the recorded pixel gives the row back
            rows = np.flatnonzero(fwd["image"] == b)
            d = R.depth_image(a["m"][b], Hb, Wb, a["input"], a["scale"])
            q = R.points(d, a["P"][b], a["T"][b]).astype(F)
            px = fwd["pixels"][rows]
            C.same_bits(np.ascontiguousarray(q[px // a["Wg"], px % a["Wg"]]), np.ascontiguousarray(cloud[rows, :3]))
            assert len(np.unique(px)) == len(px)                    # a pixel owns at most one row
    for case in C.PILLAR_CASES:
        a, fwd = C.pillar_build(case), C.pillar_forward(case)
        sp = fwd["slot_points"]
        assert ((sp >= 0).sum(axis=1) == fwd["num_points"]).all()
        C.same_bits(np.where((sp >= 0)[:, :, None], a["points"][np.maximum(sp, 0)], F(0)), np.ascontiguousarray(fwd["voxels"][:, :, :4]))
        held = sp[sp >= 0]
        assert len(np.unique(held)) == len(held)                    # a row is in at most one slot


# ---------------------------------------------------------------------------------------------- csrc/pl_bwd_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pl_bwd_hostcheck") / "libpl_bwd_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.pl_bwd_pillars_host.argtypes = [p, p, p, p, i, ll, i, i, p, ll]
    lib.pl_bwd_plane_host.argtypes = [p, ll, p, p, p, i, i, i, i, i, p, p, ctypes.c_float, p, i, p, p]
    lib.pl_bwd_window_host.argtypes = [i, i, i, p, p]
    lib.pl_bwd_taps_host.argtypes = [i, i, i, p, p, p]
    lib.pl_bwd_window_host.restype = lib.pl_bwd_taps_host.restype = None
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def calib_records(a):
    B = a["m"].shape[0]
    P, T = np.broadcast_to(np.asarray(a["P"], np.float64), (B, 3, 4)), np.broadcast_to(np.asarray(a["T"], np.float64), (B, 4, 4))
    return np.ascontiguousarray(np.concatenate([P.reshape(B, 12), T.reshape(B, 16)], axis=1))


def plane_arrays(case):
    """the buffers of a projection case as the C call takes them: pixels padded with a sentinel that would be refused if read"""
    a, fwd = C.project_build(case), C.project_forward(case)
    cap, n = C.project_capacity(case), len(fwd["pixels"])
    pixels = np.full(cap, -12345, np.int32)
    pixels[:n] = fwd["pixels"]
    return dict(d_points=np.ascontiguousarray(C.project_upstream(case)), pixels=pixels, offsets=np.ascontiguousarray(fwd["offsets"]),
                m=np.ascontiguousarray(a["m"]), sizes=np.ascontiguousarray(np.asarray(a["sizes"], np.int32)), calib=calib_records(a),
                scales=None if a["scales"] is None else np.ascontiguousarray(a["scales"]), capacity=cap,
                flags=1 if a["input"] == "depth" else 0)


def plane_run(host, case, **kw):
    a = C.project_build(case)
    B, h, w = a["m"].shape
    arr = plane_arrays(case)
    d_m, G = np.full((B, h, w), -7.0, F), np.full((B, a["Hg"], a["Wg"]), -7.0, F)
    arg = dict(d_points=ptr(arr["d_points"]), capacity=arr["capacity"], pixels=ptr(arr["pixels"]), offsets=ptr(arr["offsets"]), m=ptr(arr["m"]),
               B=B, h=h, w=w, Hg=a["Hg"], Wg=a["Wg"], sizes=ptr(arr["sizes"]), calib=ptr(arr["calib"]), scale=float(a["scale"]),
               scales=ptr(arr["scales"]), flags=arr["flags"], d_m=ptr(d_m), G=ptr(G))
    arg.update(kw)
    rc = host.pl_bwd_plane_host(*[arg[k] for k in ("d_points", "capacity", "pixels", "offsets", "m", "B", "h", "w", "Hg", "Wg", "sizes", "calib",
                                                   "scale", "scales", "flags", "d_m", "G")])
    return rc, d_m, G


@pytest.mark.parametrize("case", C.PROJECT_CASES)
def test_header_plane_matches_restatement(host, case):
    ref = C.project_reference(case)
    rc, d_m, G = plane_run(host, case)
    assert rc == 0
    C.same_bits(G, ref["G"])
    C.same_bits(d_m, ref["d_m"])


def pillar_arrays(case):
    a, fwd = C.pillar_build(case), C.pillar_forward(case)
    cap, P, N = C.pillar_capacity(case), len(fwd["coords"]), a["max_points"]
    slots, num = np.full((cap, N), 1 << 30, np.int32), np.full(cap, 1 << 20, np.int32)
    slots[:P], num[:P] = fwd["slot_points"], fwd["num_points"]
    return dict(d_voxels=np.ascontiguousarray(C.pillar_upstream(case)), slot_points=slots, num_points=num,
                offsets=np.ascontiguousarray(fwd["offsets"]), capacity=cap, N=N, C=9 if a["decorate"] else 4, n_max=len(a["points"]))


def pillar_run(host, case, **kw):
    arr = pillar_arrays(case)
    out = np.full((arr["n_max"], 4), -7.0, F)
    arg = dict(d_voxels=ptr(arr["d_voxels"]), slot_points=ptr(arr["slot_points"]), num_points=ptr(arr["num_points"]), offsets=ptr(arr["offsets"]),
               B=3, capacity=arr["capacity"], N=arr["N"], C=arr["C"], d_points=ptr(out), n_max=arr["n_max"])
    arg.update(kw)
    rc = host.pl_bwd_pillars_host(*[arg[k] for k in ("d_voxels", "slot_points", "num_points", "offsets", "B", "capacity", "N", "C", "d_points",
                                                     "n_max")])
    return rc, out


@pytest.mark.parametrize("case", C.PILLAR_CASES)
def test_header_pillars_match_restatement(host, case):
    rc, out = pillar_run(host, case)
    assert rc == 0
    C.same_bits(out, C.pillar_reference(case)["d_points"])


def test_header_refusals(host):
    assert plane_run(host, "odd-dense")[0] == 0 and pillar_run(host, "decorated")[0] == 0
    for kw in (dict(d_points=None), dict(pixels=None), dict(offsets=None), dict(m=None), dict(sizes=None), dict(calib=None), dict(d_m=None),
               dict(B=0), dict(h=0), dict(w=0), dict(Hg=0), dict(Wg=0), dict(flags=2), dict(scale=float("nan")), dict(Hg=1 << 16, Wg=1 << 16)):
        rc, d_m, G = plane_run(host, "odd-dense", **kw)
        assert rc == -1 and (d_m == -7).all() and (G == -7).all(), kw
    for kw in (dict(d_voxels=None), dict(slot_points=None), dict(num_points=None), dict(offsets=None), dict(d_points=None), dict(B=0),
               dict(B=65536), dict(capacity=-1), dict(N=0), dict(N=65), dict(C=5), dict(n_max=-1)):
        rc, out = pillar_run(host, "decorated", **kw)
        assert rc == -1 and (out == -7).all(), kw


def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined: the decorated pillars with a cut capacity and the
    odd shapes with the scale table, the beam grid and the cut cloud, every buffer exactly as large as the call may touch: a finding ends
    the program with a non-zero status."""
    exe = str(tmp_path / "pl_bwd_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPL_BWD_STANDALONE"]) +
                          ["-o", exe])
    for pcase, case in (("decorated-capacity", "odd-scales"), ("plain", "odd-beams8x16"), ("decorated", "odd-capacity"), ("plain", "direct-dense")):
        a, pa, arr = C.project_build(case), pillar_arrays(pcase), plane_arrays(case)
        B, h, w = a["m"].shape
        assert B == 3 or case.startswith("direct")
        if B != 3:                                                  # one header carries B for both halves: pad the pillars' table
            pa["offsets"] = np.ascontiguousarray(pa["offsets"][[0, 3]])
        head = np.array([B, pa["capacity"], pa["N"], pa["C"], pa["n_max"], arr["capacity"], h, w, a["Hg"], a["Wg"], arr["flags"],
                         arr["scales"] is not None, 0, 0, 0, 0], np.int64)
        parts = [head, np.array([a["scale"]], F), pa["offsets"], pa["num_points"], pa["slot_points"], pa["d_voxels"], arr["offsets"],
                 arr["pixels"], arr["sizes"], arr["calib"]] + ([arr["scales"]] if arr["scales"] is not None else []) + [arr["m"], arr["d_points"]]
        with open(str(tmp_path / "in.bin"), "wb") as f:
            for part in parts:
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        raw = open(str(tmp_path / "out.bin"), "rb").read()
        assert np.frombuffer(raw, np.int32, 2).tolist() == [0, 0]
        d_points = np.frombuffer(raw, F, pa["n_max"] * 4, 8).reshape(-1, 4)
        d_m = np.frombuffer(raw, F, B * h * w, 8 + d_points.nbytes).reshape(B, h, w)
        assert 8 + d_points.nbytes + d_m.nbytes == len(raw)
        if B == 3:
            C.same_bits(d_points, C.pillar_reference(pcase)["d_points"])
        C.same_bits(d_m, C.project_reference(case)["d_m"])


# ---------------------------------------------------------------------------------------------- the adjoint window
def axis_pairs():
    pairs = {(192, 375), (640, 1242), (5, 5), (1, 7), (7, 3)}
    for case in C.PROJECT_CASES:
        a = C.project_build(case)
        h, w = a["m"].shape[1:]
        for Hb, Wb in a["sizes"]:
            pairs |= {(h, Hb), (w, Wb)}
    return sorted(pairs)


@pytest.mark.parametrize("n_in,n_out", axis_pairs())
def test_adjoint_window_is_exactly_the_outputs_that_touch(host, n_in, n_out):
    i0, i1 = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64)
    a, b, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    for o in range(n_out):
        host.pl_bwd_taps_host(o, n_in, n_out, ctypes.byref(a), ctypes.byref(b), ctypes.byref(l))
        i0[o], i1[o] = a.value, b.value
    r0, r1, _ = R.axis_taps(n_in, n_out)
    assert np.array_equal(i0, r0) and np.array_equal(i1, r1)        # the restatement's taps are the header's
    assert (np.diff(i0) >= 0).all()                                  # what the bisection rests on
    seen = 0
    for i in range(n_in):
        host.pl_bwd_window_host(i, n_in, n_out, ctypes.byref(a), ctypes.byref(b))
        touch = np.flatnonzero((i0 == i) | (i1 == i))
        assert touch.tolist() == list(range(a.value, b.value + 1)), (i, a.value, b.value, touch.tolist())
        seen += len(touch)
    assert seen >= n_out
    if n_in != n_out:
        W = BR.tap_weights(n_in, n_out)
        assert ((W != 0) <= ((i0[:, None] == np.arange(n_in)) | (i1[:, None] == np.arange(n_in)))).all()
        assert np.abs(W.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -23


# ---------------------------------------------------------------------------------------------- the Python side without a GPU
def test_new_entries_are_exported_and_bound():
    import mcav.lib as L
    import pseudo_lidar  # noqa: F401
    names = ["mcav_pl_batch_project_indexed", "mcav_pl_batch_project_bwd", "mcav_pl_batch_project_bwd_workspace_bytes",
             "mcav_pillarize_indexed", "mcav_pillarize_bwd"]
    header = open(os.path.join(REPO, "include", "mcav_depth.h")).read()
    hl = L.lib()
    for n in names:
        assert n in L._SIGNATURES and n + "(" in header and hasattr(hl, n), n
    assert hl.mcav_pl_batch_project_bwd_workspace_bytes(3, 23, 37) == -(-4 * 3 * 23 * 37 // 256) * 256
    assert hl.mcav_pl_batch_project_bwd_workspace_bytes(0, 23, 37) == 0 and hl.mcav_pl_batch_project_bwd_workspace_bytes(1 << 10, 1 << 11, 1 << 11) == 0
    # refused before anything is launched: no GPU is touched
    assert hl.mcav_pl_batch_project_bwd(None, 0, None, None, None, 1, 8, 8, 8, 8, None, None, 1.0, None, 0, None, None, 0, None) == -1
    assert hl.mcav_pillarize_bwd(None, None, None, None, 1, 1, 1, 0, None, 1, None) == -1


def test_python_side_refuses_without_a_gpu():
    import mcav.lib as L
    from pseudo_lidar import CloudBatch, PillarBatch, PseudoLiDAR, pillarize, pillarize_backward, project_batch_backward
    cloud = CloudBatch(2, 10, "cpu")
    assert cloud.pixels is None
    with pytest.raises(L.MCAVError, match="CloudBatch"):
        project_batch_backward(cloud.points, torch.zeros(10, 4))
    with pytest.raises(L.MCAVError, match="provenance"):
        project_batch_backward(cloud, torch.zeros(10, 4))
    pb = PillarBatch(2, 10, 5, 9, "cpu")
    assert pb.slot_points is None
    with pytest.raises(L.MCAVError, match="PillarBatch"):
        pillarize_backward(pb.voxels, torch.zeros(10, 5, 9))
    with pytest.raises(L.MCAVError, match="provenance"):
        pillarize_backward(pb, torch.zeros(10, 5, 9))
    pb.slot_points = torch.zeros(10, 5, dtype=torch.int32)
    pb._fwd = dict(slot_points=pb.slot_points, num_points=pb.num_points, offsets=pb.offsets, n_max=12, B=2, shape=(10, 5, 9))
    with pytest.raises(L.MCAVError, match=r"\[10, 5, 9\]"):
        pillarize_backward(pb, torch.zeros(10, 5, 4))
    with pytest.raises(L.MCAVError, match="GPU"):
        pillarize_backward(pb, torch.zeros(10, 5, 9))                                      # CPU buffers
    # a plane that requires a gradient is refused on the CPU like any other: there is no eager fall-back behind the autograd node
    pl = PseudoLiDAR.from_matrices(np.eye(4), np.eye(3, 4), 0)
    with pytest.raises(L.MCAVError, match="GPU"):
        pl.project_batch(torch.zeros(1, 8, 8, requires_grad=True))
    with pytest.raises(L.MCAVError, match="GPU"):
        pillarize(torch.zeros(10, 4, requires_grad=True), torch.zeros(3, dtype=torch.int32), provenance=True)
