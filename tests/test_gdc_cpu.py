"""CPU: the graph-based depth correction (include/mcav_depth.h: mcav_gdc_graph, mcav_gdc_solve; pseudo_lidar.gdc).  The float32 restatement
(tests/gdc_ref.py) against its float64 form; the closed-form weights against the general solve; the windowed KNN at full window against
brute force; the float64 conjugate gradient against the dense least-squares solution; what the correction buys on the scene; the header
csrc/gdc_math.h compiled for the host against the restatement, bit for bit, on the cases the GPU tests run (tests/gdc_cases.py), once more
as a stand-alone program under the address and undefined-behaviour sanitizers; select_beams; what the library and the Python side refuse
without a GPU.

Measured here (float32 restatement against float64 arithmetic on the same graph, largest |difference| in metres over all cases):
iters = 1: 6.8e-6, iters = 2: 1.2e-5, iters = 5: 3.4e-4 (the `holes` case; 5.9e-5 on the scene).  Weights, float32 against float64 on
the scene: 4.9e-7, no neighbour differs; the largest |w| is 0.77."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gdc_cases as C
import gdc_ref as R
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "gdc_hostcheck", "gdc_hostcheck.cpp")
LIB = os.path.join(PKG, "mcav", "libmcav_depth.so")
F = np.float32


# ---------------------------------------------------------------------------------------------- the definition against itself
@pytest.mark.parametrize("case", C.CASES)
def test_restatement_float32_matches_float64(case):
    """The same graph wherever the float64 distances do not tie or nearly tie.  Weights: w'_j = 1 - d_j t carries a few roundings (at most
    4 of 2^-24, |w'| <= ~1), and their sum m - s^2 / (lam + q) can be as small as m reg / (1 + reg) (all d_j equal: Cauchy-Schwarz is
    tight), so the sum's relative error, and with it every weight's, is at most 4 * 2^-24 * (1 + 1 / reg); twice that with the
    numerator's own roundings.  Measured: 1.05e-4 at worst (the `holes` case), 3.5e-5 on `r1`, 4.9e-7 on the scene; no row of any case differs."""
    C.check_non_trivial(case)
    a = C.build(case)
    n32, w32, f32 = C.graph32(case)
    n64, w64, f64 = C.graph64(case)
    assert np.array_equal(f32, f64)
    assert ((n32 >= 0) == (n64 >= 0)).all()
    same_row = (n32 == n64).all(-1)
    if case != "wall":                                       # exact ties are decided alike; near ties need not be
        assert same_row.mean() >= 0.97, same_row.mean()
    else:
        assert same_row.all()
    # where the graphs differ, the float64 distances of the two choices nearly tie: a float32 coordinate carries two roundings (quotient,
    # product: <= 2 * 2^-24 |X|), a coordinate difference three (<= 5 * 2^-24 Xmax), so d2 is off by at most 2 sqrt(3 d2) * 5 * 2^-24 Xmax
    # plus its own three roundings: below 32 * 2^-24 * Xmax * sqrt(d2) for each of the two candidates compared
    for b in range(len(n32)):
        x, y, z = (c.reshape(-1) for c in R.points(a["depth"][b], a["K"][b], np.float64))
        rows = np.flatnonzero(~same_row[b].reshape(-1))
        ok = R.valid_mask(a["depth"][b], a["params"]["min_depth"], a["params"]["max_depth"]).reshape(-1)
        xmax = max(np.abs(c[ok]).max() for c in (x, y, z))
        for i in rows:
            d2 = lambda j: (x[j] - x[i]) ** 2 + (y[j] - y[i]) ** 2 + (z[j] - z[i]) ** 2
            j32, j64 = n32[b].reshape(-1, n32.shape[-1])[i], n64[b].reshape(-1, n32.shape[-1])[i]
            for s in np.flatnonzero(j32 != j64):
                da, db = d2(j32[s]), d2(j64[s])
                assert abs(da - db) <= 2 * 32 * 2.0 ** -24 * xmax * np.sqrt(max(da, db)), (case, b, i, s, da, db)
    diff = np.abs(w32.astype(np.float64) - w64)[same_row]
    bound = 8 * 2.0 ** -24 * (1 + 1 / a["params"]["reg"]) * max(1.0, float(np.abs(w64).max()))
    print(case, "rows alike %.4f" % same_row.mean(), "weights differ by %.3g (bound %.3g)" % (diff.max(), bound))
    assert diff.max() <= bound
    assert np.abs(w32.sum(-1)[(f32 & 1) != 0] - 1).max() <= 16 * 2.0 ** -24 * max(1.0, float(np.abs(w32).max())) * a["params"]["k"]


@pytest.mark.parametrize("case", ["scene", "holes", "wall", "k16", "k1"])
def test_closed_form_weights_match_the_general_solve(case):
    a = C.build(case)
    nbr, _, fl = C.graph64(case)
    z = a["depth"].astype(np.float64)
    B, H, W, k = nbr.shape
    used = nbr >= 0
    zn = np.stack([z[b].reshape(-1)[np.where(used[b], nbr[b], 0)] for b in range(B)])
    d = np.where(used, zn - z[..., None], 0.0)
    rows = np.random.RandomState(3).choice(B * H * W, 200, replace=False)
    worst = R.check_closed_form(d, used, a["params"]["reg"], rows=rows, bound=1e-8)
    print(case, "closed form vs np.linalg.solve: %.3g" % worst)


def test_full_window_is_exact_knn():
    a = C.build("full")
    nbr, _, _ = C.graph32("full")
    for b in range(len(a["depth"])):
        brute = R.brute_force_knn(a["depth"][b], a["K"][b], a["params"]["k"])
        assert np.array_equal(brute, nbr[b])
    holes = C.build("holes")
    small = holes["depth"][0, 0:8, 8:16]
    got = R.graph_image(small, np.zeros_like(small), holes["K"][0], k=6, radius=7)[0]
    assert (got < 0).any() and np.array_equal(got, R.brute_force_knn(small, holes["K"][0], 6))


@pytest.mark.parametrize("case", ["scene", "full"])
def test_float64_conjugate_gradient_reaches_the_dense_solution(case):
    """(not on `holes`: its 2 x 2 island holds no known pixel, so the minimiser is not unique there -- lstsq returns the one of least
    norm, the iteration the one nearest its start; test_holes_reach_the_same_minimum compares the minima)"""
    a = C.build(case)
    dense = C.dense64(case)
    out, info = R.gdc(a["depth"], a["sparse"], a["K"], min_known=a["min_known"], iters=5000, tol=0.0, dtype=np.float64,
                      graph_of=C.graph32(case), **a["params"])
    ok = np.isfinite(dense)
    err = np.abs(out - dense)[ok].max()
    print(case, "float64 CG against lstsq: %.3g m after" % err, info[:, 2], "iterations")
    assert err <= 1e-8
    assert np.array_equal(np.isfinite(out), ok)


def test_holes_reach_the_same_minimum():
    a = C.build("holes")
    nbr, w, fl = C.graph32("holes")
    dense = C.dense64("holes")
    out, _ = R.gdc(a["depth"], a["sparse"], a["K"], iters=3000, tol=0.0, dtype=np.float64, graph_of=(nbr, w, fl), **a["params"])
    for b in range(2):
        op = R.Operator(nbr[b], w[b], fl[b], np.float64)
        cost = lambda z: R.dot64(op.forward(np.where(op.graph, z.reshape(-1), 0.0)))
        print("holes, image %d: |M z|^2 = %.12g (CG), %.12g (lstsq)" % (b, cost(out[b]), cost(dense[b])))
        assert abs(cost(out[b]) - cost(dense[b])) <= 1e-9 * cost(dense[b])


def test_the_correction_pays_on_the_scene():
    a = C.build("scene")
    dense = C.dense64("scene")
    t = a["truth"].astype(np.float64)
    before = np.mean(np.abs(a["depth"] - t) / t, axis=(1, 2))
    after = np.mean(np.abs(dense - t) / t, axis=(1, 2))
    print("mean relative error", before, "->", after)
    assert (after <= before / 5).all()
    known = (C.graph32("scene")[2] & 3) == 3
    assert np.array_equal(dense[known], a["sparse"][known].astype(np.float64))


def test_solver_leaves_the_rest_alone():
    """off the graph the input's bits, known graph pixels their sparse value, a passed-through image its input and (.., .., 0, 1)"""
    for case in ("holes", "mixed"):
        a = C.build(case)
        _, _, fl = C.graph32(case)
        for iters in (0, 5):
            out, info = C.solved32(case, iters)
            off = (fl & 1) == 0
            assert np.array_equal(out[off].view(np.uint32), a["depth"][off].view(np.uint32))
            known = (fl & 3) == 3
            for b in range(len(out)):
                if info[b, 1] >= a["min_known"]:
                    assert np.array_equal(out[b][known[b]].view(np.uint32), a["sparse"][b][known[b]].view(np.uint32))
                    assert info[b, 2] == iters
                else:
                    assert np.array_equal(out[b].view(np.uint32), a["depth"][b].view(np.uint32)) and info[b, 2:].tolist() == [0, 1]
    assert C.solved32("mixed", 5)[1][:, 1].tolist() == [80, 0, 2]


# ---------------------------------------------------------------------------------------------- csrc/gdc_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gdc_hostcheck") / "libgdc_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.gdc_host_graph.argtypes = [p, p, p, i, i, i, i, i, f, f, f, p, p, p]
    lib.gdc_host_params_ok.argtypes = [i, i, f, f, f]
    return lib


def same_graph(got, want):
    for g, w_, dt in zip(got, want, (np.int32, np.uint32, np.uint8)):
        assert g.shape == w_.shape
        assert np.array_equal(np.ascontiguousarray(g).view(dt), np.ascontiguousarray(w_).view(dt))


@pytest.mark.parametrize("case", C.CASES)
def test_header_matches_restatement(host, case):
    a = C.build(case)
    p = a["params"]
    B, H, W = a["depth"].shape
    nbr, w, fl = np.full((B, H, W, p["k"]), -7, np.int32), np.full((B, H, W, p["k"]), -7.0, F), np.full((B, H, W), 77, np.uint8)
    rc = host.gdc_host_graph(a["depth"].ctypes.data, a["sparse"].ctypes.data, a["K"].ctypes.data, B, H, W, p["k"], p["radius"], p["reg"],
                             p["min_depth"], p["max_depth"], nbr.ctypes.data, w.ctypes.data, fl.ctypes.data)
    assert rc == 0
    same_graph((nbr, w, fl), C.graph32(case))


def test_header_parameter_checks(host):
    ok = lambda **kw: host.gdc_host_params_ok(*[dict(dict(k=10, radius=3, reg=1e-3, min_depth=1e-3, max_depth=80.0), **kw)[n]
                                                for n in ("k", "radius", "reg", "min_depth", "max_depth")])
    assert ok() == 1 and ok(k=1) == 1 and ok(k=16, radius=7) == 1 and ok(min_depth=0.0) == 1
    for kw in (dict(k=0), dict(k=17), dict(radius=0), dict(radius=8), dict(reg=0.0), dict(reg=-1.0), dict(reg=float("nan")),
               dict(reg=float("inf")), dict(min_depth=-1.0), dict(max_depth=1e-3), dict(max_depth=float("nan")), dict(min_depth=float("nan"))):
        assert ok(**kw) == 0, kw


def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the case with holes, clipped windows, short
    rows and isolated pixels, and on the full-window case: a finding ends the program with a non-zero status."""
    exe = str(tmp_path / "gdc_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGDC_STANDALONE"]) +
                          ["-o", exe])
    for case in (C.HARDEST, "full", "k16"):
        a = C.build(case)
        p = a["params"]
        B, H, W = a["depth"].shape
        with open(str(tmp_path / "in.bin"), "wb") as f:
            for part in (np.array([B, H, W, p["k"], p["radius"]], np.int32), np.array([p["reg"], p["min_depth"], p["max_depth"]], F),
                         a["depth"], a["sparse"], a["K"]):
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        raw = open(str(tmp_path / "out.bin"), "rb").read()
        n = B * H * W
        assert len(raw) == 4 + 8 * n * p["k"] + n and np.frombuffer(raw, np.int32, 1)[0] == 0
        nbr = np.frombuffer(raw, np.int32, n * p["k"], 4).reshape(B, H, W, p["k"])
        w = np.frombuffer(raw, F, n * p["k"], 4 + 4 * n * p["k"]).reshape(B, H, W, p["k"])
        fl = np.frombuffer(raw, np.uint8, n, 4 + 8 * n * p["k"]).reshape(B, H, W)
        same_graph((nbr, w, fl), C.graph32(case))


# ---------------------------------------------------------------------------------------------- select_beams
def test_select_beams_on_a_hand_made_scan():
    from geometry.velodyne import select_beams
    import mcav.lib as L
    elev = np.array([-24.9, -24.0, -12.0, 0.0, 1.99, 2.0, 5.0, -30.0, 0.2])          # degrees; 4 bins of 6.725 from -24.9
    r = 10.0
    pts = np.stack([r * np.cos(np.radians(elev)), np.zeros(len(elev)), r * np.sin(np.radians(elev)), np.arange(len(elev))], axis=1).astype(F)
    pts = np.concatenate([pts, np.array([[np.nan, 0, 0, 9], [0, 0, 0, 10]], F)])      # a NaN row; the origin has elevation 0
    e64 = np.degrees(np.arctan2(pts[:, 2].astype(np.float64), np.hypot(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))))
    want_bin = np.floor((e64 - -24.9) / 26.9 * 4)
    got = select_beams(pts, keep=[0, 3], of=4, fov=(-24.9, 2.0))
    keep = np.isin(want_bin, [0, 3])
    assert np.array_equal(got.view(np.uint32), pts[keep].view(np.uint32))
    ids = got[:, 3].tolist()
    assert all(float(i) in ids for i in (1, 3, 4, 8, 10)) and not any(float(i) in ids for i in (2, 6, 7, 9)) and ids == sorted(ids)
    assert select_beams(pts, keep=[], of=4).shape == (0, 4)
    every = select_beams(pts, keep=range(64))
    assert every[:, 3].tolist() == [float(i) for i in range(len(pts)) if 0 <= np.floor((e64[i] + 24.9) / 26.9 * 64) < 64]
    assert np.array_equal(select_beams(pts, keep=[1, 1, 2], of=4), select_beams(pts, keep=(2, 1), of=4))
    for kw in (dict(keep=[4], of=4), dict(keep=[-1]), dict(keep=[0], of=0), dict(keep=[0], fov=(2.0, -24.9))):
        with pytest.raises(L.MCAVError):
            select_beams(pts, **kw)
    with pytest.raises(L.MCAVError):
        select_beams(np.zeros((3, 2), F), keep=[0])


# ---------------------------------------------------------------------------------------------- the library and the Python side without a GPU
def test_abi_refuses_bad_arguments():
    """argument checks come before any launch: with pointers that are never followed"""
    if not os.path.exists(LIB):                              # as tests/test_abi_symbols.py
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(LIB)
    p, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    lib.mcav_gdc_workspace_bytes.restype = sz
    lib.mcav_gdc_workspace_bytes.argtypes = [i] * 5
    lib.mcav_gdc_graph.argtypes = [p] * 3 + [i] * 5 + [f] * 3 + [p] * 4 + [sz, p]
    lib.mcav_gdc_solve.argtypes = [p] * 5 + [i] * 7 + [f] + [p] * 3 + [sz, p]
    need = lib.mcav_gdc_workspace_bytes(2, 24, 40, 10, 3)
    n, G = 2 * 24 * 40, 4
    assert need >= (8 * 10 + 12) * n + 4 * 2 * G * 256 + 12 * 2 * G + 44 * 2 and need % 256 == 0
    for bad in ((0, 24, 40, 10, 3), (2, 0, 40, 10, 3), (2, 24, 40, 0, 3), (2, 24, 40, 17, 3), (2, 24, 40, 10, 0), (2, 24, 40, 10, 8),
                (70000, 24, 40, 10, 3), (1, 4097, 4096, 10, 3), (40, 4096, 4096, 16, 3)):
        assert lib.mcav_gdc_workspace_bytes(*bad) == 0, bad
    A = 4096                                                 # a non-null, aligned address that is never read
    graph = lambda **kw: lib.mcav_gdc_graph(*[dict(dict(depth=A, sparse=A, K=A, B=2, H=24, W=40, k=10, radius=3, reg=1e-3, lo=1e-3, hi=80.0,
                                                             nbr=A, w=A, fl=A, ws=A, nbytes=need, stream=None), **kw)[n_]
                                              for n_ in ("depth", "sparse", "K", "B", "H", "W", "k", "radius", "reg", "lo", "hi", "nbr", "w",
                                                         "fl", "ws", "nbytes", "stream")])
    solve = lambda **kw: lib.mcav_gdc_solve(*[dict(dict(depth=A, sparse=2 * A, nbr=A, w=A, fl=A, B=2, H=24, W=40, k=10, radius=3, mk=1, iters=5,
                                                             tol=1e-4, out=3 * A, info=A, ws=A, nbytes=need, stream=None), **kw)[n_]
                                              for n_ in ("depth", "sparse", "nbr", "w", "fl", "B", "H", "W", "k", "radius", "mk", "iters",
                                                         "tol", "out", "info", "ws", "nbytes", "stream")])
    for kw in (dict(depth=None), dict(sparse=None), dict(K=None), dict(nbr=None), dict(w=None), dict(fl=None), dict(ws=None), dict(B=0),
               dict(H=0), dict(W=-1), dict(k=0), dict(k=17), dict(radius=0), dict(radius=8), dict(reg=0.0), dict(reg=float("nan")),
               dict(lo=-1.0), dict(hi=1e-3), dict(hi=float("nan"))):
        assert graph(**kw) == -1, kw
    assert graph(nbytes=need - 1) == -2
    for kw in (dict(depth=None), dict(sparse=None), dict(nbr=None), dict(w=None), dict(fl=None), dict(out=None), dict(info=None),
               dict(ws=None), dict(B=0), dict(k=17), dict(radius=8), dict(iters=-1), dict(tol=-1.0), dict(tol=float("nan")), dict(out=A),
               dict(out=2 * A), dict(ws=A + 4)):
        assert solve(**kw) == -1, kw
    assert solve(nbytes=need - 1) == -2


def test_gdc_refuses_bad_arguments_without_a_gpu():
    import torch
    import mcav.lib as L
    from pseudo_lidar import GDCResult, gdc
    from pseudo_lidar.PseudoLiDAR import grid_intrinsics
    d = torch.ones(2, 8, 8)
    for kw in (dict(depth=d, sparse=d, K=[1, 1, 1, 1]),                                 # CPU tensors
               dict(depth=np.ones((2, 8, 8), F), sparse=d, K=[1, 1, 1, 1]),
               dict(depth=torch.ones(8, 8), sparse=torch.ones(8, 8), K=[1, 1, 1, 1])):
        with pytest.raises(L.MCAVError):
            gdc(**kw)
    assert callable(GDCResult)
    P = np.array([[700.0, 0, 600.0, 40.0], [0, 710.0, 180.0, 2.0], [0, 0, 1, 0.003]])
    K = grid_intrinsics(P, [(370, 1226), (375, 1242)], 192, 640)
    assert K.dtype == F and K.shape == (2, 4)
    assert np.allclose(K[1], [700.0 * 640 / 1242, 710.0 * 192 / 375, 600.0 * 640 / 1242, 180.0 * 192 / 375], rtol=1e-6)


def test_inference_gdc_flags():
    import inference
    base = ["--config", "c.yaml", "--checkpoint", "x.pth", "--out", "o"]
    parse = lambda argv: inference.gdc_arguments(inference.build_parser().parse_args(argv))
    assert parse(base) is None
    assert parse(base + ["--gdc"]) == dict(beams=(5, 7, 9, 11), iters=400, k=10, radius=3)
    assert parse(base + ["--gdc", "--gdc-beams", "1", "2", "--gdc-iters", "50", "--gdc-k", "4", "--gdc-radius", "2"]) == \
        dict(beams=(1, 2), iters=50, k=4, radius=2)
