"""CPU: the batch pseudo-LiDAR projection (include/mcav_depth.h: mcav_pl_batch_project, PseudoLiDAR.project_batch).  The restatement
(tests/pl_batch_ref.py) against the reference's golden clouds and against torch's resize; the headers csrc/pl_math.h and csrc/eval_math.h
compiled for the host against the restatement, bit for bit, on the cases the GPU tests run (tests/pl_batch_cases.py), once more as a
stand-alone program under the address and undefined-behaviour sanitizers; properties of the restatement; the loader's
datasets.calibration."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pl_batch_cases as C
import pl_batch_ref as R
from conftest import GOLDEN, PKG, REPO

SRC = os.path.join(REPO, "tests", "pl_batch_hostcheck", "pl_batch_hostcheck.cpp")


def bits_equal(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- restatement vs the reference
def test_restatement_matches_reference_golden():
    """input="depth", equal sizes, B = 1 on the golden matrices and depths: the rows are float32(golden cloud[:, :3]) in the same order, the
    plain cloud and every k-th survivor.  The golden was computed with a matmul; where a float64 coordinate differs from it by an ulp the
    float32 values may differ by one float32 ulp -- the test prints how many rows needed that."""
    g = np.load(os.path.join(GOLDEN, "pseudo_lidar.npz"))
    loose = 0
    for name in "abc":
        cloud, offsets = R.project_batch(g["depth_" + name][None], P=g["P_" + name], T=g["T"], input="depth",
                                         sparsity=int(g["sparsity_" + name]))
        want = g["cloud_" + name][:, :3].astype(np.float32)
        assert offsets.tolist() == [0, len(want)] and cloud.shape == (len(want), 4)
        assert not cloud[:, 3].any()
        ulp = np.abs(cloud[:, :3].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (name, ulp.max())
        loose += int((ulp.max(axis=1) > 0).sum())
    print("rows compared to 1 float32 ulp instead of bit for bit: %d" % loose)


@pytest.mark.parametrize("h,w,H,W", [(8, 13, 23, 37), (8, 13, 20, 33), (24, 40, 375, 400), (192, 640, 375, 1242), (7, 9, 7, 9)])
def test_resize_is_the_protocols_upsample(h, w, H, W):
    """pl_batch_ref.resize restates csrc/eval_math.h bilinear_sample, which test_eval_depth_cpu pins to torch's resize within 2 ulps"""
    from eval_protocol_ref import upsample
    disp = np.random.RandomState(h + W).rand(h, w).astype(np.float32)
    got, want = R.resize(disp, H, W), upsample(disp, H, W)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp.max() <= 2, ulp.max()
    if (h, w) == (H, W):
        assert np.array_equal(got, disp)


def test_fma32_rounds_once():
    """against exact rational arithmetic, on products whose float64 sum is a double-rounding trap"""
    from fractions import Fraction
    rng = np.random.RandomState(3)
    a = rng.rand(4000).astype(np.float32)
    b = rng.rand(4000).astype(np.float32)
    c = (rng.rand(4000) * 10.0 ** rng.randint(-8, 1, 4000)).astype(np.float32)
    a[:3], b[:3], c[:3] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32([2.0 ** -30, -2.0 ** -60, 2.0 ** -47])
    got = R.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                    # float(Fraction) rounds once to float64; settle the float32 neighbours exactly
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])


def test_fixture_holds_every_kind_of_pixel():
    for case in ("odd-maxdepth", "chunks-maxdepth", "direct-maxdepth"):
        a = C.build(case)
        for b, (Hb, Wb) in enumerate(a["sizes"]):
            assert np.isnan(a["m"][b]).sum() == 1 and np.isposinf(a["m"][b]).sum() == 1
            d = R.depth_image(a["m"][b], Hb, Wb, a["input"], a["scale"])
            q = R.points(d, a["P"][b], a["T"][b])
            with np.errstate(invalid="ignore"):
                assert (d > a["max_depth"]).any() and (q[..., 2] >= 1.0).any() and (q[..., 0] < 0).any()
    for case in C.CASES:
        C.check_non_trivial(case)


# ---------------------------------------------------------------------------------------------- csrc/pl_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pl_batch_hostcheck") / "libpl_batch_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.plb_host_project.argtypes = [p, i, i, i, i, i, p, p, p, p, p, i, i, ctypes.c_float, dbl, dbl, i, i, p, ctypes.c_size_t, p]
    lib.plb_host_table_bin.argtypes = [p, i, dbl]
    lib.plb_host_table_ok.argtypes = [p, i]
    lib.plb_host_differs_from_eval.argtypes = [p, i, i, i, i, ctypes.c_float]
    return lib


def flat_args(a):
    """the arrays of a case as the C side takes them"""
    m = np.ascontiguousarray(a["m"], np.float32)
    B = m.shape[0]
    sizes = np.ascontiguousarray(a["sizes"], np.int32).reshape(B, 2)
    calib = np.ascontiguousarray(np.concatenate([np.reshape(a["P"], (B, 12)), np.reshape(a["T"], (B, 16))], axis=1), np.float64)
    inten = None if a["intensity"] is None else np.ascontiguousarray(a["intensity"], np.float32)
    elev, azim = (None, None) if a["beams"] is None else (np.ascontiguousarray(t, np.float64) for t in a["beams"])
    return m, sizes, calib, inten, elev, azim


def host_project(host, a, capacity=None):
    m, sizes, calib, inten, elev, azim = flat_args(a)
    B, h, w = m.shape
    nb, na = (0, 0) if elev is None else (elev.size - 1, azim.size - 1)
    capacity = B * (nb * na if nb else a["Hg"] * a["Wg"]) if capacity is None else capacity
    cloud = np.full((capacity, 4), -7.0, np.float32)
    offsets = np.zeros(B + 1, np.int32)
    ptr = lambda x: None if x is None else x.ctypes.data
    rc = host.plb_host_project(ptr(m), B, h, w, a["Hg"], a["Wg"], ptr(sizes), ptr(calib), ptr(inten), ptr(elev), ptr(azim), nb, na,
                               a["scale"], a["max_height"], a["max_depth"], a["sparsity"], 1 if a["input"] == "depth" else 0,
                               ptr(cloud), capacity, ptr(offsets))
    assert rc == 0
    return cloud, offsets


@pytest.mark.parametrize("case", C.CASES)
def test_header_matches_restatement(host, case):
    want, woff = C.reference(case)
    cloud, offsets = host_project(host, C.build(case))
    assert np.array_equal(offsets, woff)
    bits_equal(cloud[:woff[-1]], want)
    assert (cloud[woff[-1]:] == -7.0).all()


@pytest.mark.parametrize("h,w,H,W", [(8, 13, 23, 37), (24, 40, 375, 400), (192, 640, 375, 1242)])
def test_header_resize_and_depth_are_eval_maths(host, h, w, H, W):
    """pl_math.h spells the protocol's resize and depth conversion out once more (so that the device keeps products and sums apart); on
    the host it is eval_math.h's, bit for bit, and both are the restatement"""
    disp = np.random.RandomState(h + W).rand(h, w).astype(np.float32)
    assert host.plb_host_differs_from_eval(disp.ctypes.data, h, w, H, W, 5.4) == 0
    a = dict(C.build("direct-dense"), m=disp[None], sizes=[(H, W)], Hg=H, Wg=W, max_height=np.inf, scale=5.4,
             P=C.scaled_P(C.DATES[0], H, W)[None])
    want, woff = R.project_batch(**a)
    cloud, offsets = host_project(host, a)
    assert woff[-1] == H * W and np.array_equal(offsets, woff)
    bits_equal(cloud, want)


def test_header_small_capacity(host):
    want, woff = C.reference("odd-dense")
    cap = int(woff[1]) + 5
    cloud, offsets = host_project(host, C.build("odd-dense"), capacity=cap)
    assert np.array_equal(offsets, woff)
    bits_equal(cloud, want[:cap])


def test_header_table_bin_edges(host):
    tab = np.array([-1.0, -0.25, 0.0, 0.5, 2.0])
    for v, k in [(-1.0, 0), (-0.25, 1), (0.0, 2), (-0.0, 2), (0.5, 3), (1.999, 3), (2.0, -1), (-1.0000001, -1), (np.nan, -1), (np.inf, -1)]:
        assert host.plb_host_table_bin(tab.ctypes.data, 4, v) == k == int(R.table_bin(tab, np.float64(v))), v
    for bad in ([0.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf], [-np.inf, 0.0, 1.0]):
        assert host.plb_host_table_ok(np.array(bad).ctypes.data, 2) == 0
    assert host.plb_host_table_ok(tab.ctypes.data, 4) == 1


def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the case with three images of different
    sizes, an intensity plane and beams: a finding ends the program with a non-zero status."""
    exe = str(tmp_path / "pl_batch_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPLB_STANDALONE"]) +
                          ["-o", exe])
    case = "odd-beams8x16_intensity_depth"
    a = C.build(case)
    m, sizes, calib, inten, elev, azim = flat_args(a)
    B, h, w = m.shape
    cap = B * 8 * 16
    head = np.array([B, h, w, a["Hg"], a["Wg"], 8, 16, a["sparsity"], 1, 1, cap, 0], np.int32)
    with open(str(tmp_path / "in.bin"), "wb") as f:
        for part in (head, np.array([a["scale"], a["max_height"], a["max_depth"]], np.float64), sizes, calib, m, inten, elev, azim):
            f.write(part.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    status = np.frombuffer(raw, np.int32, 1)[0]
    offsets = np.frombuffer(raw, np.int32, B + 1, 4)
    cloud = np.frombuffer(raw, np.float32, cap * 4, 4 * (B + 2)).reshape(cap, 4)
    want, woff = C.reference(case)
    assert status == 0 and np.array_equal(offsets, woff)
    bits_equal(cloud[:woff[-1]], want)
    assert (cloud[woff[-1]:].view(np.uint32) == 0xFFFFFFFF).all()


# ---------------------------------------------------------------------------------------------- properties of the restatement
def one_image(case, b=0):
    a = C.build(case)
    Hb, Wb = a["sizes"][b]
    d = R.depth_image(a["m"][b], Hb, Wb, a["input"], a["scale"])
    q = R.points(d, a["P"][b], a["T"][b])
    return a, d, q, R.kept(q, d, a["max_height"], a["max_depth"])


def test_beam_mode_is_order_independent():
    for case in ("odd-beams8x16", "chunks-beams64x512"):
        a, d, q, keep = one_image(case)
        base = R.beam_winners(q, keep, *a["beams"])
        for seed in range(3):
            order = np.random.RandomState(seed).permutation(keep.size)
            assert np.array_equal(R.beam_winners(q, keep, *a["beams"], order=order), base)
        assert np.array_equal(R.beam_winners(q, keep, *a["beams"], order=np.arange(keep.size)[::-1]), base)


def test_nearest_wins_and_ties_go_to_the_lowest_pixel():
    """Two pixels of one cell with equal float32 range: points whose float64 ranges differ below float32 resolution."""
    elev, azim = np.array([-1.0, 1.0]), np.array([-1.0, 1.0])
    q = np.array([[10.0, 0.0, -1.0], [10.0 + 1e-9, 0.0, -1.0], [10.0, 0.0, -1.0], [30.0, 0.0, -1.0], [5.0, 0.0, -1.0]]).reshape(1, 5, 3)
    r = R.range32(q)[0]
    assert r[0] == r[1] == r[2] and q[0, 1, 0] != q[0, 0, 0]
    keep = np.array([[False, True, True, True, False]])
    assert R.beam_winners(q, keep, elev, azim).tolist() == [1]                       # 1 and 2 tie: the lower index; 4 is nearer but not kept
    for order in ([2, 1, 3, 0, 4], [3, 2, 1, 0, 4]):
        assert R.beam_winners(q, keep, elev, azim, order=np.array(order)).tolist() == [1]
    keep[0, 4] = True
    assert R.beam_winners(q, keep, elev, azim).tolist() == [4]                       # the nearest wins


def test_every_beam_point_is_a_dense_point():
    for shape in C.SHAPES:
        dense, doff = C.reference(shape + "-dense")
        for variant in ("beams8x16", "beams64x512"):
            beam, boff = C.reference("%s-%s" % (shape, variant))
            for b in range(len(doff) - 1):
                rows = set(map(bytes, dense[doff[b]:doff[b + 1]]))
                mine = beam[boff[b]:boff[b + 1]]
                assert len(mine) and all(bytes(r) in rows for r in mine)
                assert len(set(map(bytes, mine))) <= len(mine) <= doff[b + 1] - doff[b]


def test_points_on_table_edges():
    """A point exactly on an edge belongs to the upper cell; on the last edge it is dropped."""
    elev = np.array([-1.0, -0.25, 0.0, 1.0])            # s = q2 |q2| / (q0^2 + q1^2)
    azim = np.array([-1.0, 0.0, 0.5, 1.0])              # a = q1 / q0
    q = np.array([[2.0, 0.0, -1.0],                     # s = -0.25 exactly, a = 0 exactly: cell (1, 1)
                  [2.0, 1.0, 0.0],                      # s = 0, a = 0.5: cell (2, 2)
                  [2.0, 2.0, 0.0],                      # a = 1: the last edge, dropped
                  [1.0, 0.0, 1.0],                      # s = 1: the last edge, dropped
                  [2.0, -2.0, -0.5],                    # a = -1, s = -0.03125: cell (1, 0)
                  [1.0, 0.0, -1.0],                     # s = -1: cell (0, 1)
                  [0.0, 0.0, -1.0],                     # q0 = 0: in front of no cell
                  [2.0, np.nan, 0.0]]).reshape(1, 8, 3)
    beam, az = R.cells_of(q, elev, azim)
    assert beam[0].tolist() == [1, 2, -1, -1, 1, 0, -1, -1]
    assert az[0].tolist() == [1, 2, -1, -1, 0, 1, -1, -1]


def test_beam_tables_refuses_non_increasing_input():
    import mcav.lib as L
    from pseudo_lidar import BeamTables, beam_tables
    t = beam_tables()
    assert t.n_beams == 64 and t.n_azimuth == 512 and t.elev.dtype == t.azim.dtype == np.float64
    want = C.uniform_tables(64, 512)
    assert np.array_equal(t.elev, want[0]) and np.array_equal(t.azim, want[1])
    assert (np.diff(t.elev) > 0).all() and (np.diff(t.azim) > 0).all()
    assert np.allclose(np.rad2deg(np.arctan(t.azim[[0, -1]])), [-45, 45]) and np.allclose(np.diff(np.rad2deg(np.arctan(t.azim))), 90 / 512)
    small = beam_tables(8, 16)
    assert tuple(len(x) for x in small) == (9, 17)
    for kw in (dict(elevation=(2.0, -23.6)), dict(azimuth=(45.0, -45.0)), dict(azimuth=(10.0, 10.0)), dict(azimuth=(-100.0, 100.0))):
        with pytest.raises(L.MCAVError):
            beam_tables(**kw)
    with pytest.raises(L.MCAVError):
        beam_tables(0, 16)
    hdl = np.concatenate([np.linspace(-24.9, -8.87, 33)[:-1], np.linspace(-8.53, 2.0, 33)])      # two blocks of unequal pitch: accepted
    e = np.tan(np.deg2rad(hdl))
    BeamTables(e * np.abs(e), t.azim)
    for bad in ([0.0, 0.0, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf], [1.0]):
        with pytest.raises(L.MCAVError):
            BeamTables(bad, t.azim)


def test_project_batch_refuses_bad_arguments_without_a_gpu():
    import torch
    import mcav.lib as L
    from pseudo_lidar import PseudoLiDAR, beam_tables
    pl = PseudoLiDAR.from_matrices(C.velo_T(C.DATES[0]), C.scaled_P(C.DATES[0], 8, 16), 0)
    with pytest.raises(L.MCAVError):
        pl.project_batch(torch.zeros(1, 8, 16))                                      # a CPU tensor
    with pytest.raises(L.MCAVError):
        pl.project_batch(torch.zeros(8, 16))                                         # wrong rank
    with pytest.raises(L.MCAVError):
        pl.project_batch(np.zeros((1, 8, 16), np.float32))
    pl3 = PseudoLiDAR.from_matrices(pl.T, pl.P, 3)
    assert pl3.sparsity == 3 and beam_tables(8, 16).n_beams == 8


# ---------------------------------------------------------------------------------------------- the loader
def test_loader_calibration_is_opt_in(tmp_path):
    import torch
    from dataloaders import UnSupKittiDataset, read_calib_file
    from kitti_velo_tree import make_velo_tree, velo_config
    split, rows, _ = make_velo_tree(str(tmp_path), frames=4, sweep=100, extra=10)
    cfg = velo_config(split, str(tmp_path))
    plain = UnSupKittiDataset(cfg)
    cfg2 = velo_config(split, str(tmp_path))
    cfg2["datasets"]["calibration"] = True
    ds = UnSupKittiDataset(cfg2)
    assert len(ds) == len(plain) == len(rows) == 4
    new = {"P_rect", "T_velo_cam", "native_size", "path"}
    for i in range(len(ds)):
        a, b = plain[i], ds[i]
        assert set(b) - set(a) == new and not (set(a) & new)
        for k in a:                                                                  # everything else is what it was
            va, vb = a[k], b[k]
            if isinstance(va, list):
                assert all(torch.equal(x, y) for x, y in zip(va, vb))
            else:
                assert torch.equal(va, vb), k
        date = [p for p in rows[i][0].split("/") if p.startswith("2011_") and "drive" not in p][0]
        d = os.path.join(str(tmp_path), "KITTI", date)
        cam, velo = read_calib_file(os.path.join(d, "calib_cam_to_cam.txt")), read_calib_file(os.path.join(d, "calib_velo_to_cam.txt"))
        assert b["P_rect"].dtype == torch.float64 and np.array_equal(b["P_rect"].numpy(), cam["P_rect_02"].reshape(3, 4))
        T = b["T_velo_cam"].numpy()
        assert T.shape == (4, 4) and np.array_equal(T[:3, :3], velo["R"].reshape(3, 3)) and np.array_equal(T[:3, 3], velo["T"])
        assert T[3].tolist() == [0, 0, 0, 1]
        assert tuple(b["native_size"].tolist()) == tuple(b["tgt"].shape[:2]) and b["path"] == rows[i][0]
    # without the velodyne ground truth too
    from kitti_tree import config_for
    cfg3 = config_for(split, str(tmp_path), 24, 80, 2)
    cfg3["datasets"]["calibration"] = True
    s = UnSupKittiDataset(cfg3)[0]
    assert new <= set(s) and "velodyne" not in s


# ---------------------------------------------------------------------------------------------- inference.py without a GPU
def test_inference_names_and_refusals():
    import inference
    p = inference.Inference.cloud_path("out", "KITTI/2011_09_26/2011_09_26_drive_0001_sync/image_02/data/0000000003.png")
    assert p == os.path.join("out", "2011_09_26", "2011_09_26_drive_0001_sync", "pseudo_velodyne", "data", "0000000003.bin")
    with pytest.raises(ValueError):
        inference.Inference.cloud_path("out", "frame.png")
    with pytest.raises(SystemExit):
        inference.main(["--config", "c.yaml"])                                       # --checkpoint and --out are required
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            inference.Inference({})                                                  # no CPU fallback
