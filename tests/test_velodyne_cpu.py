"""CPU: KITTI Eigen ground truth from raw Velodyne scans (include/mcav_depth.h: mcav_velo_depth_map, geometry/velodyne.py).  The
restatement (tests/velo_ref.py) against a transcription of monodepth2's generate_depth_map, and the per-point header csrc/velo_math.h
compiled for the host against the restatement, on the same cases; the calibration composition; the velodyne ground-truth mode of the KITTI
reader."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import velo_ref as V
from conftest import PKG, REPO

SIZES = [("2011_09_26", 375, 1242), ("2011_09_28", 370, 1226)]


def bits_equal(got, want):
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- restatement vs monodepth2
@pytest.mark.parametrize("seed", range(4))
def test_restatement_matches_monodepth2_inside(host, seed):
    date, H, W = SIZES[seed % 2]
    P = V.kitti_P(date)
    velo = V.scan(seed + 10 * (seed % 2))
    a = V.monodepth2(P, velo, (H, W)).astype(np.float32)
    b = V.restated(P, velo, (H, W))
    assert (b > 0).sum() > 5000                         # a real sweep lands ~15 k points
    assert np.array_equal(a[:, 1:-1], b[:, 1:-1])
    bits_equal(host_map(host, P, velo, H, W), b)        # csrc/velo_math.h


def test_edge_aliasing_only_on_edge_columns(host):
    H, W = 375, 1242
    P = V.kitti_P("2011_09_26")
    velo = V.edge_aliasing_case(P, (H, W))
    perm = np.random.RandomState(3).permutation(len(velo))
    b = V.restated(P, velo, (H, W))
    assert np.array_equal(b, V.restated(P, velo[perm], (H, W)))       # order-independent
    ndiff = 0
    for v in (velo, velo[perm]):
        a = V.monodepth2(P, v, (H, W)).astype(np.float32)
        assert np.array_equal(a[:, 1:-1], b[:, 1:-1])
        ndiff += int((a != b).sum())
        bits_equal(host_map(host, P, v, H, W), b)
    assert ndiff > 0                                    # the aliasing shows on columns 0 and W-1


def test_negative_camera_depth_is_zero(host):
    H, W = 375, 1242
    P = V.kitti_P("2011_09_26")
    rng = np.random.RandomState(5)
    near = np.stack([np.array([rng.uniform(0.0, 0.2), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 0.5], np.float32)
                     for _ in range(200)])
    ok, u, v, d = V.landing(P, near, (H, W))
    assert ok.sum() > 0 and (d[ok] < 0).all()           # they land, behind the camera
    b = V.restated(P, near, (H, W))
    assert not (b != 0).any() and not np.signbit(b).any()
    assert np.array_equal(V.monodepth2(P, near, (H, W)).astype(np.float32), b)
    bits_equal(host_map(host, P, near, H, W), b)


def test_half_even_ties(host):
    b = V.restated(V.P_DYADIC, V.tie_points(), (8, 8))
    bits_equal(host_map(host, V.P_DYADIC, V.tie_points(), 8, 8), b)
    assert sorted(map(tuple, np.argwhere(b > 0).tolist())) == [(1, 1), (1, 3)]
    assert b[1, 1] == 2 and b[1, 3] == 2
    assert np.array_equal(V.monodepth2(V.P_DYADIC, V.tie_points(), (8, 8)).astype(np.float32), b)


def test_special_points(host):
    H, W = 370, 1226
    P = V.kitti_P("2011_09_28")
    velo = np.concatenate([V.scan(7, 5000), V.special_points()])
    b = V.restated(P, velo, (H, W))
    assert np.array_equal(V.monodepth2(P, velo, (H, W)).astype(np.float32), b)
    ok, _, _, _ = V.landing(P, V.special_points(), (H, W))
    assert not ok.any()
    # +inf is kept: a float64 depth above FLT_MAX
    huge = np.array([[1e38, 2e38, 2e38, 0]], np.float32)
    m = V.restated(V.P_OVERFLOW, huge, (4, 4))
    assert m[0, 0] == np.inf and (m.reshape(-1)[1:] == 0).all()
    bits_equal(host_map(host, P, velo, H, W), b)
    bits_equal(host_map(host, V.P_OVERFLOW, huge, 4, 4), m)


def test_image_borders(host):
    H, W = 375, 1242
    P = V.kitti_P("2011_09_26")
    pts = np.stack([V.point_at(P, W - 1, 100, 12.0), V.point_at(P, 600, H - 1, 13.0), V.point_at(P, W, 120, 14.0),
                    V.point_at(P, 600, H, 15.0), V.point_at(P, -1, 100, 16.0)])
    ok, u, v, _ = V.landing(P, pts, (H, W))
    assert ok.tolist() == [True, True, False, False, False]
    assert (u[0], v[0], u[1], v[1]) == (W - 1, 100, 600, H - 1)
    b = V.restated(P, pts, (H, W))
    assert b[100, W - 1] == np.float32(V.project(P, pts[:1])[3][0]) and b[H - 1, 600] > 0 and (b > 0).sum() == 2
    bits_equal(host_map(host, P, pts, H, W), b)


def test_depth_from_x_and_flip(host):
    H, W = 375, 1242
    P = V.kitti_P("2011_09_26")
    velo = V.scan(11, 30000)
    bx = V.restated(P, velo, (H, W), depth_from_x=True)
    ax = V.monodepth2(P, velo, (H, W), vel_depth=True).astype(np.float32)
    assert np.array_equal(ax[:, 1:-1], bx[:, 1:-1])
    ok, u, v, _ = V.landing(P, velo, (H, W))
    assert np.array_equal(bx[v[ok], u[ok]] > 0, velo[ok, 0] > 0)
    assert np.array_equal(V.restated(P, velo, (H, W), flip=True), V.restated(P, velo, (H, W))[:, ::-1])
    bits_equal(host_map(host, P, velo, H, W, depth_from_x=True), bx)
    bits_equal(host_map(host, P, velo, H, W, flip=True), V.restated(P, velo, (H, W), flip=True))


# ---------------------------------------------------------------------------------------------- csrc/velo_math.h on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("velo_hostcheck") / "libvelo_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(REPO, "tests", "velo_hostcheck", "velo_hostcheck.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.vd_project.argtypes = [p, i, p, i, i, i, p, p, p, p]
    lib.vd_map.argtypes = [p, i, p, i, i, i, i, p]
    return lib


def host_project(host, P, pts, H, W, depth_from_x=False):
    pts = np.ascontiguousarray(pts, np.float32)
    P = np.ascontiguousarray(P, np.float64).reshape(12)
    n = len(pts)
    landed, u, v, key = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    host.vd_project(pts.ctypes.data, n, P.ctypes.data, H, W, int(depth_from_x), landed.ctypes.data, u.ctypes.data, v.ctypes.data,
                    key.ctypes.data)
    return landed.astype(bool), u, v, key


def host_map(host, P, pts, H, W, flip=False, depth_from_x=False):
    pts = np.ascontiguousarray(pts, np.float32)
    P = np.ascontiguousarray(P, np.float64).reshape(12)
    out = np.zeros((H, W), np.float32)
    host.vd_map(pts.ctypes.data, len(pts), P.ctypes.data, H, W, int(flip), int(depth_from_x), out.ctypes.data)
    return out


CASES = [("sweep26", lambda: (V.kitti_P("2011_09_26"), V.scan(21, 60000), 375, 1242)),
         ("sweep28", lambda: (V.kitti_P("2011_09_28"), V.scan(22, 60000), 370, 1226)),
         ("edges", lambda: (V.kitti_P("2011_09_26"), V.edge_aliasing_case(V.kitti_P("2011_09_26"), (375, 1242)), 375, 1242)),
         ("special", lambda: (V.kitti_P("2011_09_28"), np.concatenate([V.scan(8, 3000), V.special_points()]), 370, 1226)),
         ("ties", lambda: (V.P_DYADIC, V.tie_points(), 8, 8)),
         ("overflow", lambda: (V.P_OVERFLOW, np.array([[1e38, 2e38, 2e38, 0], [1, 1, 1, 0]], np.float32), 4, 4))]


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("depth_from_x", [False, True])
def test_header_matches_restatement(host, name, make, depth_from_x):
    P, pts, H, W = make()
    landed, u, v, key = host_project(host, P, pts, H, W, depth_from_x)
    ok, ru, rv, d = V.landing(P, pts, (H, W), depth_from_x)
    assert np.array_equal(landed, ok)
    assert np.array_equal(u[ok], ru[ok]) and np.array_equal(v[ok], rv[ok])
    with np.errstate(over="ignore"):
        assert np.array_equal(key[ok], V.depth_key(d[ok].astype(np.float32)))
    for flip in (False, True):
        got = host_map(host, P, pts, H, W, flip, depth_from_x)
        want = V.restated(P, pts, (H, W), flip, depth_from_x)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, flip)


# ---------------------------------------------------------------------------------------------- calibration and the KITTI reader
def test_velo_to_image_composition(tmp_path):
    from dataloaders import read_calib_file
    from geometry.velodyne import velo_to_image
    from kitti_tree import SIZES as TREE_SIZES
    from kitti_velo_tree import make_velo_tree, tree_P
    make_velo_tree(str(tmp_path), frames=2, sweep=100, extra=10)
    for date in ("2011_09_26", "2011_09_28"):
        d = os.path.join(str(tmp_path), "KITTI", date)
        P, hw = velo_to_image(d)
        c = read_calib_file(os.path.join(d, "calib_cam_to_cam.txt"))
        v = read_calib_file(os.path.join(d, "calib_velo_to_cam.txt"))
        R = np.eye(4)
        R[:3, :3] = c["R_rect_00"].reshape(3, 3)
        v2c = np.vstack((np.hstack((v["R"].reshape(3, 3), v["T"].reshape(3, 1))), [0, 0, 0, 1.0]))
        want = np.dot(np.dot(c["P_rect_02"].reshape(3, 4), R), v2c)
        assert P.dtype == np.float64 and np.array_equal(P, want) and np.array_equal(P, tree_P(date))
        assert hw == tuple(int(x) for x in c["S_rect_02"][::-1]) == TREE_SIZES[date]


def test_load_velodyne_points(tmp_path):
    from geometry.velodyne import load_velodyne_points
    pts = V.scan(4, 1000)
    pts.tofile(str(tmp_path / "a.bin"))
    got = load_velodyne_points(str(tmp_path / "a.bin"))
    assert got.dtype == np.float32 and got.shape == (1000, 4) and np.array_equal(got, pts)


def test_dataset_derives_scan_paths(tmp_path):
    from dataloaders import UnSupKittiDataset
    from kitti_velo_tree import make_velo_tree, velo_config
    split, rows, scans = make_velo_tree(str(tmp_path), sweep=100, extra=10)
    ds = UnSupKittiDataset(velo_config(split, str(tmp_path)))
    assert ds.native_gt and ds.velodyne_gt and len(ds) == 6
    for s, r in zip(ds.samples, rows):
        assert s["velodyne"] == scans[r[0]] and s["groundtruth"] is None
    s = ds[0]
    assert s["velodyne"].dtype == __import__("torch").float32 and tuple(s["velodyne"].shape) == (110, 4)
    assert np.array_equal(s["velodyne"].numpy(), np.fromfile(scans[rows[0][0]], np.float32).reshape(-1, 4))   # unfiltered
    assert tuple(s["velodyne_size"].tolist()) == (47, 156) and tuple(s["velodyne_P"].shape) == (3, 4)
    assert "groundtruth" not in s


def test_dataset_scan_override_and_missing(tmp_path):
    import shutil
    from dataloaders import UnSupKittiDataset
    from kitti_velo_tree import make_velo_tree, velo_config
    split, rows, scans = make_velo_tree(str(tmp_path), sweep=100, extra=10)
    other = str(tmp_path / "elsewhere.bin")
    shutil.copy(scans[rows[1][0]], other)
    lines = [" ".join(r[:3] + [other]) if i == 0 else " ".join(r) for i, r in enumerate(rows)]
    with open(split, "w") as f:
        f.write("\n".join(lines) + "\n")
    ds = UnSupKittiDataset(velo_config(split, str(tmp_path)))
    assert ds.samples[0]["velodyne"] == other and ds.samples[1]["velodyne"] == scans[rows[1][0]]
    os.remove(scans[rows[2][0]])
    with pytest.raises(ValueError, match=os.path.basename(scans[rows[2][0]])):
        UnSupKittiDataset(velo_config(split, str(tmp_path)))
    with open(split, "w") as f:
        f.write(" ".join(rows[0][:3] + [str(tmp_path / "missing.bin")]) + "\n")
    with pytest.raises(ValueError, match="missing.bin"):
        UnSupKittiDataset(velo_config(split, str(tmp_path)))


def test_dataset_size_mismatch_raises(tmp_path):
    from dataloaders import UnSupKittiDataset
    from kitti_velo_tree import make_velo_tree, velo_config
    split, rows, _ = make_velo_tree(str(tmp_path), sweep=100, extra=10)
    calib = os.path.join(str(tmp_path), "KITTI", "2011_09_26", "calib_cam_to_cam.txt")
    with open(calib, "a") as f:
        f.write("S_rect_02: 1.242000e+03 3.750000e+02\n")        # the full KITTI size; the tree's images are 1/8 of it
    ds = UnSupKittiDataset(velo_config(split, str(tmp_path)))
    with pytest.raises(ValueError, match="S_rect_02"):
        ds[0]


def test_unknown_groundtruth_mode_lists_velodyne(tmp_path):
    from dataloaders import UnSupKittiDataset
    from kitti_velo_tree import make_velo_tree, velo_config
    split, _, _ = make_velo_tree(str(tmp_path), sweep=100, extra=10)
    cfg = velo_config(split, str(tmp_path))
    cfg["datasets"]["groundtruth"] = "lidar"
    with pytest.raises(ValueError, match="velodyne"):
        UnSupKittiDataset(cfg)
