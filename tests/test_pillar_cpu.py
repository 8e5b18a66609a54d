"""CPU: the pillar voxeliser (include/mcav_depth.h: mcav_pillarize, pseudo_lidar.pillarize).  The restatement (tests/pillar_ref.py) against a
sequential transcription of second.pytorch's points_to_voxel; the header csrc/pillar_math.h compiled for the host against the restatement,
bit for bit, on the cases the GPU tests run (tests/pillar_cases.py), once more as a stand-alone program under the address and
undefined-behaviour sanitizers; properties of the definition; what the Python side refuses without a GPU; the new inference path names."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pillar_cases as C
import pillar_ref as R
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "pillar_hostcheck", "pillar_hostcheck.cpp")
F = np.float32


def same(got, want):
    """every output, bit for bit"""
    assert sorted(got) == sorted(want) == ["coords", "num_points", "offsets", "voxels"]
    assert np.array_equal(got["offsets"], want["offsets"])
    assert got["coords"].shape == want["coords"].shape and np.array_equal(got["coords"], want["coords"])
    assert np.array_equal(got["num_points"], want["num_points"])
    assert got["voxels"].shape == want["voxels"].shape and got["voxels"].dtype == want["voxels"].dtype == F
    assert np.array_equal(got["voxels"].view(np.uint32), want["voxels"].view(np.uint32))


# ---------------------------------------------------------------------------------------------- restatement vs the sequential loop
@pytest.mark.parametrize("case", C.CASES)
def test_restatement_matches_sequential_transcription(case):
    C.check_non_trivial(case)
    a, want = C.build(case), C.reference(case)
    seq = R.sequential_batch(a["points"], a["offsets"], a["grid"], a["max_points"])
    same(seq, dict(want, voxels=np.ascontiguousarray(want["voxels"][:, :, :4])))
    if a["decorate"]:                                        # the plain columns of a decorated call are the plain call's
        plain = R.pillarize(**dict(a, decorate=False))
        same(plain, dict(want, voxels=np.ascontiguousarray(want["voxels"][:, :, :4])))


def test_kitti_grid_is_432_by_496():
    g = R.make_grid()
    assert (g.nx, g.ny) == (432, 496)
    assert all(isinstance(v, F) for v in g[:6])


# ---------------------------------------------------------------------------------------------- csrc/pillar_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pillar_hostcheck") / "libpillar_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    lib.pil_host_pillarize.argtypes = [p, p, i, ll, f, f, f, f, f, f, i, i, i, i, p, p, p, ll, p]
    lib.pil_host_axis_cell.argtypes = [f, f, f, i]
    lib.pil_host_image_of.argtypes = [p, i, i]
    return lib


def host_pillarize(host, a, capacity=None):
    pts, off, g, N = np.ascontiguousarray(a["points"]), np.ascontiguousarray(a["offsets"]), a["grid"], a["max_points"]
    B, Cc = len(off) - 1, 9 if a["decorate"] else 4
    cap = min(len(pts), B * g.ny * g.nx) if capacity is None else capacity
    vox = np.full((cap, N, Cc), -7.0, F)
    coords, num, poff = np.full((cap, 4), -7, np.int32), np.full(cap, -7, np.int32), np.full(B + 1, -7, np.int32)
    rc = host.pil_host_pillarize(pts.ctypes.data, off.ctypes.data, B, len(pts), g.x0, g.y0, g.z0, g.z1, g.vx, g.vy, g.nx, g.ny, N,
                                 1 if a["decorate"] else 0, vox.ctypes.data, coords.ctypes.data, num.ctypes.data, cap, poff.ctypes.data)
    assert rc == 0
    return dict(voxels=vox, coords=coords, num_points=num, offsets=poff)


def used(out, P):
    return dict(voxels=out["voxels"][:P], coords=out["coords"][:P], num_points=out["num_points"][:P], offsets=out["offsets"])


@pytest.mark.parametrize("case", C.CASES)
def test_header_matches_restatement(host, case):
    want = C.reference(case)
    got = host_pillarize(host, C.build(case))
    P = int(want["offsets"][-1])
    same(used(got, P), want)
    assert (got["voxels"][P:] == -7.0).all() and (got["coords"][P:] == -7).all() and (got["num_points"][P:] == -7).all()


def test_header_small_capacity(host):
    case = "pair-N5-c9"
    want = C.reference(case)
    cap = int(want["offsets"][1]) + 3                        # ends inside the second image
    got = host_pillarize(host, C.build(case), capacity=cap)
    same(got, R.pillarize(capacity=cap, **C.build(case)))
    assert np.array_equal(got["offsets"], want["offsets"]) and len(got["coords"]) == cap < int(want["offsets"][-1])


def test_header_edges_and_special_values(host):
    """lower edges in, upper edges out, -0.0 is cell 0, NaN and the infinities name no cell -- the header and the restatement alike"""
    nan, inf = np.nan, np.inf
    table = [(0.0, 0), (-0.0, 0), (0.16, 1), (np.nextafter(F(0.16), F(0)), 0), (69.12, -1), (np.nextafter(F(69.12), F(0)), 431), (-1e-30, -1),
             (nan, -1), (inf, -1), (-inf, -1), (3.0e38, -1), (-3.0e38, -1)]
    for v, cell in table:
        got = host.pil_host_axis_cell(v, 0.0, 0.16, 432)
        c, ok = R.axis_cells(np.array([v], F), F(0.0), F(0.16), 432)
        assert got == cell == (int(c[0]) if ok[0] else -1), (v, got, cell)
    g = R.make_grid(x=(0.0, 2.0), y=(0.0, 2.0), z=(-1.0, 1.0), size=(1.0, 1.0))
    pts = np.array([[-0.0, -0.0, -1.0, 1], [0, 0, 1.0, 2], [2.0, 0, 0, 3], [0, 2.0, 0, 4], [1.0, 1.0, np.nextafter(F(1), F(0)), 5],
                    [nan, 0, 0, 6], [0, 0, nan, 7], [inf, 0, 0, 8], [0, -inf, 0, 9]], F)
    out = R.pillarize(pts, [0, len(pts)], g, max_points=4)
    assert out["coords"].tolist() == [[0, 0, 0, 0], [0, 0, 1, 1]] and out["num_points"].tolist() == [1, 1]
    assert out["voxels"][:, 0, 3].tolist() == [1.0, 5.0]
    assert np.signbit(out["voxels"][0, 0, :3]).all()          # the -0.0 coordinates are copied bit for bit
    same(used(host_pillarize(host, dict(points=pts, offsets=np.array([0, len(pts)], np.int32), grid=g, max_points=4, decorate=False)), 2), out)


def test_header_image_of_steps_over_empty_images(host):
    off = np.array([0, 3, 3, 3, 7, 7], np.int32)
    for i, b in [(0, 0), (2, 0), (3, 3), (6, 3)]:
        assert host.pil_host_image_of(off.ctypes.data, 5, i) == b == int(R.image_of(off, i))


def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the hardest case (chunked selection, a cut last
    image, decorated columns) with a capacity that ends inside the second image: a finding ends the program with a non-zero status."""
    exe = str(tmp_path / "pillar_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPIL_STANDALONE"]) +
                          ["-o", exe])
    a, want = C.build(C.HARDEST), C.reference(C.HARDEST)
    g, N, B = a["grid"], a["max_points"], len(a["offsets"]) - 1
    for cap in (int(want["offsets"][-1]), int(want["offsets"][1]) + 3):
        head = np.array([B, len(a["points"]), g.nx, g.ny, N, 1, cap, 0], np.int64)
        with open(str(tmp_path / "in.bin"), "wb") as f:
            for part in (head, np.array(g[:6], F), a["offsets"], a["points"]):
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        raw = open(str(tmp_path / "out.bin"), "rb").read()
        assert np.frombuffer(raw, np.int32, 1)[0] == 0
        at = 4
        poff = np.frombuffer(raw, np.int32, B + 1, at); at += 4 * (B + 1)
        num = np.frombuffer(raw, np.int32, cap, at); at += 4 * cap
        coords = np.frombuffer(raw, np.int32, 4 * cap, at).reshape(cap, 4); at += 16 * cap
        vox = np.frombuffer(raw, F, cap * N * 9, at).reshape(cap, N, 9)
        assert at + 4 * vox.size == len(raw)
        same(dict(voxels=vox, coords=coords, num_points=num, offsets=poff), R.pillarize(capacity=cap, **a))


# ---------------------------------------------------------------------------------------------- properties of the definition
def test_permuting_an_image_changes_slots_only():
    """The set of pillars, their coords and offsets do not depend on the order of an image's points; a pillar of at most N points keeps
    the same set of rows, a fuller one keeps the N that now come first, in the new order."""
    a = C.build("pair-N5-c4")
    base = C.reference("pair-N5-c4")
    pts, off, N = a["points"].copy(), a["offsets"], a["max_points"]
    perm = np.random.RandomState(5).permutation(int(off[1]))
    moved = pts.copy()
    moved[:off[1]] = pts[:off[1]][perm]
    out = R.pillarize(moved, off, a["grid"], N)
    assert np.array_equal(out["offsets"], base["offsets"]) and np.array_equal(out["coords"], base["coords"])
    assert np.array_equal(out["num_points"], base["num_points"])
    counts = R.cell_counts(pts, off, a["grid"])
    changed = 0
    for r, (b, _, iy, ix) in enumerate(base["coords"]):
        k = int(base["num_points"][r])
        rows = lambda v: sorted(map(bytes, v[r, :k]))
        if b != 0:
            assert np.array_equal(out["voxels"][r].view(np.uint32), base["voxels"][r].view(np.uint32))
        elif counts[b, iy, ix] <= N:
            assert rows(out["voxels"]) == rows(base["voxels"])
        else:
            ixs, iys, keep = R.cells_of(moved[:off[1]], a["grid"])
            first = moved[:off[1]][keep & (ixs == ix) & (iys == iy)][:N]
            assert np.array_equal(out["voxels"][r, :k].view(np.uint32), first.view(np.uint32))
            changed += rows(out["voxels"]) != rows(base["voxels"])
    assert changed >= 3                                      # the planted cells of 65, 130 and 300 points kept other points
    same(R.sequential_batch(moved, off, a["grid"], N), out)


def test_padding_and_decorated_columns():
    """slots behind num_points are +0.0 in every column; the decorated columns are what a float64 reading of the definition gives, within
    the roundings the definition spells out"""
    a, want = C.build("mixed-N32-c9"), C.reference("mixed-N32-c9")
    v, k, g = want["voxels"], want["num_points"], a["grid"]
    pad = np.arange(32)[None, :] >= k[:, None]
    assert pad.any() and (v.view(np.uint32)[pad] == 0).all()
    for r in range(len(v)):
        rows = v[r, :k[r]].astype(np.float64)
        mean = rows[:, :3].sum(0) / k[r]
        assert np.abs(rows[:, 4:7] - (rows[:, :3] - mean)).max() <= 4 * 2.0 ** -24 * 4.0          # |coordinates| < 4 m here
        cx = g.x0 + g.vx * (want["coords"][r, 3] + 0.5)
        cy = g.y0 + g.vy * (want["coords"][r, 2] + 0.5)
        assert np.abs(rows[:, 7] - (rows[:, 0] - cx)).max() <= 4 * 2.0 ** -24 * 4.0 and np.abs(rows[:, 7]).max() <= g.vx / 2 + 1e-6
        assert np.abs(rows[:, 8] - (rows[:, 1] - cy)).max() <= 4 * 2.0 ** -24 * 4.0 and np.abs(rows[:, 8]).max() <= g.vy / 2 + 1e-6


def test_rows_behind_the_count_are_never_read():
    for case in ("mixed-N4-c4", "over-N4-c9"):
        a, want = C.build(case), C.reference(case)
        n = R.live_rows(a["points"], a["offsets"])
        cut = R.pillarize(a["points"][:n], a["offsets"], a["grid"], a["max_points"], a["decorate"])
        same(cut, want)
        if n < len(a["points"]):
            _, _, keep = R.cells_of(a["points"][n:], a["grid"])
            assert keep.all()                                # reading them would have shown


# ---------------------------------------------------------------------------------------------- the Python side without a GPU
def test_pillar_grid_refuses_bad_ranges():
    import mcav.lib as L
    from pseudo_lidar import PillarGrid
    g = PillarGrid()
    assert (g.nx, g.ny) == (432, 496) == (R.make_grid().nx, R.make_grid().ny)
    small = PillarGrid(x=(-1.0, 2.5), y=(-1.0, 1.25), z=(-1.0, 1.0), size=(0.5, 0.25))
    assert (small.nx, small.ny) == (7, 9) and small.scalars() == (-1.0, -1.0, -1.0, 1.0, 0.5, 0.25)
    for kw in (dict(x=(1.0, 1.0)), dict(x=(2.0, 1.0)), dict(y=(0.0, float("nan"))), dict(z=(1.0, -3.0)), dict(z=(0.0, float("inf"))),
               dict(size=(0.0, 0.16)), dict(size=(0.16, -1.0)), dict(size=(float("nan"), 0.16)), dict(size=(1e-50, 0.16)),
               dict(x=(0.0, 1e39)), dict(x=(0.0, 69.12, 1.0)), dict(size=0.16), dict(x=(0.0, 0.01))):
        with pytest.raises(L.MCAVError):
            PillarGrid(**kw)


def test_pillarize_refuses_bad_arguments_without_a_gpu():
    import torch
    import mcav.lib as L
    from pseudo_lidar import CloudBatch, PillarGrid, pillarize
    pts, off = torch.zeros(8, 4), torch.zeros(2, dtype=torch.int32)
    bad = [dict(points=pts, offsets=off),                                             # CPU tensors
           dict(points=np.zeros((8, 4), F), offsets=off),
           dict(points=torch.zeros(8, 3), offsets=off), dict(points=torch.zeros(8), offsets=off),
           dict(points=torch.zeros(2, 8, 4), offsets=off),                            # wrong ranks
           dict(points=pts, offsets=torch.zeros(1, 2, dtype=torch.int32)), dict(points=pts, offsets=torch.zeros(1, dtype=torch.int32)),
           dict(points=pts, offsets=off, max_points=0), dict(points=pts, offsets=off, max_points=65),
           dict(points=pts, offsets=off, grid=(0.0, 69.12))]
    for kw in bad:
        with pytest.raises(L.MCAVError):
            pillarize(**kw)
    assert callable(CloudBatch.pillars) and PillarGrid().nx == 432


def test_inference_pillar_names_and_flags():
    import inference
    p = inference.Inference.pillar_path("out", "KITTI/2011_09_26/2011_09_26_drive_0001_sync/image_02/data/0000000003.png")
    assert p == os.path.join("out", "2011_09_26", "2011_09_26_drive_0001_sync", "pseudo_pillars", "data", "0000000003.npz")
    assert inference.Inference.cloud_path("out", "KITTI/2011_09_26/2011_09_26_drive_0001_sync/image_02/data/0000000003.png") == \
        os.path.join("out", "2011_09_26", "2011_09_26_drive_0001_sync", "pseudo_velodyne", "data", "0000000003.bin")
    with pytest.raises(ValueError):
        inference.Inference.pillar_path("out", "frame.png")
    assert callable(inference.Inference.pillars)
    parse = lambda argv: inference.pillar_arguments(inference.build_parser().parse_args(argv))
    base = ["--config", "c.yaml", "--checkpoint", "x.pth", "--out", "o"]
    assert parse(base) is None
    kw = parse(base + ["--pillars"])
    assert (kw["grid"].nx, kw["grid"].ny, kw["max_points"]) == (432, 496, 32)
    kw = parse(base + ["--pillars", "--pillar-size", "0.5", "0.25", "--pillar-points", "5", "--pillar-range", "-1", "2.5", "-1", "1.25", "-1", "1"])
    assert (kw["grid"].nx, kw["grid"].ny, kw["max_points"], kw["grid"].z) == (7, 9, 5, (-1.0, 1.0))
    import mcav.lib as L
    with pytest.raises(L.MCAVError):
        inference.main(base + ["--pillars", "--pillar-range", "1", "0", "-1", "1", "-1", "1"])      # refused before the config is read
