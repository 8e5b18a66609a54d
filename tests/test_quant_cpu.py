"""CPU: the soft-occupancy grid (include/mcav_depth.h: mcav_cloud_occupancy, mcav_cloud_occupancy_bwd; pseudo_lidar.occupancy).  The
restatement (tests/quant_ref.py) against its plain float64 formulation within the bound its docstring derives, and against six wrong
definitions that must each exceed it; the header csrc/quant_math.h compiled for the host against the restatement, bit for bit, on the
cases the GPU tests run (tests/quant_cases.py), once more as a stand-alone program under the address and undefined-behaviour sanitizers;
quant_exp against the float64 exponential and against C's fmaf; order-freeness; the refusals; what is exported, declared and bound;
what the Python side refuses without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quant_cases as C
import quant_ref as R
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "quant_hostcheck", "quant_hostcheck.cpp")
F = np.float32
SENTINEL = -7.0
ENTRIES = ("mcav_cloud_occupancy_workspace_bytes", "mcav_cloud_occupancy", "mcav_cloud_occupancy_bwd")


# ---------------------------------------------------------------------------------------------- restatement vs the float64 formulation
@pytest.mark.parametrize("case", C.CASES)
def test_restatement_within_the_derived_bound_of_float64(case):
    C.check_non_trivial(case)
    a, want = C.build(case), C.reference(case)
    f64 = R.occupancy_f64(**a)
    err = np.abs(want["canvas"].astype(np.float64) - f64["canvas"])
    assert (err <= f64["bound"]).all(), float((err / np.maximum(f64["bound"], 1e-300)).max())
    assert (f64["canvas"] > 0).sum() > 1000 and f64["bound"].max() < 1e-4 * max(f64["canvas"].max(), 1.0)
    b64 = R.occupancy_bwd_f64(a["points"], a["offsets"], C.upstream(case), a["grid"], a["sigma2"])
    got = C.reference_bwd(case)
    err = np.abs(got.astype(np.float64) - b64["d_points"])
    assert (err <= b64["bound"]).all(), float((err / np.maximum(b64["bound"], 1e-300)).max())
    assert not got[:, 3].any() and (got[:, :3] != 0).any(axis=1).sum() > 500


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_wrong_definitions_exceed_the_bound(mutant):
    """each mutant of the float64 formulation lies further from the restatement than the bound allows, somewhere: the bound tells them
    apart"""
    case = C.MUTANT_CASE
    a = C.build(case)
    right = R.occupancy_f64(**a)
    if mutant == "backward-without-2":
        right = R.occupancy_bwd_f64(a["points"], a["offsets"], C.upstream(case), a["grid"], a["sigma2"])
        wrong = R.occupancy_bwd_f64(a["points"], a["offsets"], C.upstream(case), a["grid"], a["sigma2"], mutant=mutant)
        err = np.abs(C.reference_bwd(case).astype(np.float64) - wrong["d_points"])
    else:
        wrong = R.occupancy_f64(mutant=mutant, **a)
        err = np.abs(C.reference(case)["canvas"].astype(np.float64) - wrong["canvas"])
    assert (err > 100 * right["bound"]).sum() > 10
    if mutant == "border-neighbours":                        # differs at the border only
        inner = (slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
        assert (err[inner] <= right["bound"][inner]).all()


# ---------------------------------------------------------------------------------------------- csrc/quant_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("quant_hostcheck") / "libquant_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, f, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_size_t
    lib.quant_host_workspace_bytes.restype = sz
    lib.quant_host_workspace_bytes.argtypes = [i, ll, i, i, i]
    lib.quant_host_occupancy.argtypes = [p, p, i, ll] + [f] * 6 + [i] * 3 + [f, p, p, p, sz]
    lib.quant_host_occupancy_bwd.argtypes = [p, p, p, p, i, ll] + [f] * 6 + [i] * 3 + [f, p]
    lib.quant_host_constants.argtypes = [p]
    lib.quant_host_exp_max_ulp.restype = lib.quant_host_exp_cut.restype = f
    lib.quant_host_exp.argtypes = [p, p, ll]
    lib.quant_host_cell.argtypes = [f] * 9 + [i] * 3 + [p]
    lib.quant_host_exp_scan.restype = ctypes.c_double
    lib.quant_host_exp_scan.argtypes = [ctypes.c_uint32] * 3 + [p]
    return lib


def aligned(shape, dtype, fill, align=256, offset=0):
    """an array whose first byte sits `offset` behind a multiple of `align`"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.empty(n + 2 * align, np.uint8)
    start = (-raw.ctypes.data) % align + offset
    out = raw[start:start + n].view(dtype).reshape(shape)
    out[...] = fill
    return out


def host_forward(host, a, record=True, **change):
    pts, off, g = np.ascontiguousarray(a["points"]), np.ascontiguousarray(a["offsets"]), a["grid"]
    B, n_max = len(off) - 1, len(pts)
    arg = dict(points=aligned(pts.shape, F, pts), offsets=off, B=B, n_max=n_max, x0=g.x0, y0=g.y0, z0=g.z0, vx=g.vx, vy=g.vy, vz=g.vz, nx=g.nx,
               ny=g.ny, nz=g.nz, sigma2=a["sigma2"], canvas=aligned((B, g.nz, g.ny, g.nx), F, SENTINEL),
               count=np.full(n_max, -7, np.int32) if record else None)
    nbytes = host.quant_host_workspace_bytes(B, n_max, g.nz, g.ny, g.nx)
    arg.update(ws=aligned((max(nbytes, 1),), np.uint8, 0), nbytes=nbytes)
    arg.update(change)
    ptr = lambda v: v if v is None or isinstance(v, int) else v.ctypes.data
    rc = host.quant_host_occupancy(ptr(arg["points"]), ptr(arg["offsets"]), arg["B"], arg["n_max"], arg["x0"], arg["y0"], arg["z0"], arg["vx"],
                                   arg["vy"], arg["vz"], arg["nx"], arg["ny"], arg["nz"], arg["sigma2"], ptr(arg["canvas"]), ptr(arg["count"]),
                                   ptr(arg["ws"]), arg["nbytes"])
    return rc, arg


def host_backward(host, a, recorded, upstream, **change):
    pts, off, g = np.ascontiguousarray(a["points"]), np.ascontiguousarray(a["offsets"]), a["grid"]
    B, n_max = len(off) - 1, len(pts)
    arg = dict(points=aligned(pts.shape, F, pts), offsets=off, count=np.ascontiguousarray(recorded), d_canvas=np.ascontiguousarray(upstream), B=B,
               n_max=n_max, x0=g.x0, y0=g.y0, z0=g.z0, vx=g.vx, vy=g.vy, vz=g.vz, nx=g.nx, ny=g.ny, nz=g.nz, sigma2=a["sigma2"],
               d_points=aligned((n_max, 4), F, SENTINEL))
    arg.update(change)
    ptr = lambda v: v if v is None or isinstance(v, int) else v.ctypes.data
    rc = host.quant_host_occupancy_bwd(ptr(arg["points"]), ptr(arg["offsets"]), ptr(arg["count"]), ptr(arg["d_canvas"]), arg["B"], arg["n_max"],
                                       arg["x0"], arg["y0"], arg["z0"], arg["vx"], arg["vy"], arg["vz"], arg["nx"], arg["ny"], arg["nz"],
                                       arg["sigma2"], ptr(arg["d_points"]))
    return rc, arg


def test_tile_constants_are_the_headers(host):
    out = np.zeros(4, np.int32)
    host.quant_host_constants(out.ctypes.data)
    assert out.tolist() == [C.TILE_X, C.TILE_Y, C.MAX_NZ, 1024]
    assert host.quant_host_exp_max_ulp() == R.QEXP_MAX_ULP <= 2.0 and host.quant_host_exp_cut() == R.QEXP_CUT


@pytest.mark.parametrize("case", C.CASES)
def test_header_matches_restatement(host, case):
    a, want = C.build(case), C.reference(case)
    n = len(want["point_count"])
    rc, arg = host_forward(host, a)
    assert rc == 0
    C.same_bits(arg["canvas"], want["canvas"])
    assert np.array_equal(arg["count"][:n], want["point_count"]) and (arg["count"][n:] == -7).all()
    rc, plain = host_forward(host, a, record=False)
    assert rc == 0
    C.same_bits(plain["canvas"], want["canvas"])
    full = np.full(len(a["points"]), 12345, np.int32)        # rows behind n hold rubbish: never read
    full[:n] = want["point_count"]
    rc, back = host_backward(host, a, full, C.upstream(case))
    assert rc == 0
    C.same_bits(back["d_points"], C.reference_bwd(case))
    assert not back["d_points"][n:].view(np.uint32).any()    # every row written: +0.0 behind the count


def test_cells_on_faces_and_special_values(host):
    g = C.grid_of("odd", 5)
    nan, inf = np.nan, np.inf
    table = [((-1.0, -1.0, -1.0), (0, 0, 0)), ((-0.0, -0.0, -0.75), (8, 4, 1)), ((-0.875, 0, 0), (1, 4, 4)), ((16.375, 0, 0), None),
             ((16.37, 1.74, 0.24), (138, 10, 4)), ((0, 1.75, 0), None),
             ((np.nextafter(F(16.375), F(0)), 0, 0), (138, 4, 4)),
             ((0, np.nextafter(F(1.75), F(0)), 0), None),     # y - y0 rounds up to 2.75 in float32: the rule's own rounding drops it
             ((0, 0, 0.25), None), ((np.nextafter(F(-1), F(-2)), 0, 0), None), ((nan, 0, 0), None), ((0, nan, 0), None), ((0, 0, nan), None),
             ((inf, 0, 0), None), ((0, -inf, 0), None), ((0, 0, inf), None), ((3e38, 0, 0), None)]
    for p, cell in table:
        out = np.full(3, -1, np.int32)
        kept = host.quant_host_cell(p[0], p[1], p[2], g.x0, g.y0, g.z0, g.vx, g.vy, g.vz, g.nx, g.ny, g.nz, out.ctypes.data)
        ix, iy, iz, keep = R.cells_of(np.array([p + (0,)], F), g)
        assert bool(kept) == bool(keep[0]) == (cell is not None), p
        if cell is not None:
            assert tuple(out) == cell == (ix[0], iy[0], iz[0]), (p, tuple(out))


# ---------------------------------------------------------------------------------------------- quant_exp
def test_quant_exp_bits_and_ulp_bound(host):
    """The header's quant_exp is the restatement's (numpy with an emulated fmaf: so it is held to C's fmaf) bit for bit, on 300 000
    arguments: random ones over [-90, 0], the first and last 2000 floats of the range, around the cut-off and the worst argument.  Its
    error against the float64 exponential stays within the header's QEXP_MAX_ULP on a stated subset -- every 509th float32 of
    [-87, -0] (2.2 million arguments) and the 2^17 floats on either side of the exhaustive scan's worst argument -- which the exhaustive
    scan (`quant_hostcheck --exp-ulp`, the stand-alone build) covers in full."""
    rng = np.random.RandomState(11)
    cut, worst = np.array([R.QEXP_CUT], F).view(np.uint32)[0], np.array([float.fromhex("-0x1.79082cp+2")], F).view(np.uint32)[0]
    bits = np.concatenate([np.arange(0x80000000, 0x80000000 + 2000), np.arange(cut - 2000, cut + 2000), np.arange(worst - 2000, worst + 2000),
                           [0, 0x7fc00000, 0xffc00000, 0xff800000]]).astype(np.uint32)
    t = np.concatenate([bits.view(F), -rng.uniform(0, 90, 290000).astype(F), -(10.0 ** rng.uniform(-30, 0, 5000)).astype(F)])
    got = np.empty_like(t)
    host.quant_host_exp(t.ctypes.data, got.ctypes.data, len(t))
    C.same_bits(got, R.quant_exp(t))
    with np.errstate(invalid="ignore"):
        dead = ~(t >= R.QEXP_CUT)
    assert dead.sum() > 1000 and not got[dead].view(np.uint32).any() and (got[~dead] >= F(2.0 ** -126)).all() and got[~dead].max() == 1.0
    live = t[~dead].astype(np.float64)
    want = np.exp(live)
    ulp = 2.0 ** (np.floor(np.log2(want)) - 23)
    assert (np.abs(got[~dead].astype(np.float64) - want) / ulp).max() <= R.QEXP_MAX_ULP
    at = ctypes.c_float(0)
    assert 0.8 < host.quant_host_exp_scan(0x80000000, int(cut), 509, ctypes.addressof(at)) <= R.QEXP_MAX_ULP
    near = host.quant_host_exp_scan(int(worst) - (1 << 17), int(worst) + (1 << 17), 1, ctypes.addressof(at))
    assert abs(near - 0.937081) < 1e-6 and near <= R.QEXP_MAX_ULP and at.value == float.fromhex("-0x1.79082cp+2")


# ---------------------------------------------------------------------------------------------- properties of the definition
@pytest.mark.parametrize("case", ["mixed-odd-z5-cell", "pair-wide-z5-sharp"])
def test_order_inside_an_image_changes_no_byte(host, case):
    a, want = C.build(case), C.reference(case)
    pts, off = a["points"].copy(), a["offsets"]
    rng = np.random.RandomState(5)
    perms = []
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), min(int(off[b + 1]), len(pts))
        perms.append(lo + rng.permutation(hi - lo))
        pts[lo:hi] = a["points"][perms[-1]]
    perm = np.concatenate(perms)
    assert (perm != np.arange(len(perm))).sum() > 1000
    moved = dict(a, points=pts)
    C.same_bits(R.occupancy(**moved)["canvas"], want["canvas"])
    rc, arg = host_forward(host, moved)
    assert rc == 0
    C.same_bits(arg["canvas"], want["canvas"])
    assert np.array_equal(arg["count"][:len(perm)], want["point_count"][perm])


def test_rows_behind_the_count_are_never_read(host):
    a, want = C.build("mixed-odd-z5-cell"), C.reference("mixed-odd-z5-cell")
    n = len(want["point_count"])
    pts = a["points"].copy()
    pts[n:] = C.in_cell(np.random.RandomState(3), a["grid"], 20, 5, 2, len(pts) - n)        # reading them would show
    rc, arg = host_forward(host, dict(a, points=pts))
    assert rc == 0 and n < len(pts)
    C.same_bits(arg["canvas"], want["canvas"])
    assert R.occupancy(**dict(a, points=pts[:n]))["canvas"].tobytes() == want["canvas"].tobytes()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(host):
    a = C.build("mixed-wide-z1-cell")
    g = a["grid"]
    nan, inf = float("nan"), float("inf")
    rc, ok = host_forward(host, a)
    assert rc == 0
    off4 = lambda v: v.ctypes.data + 4
    bad = [dict(points=None), dict(offsets=None), dict(canvas=None), dict(ws=None), dict(B=0), dict(B=-1), dict(B=65536), dict(n_max=-1),
           dict(n_max=1 << 31), dict(nx=0), dict(ny=0), dict(nz=0), dict(nz=65), dict(vx=0.0), dict(vy=-1.0), dict(vz=nan), dict(vx=inf),
           dict(x0=nan), dict(y0=inf), dict(z0=-inf), dict(sigma2=0.0), dict(sigma2=-0.01), dict(sigma2=nan), dict(sigma2=inf),
           dict(nx=1 << 15, ny=1 << 15), dict(nx=1 << 13, ny=1 << 13, nz=11),                # B * ny * nx, B * nz * ny * nx >= 2^31
           dict(points=off4(ok["points"])), dict(canvas=off4(ok["canvas"])), dict(ws=off4(ok["ws"])), dict(count=ok["count"].ctypes.data + 2)]
    for change in bad:
        rc, arg = host_forward(host, a, **change)
        assert rc == -1, change
        for name in ("canvas", "count"):
            if not isinstance(arg[name], (int, type(None))):
                assert (arg[name] == (SENTINEL if name == "canvas" else -7)).all(), change
    rc, arg = host_forward(host, a, nbytes=ok["nbytes"] - 1)
    assert rc == -2 and (arg["canvas"] == SENTINEL).all() and (arg["count"] == -7).all()
    count, up = C.reference("mixed-wide-z1-cell")["point_count"], C.upstream("mixed-wide-z1-cell")
    full = np.zeros(len(a["points"]), np.int32)
    full[:len(count)] = count
    rc, fine = host_backward(host, a, full, up)
    assert rc == 0
    for change in [dict(points=None), dict(offsets=None), dict(count=None), dict(d_canvas=None), dict(d_points=None), dict(B=0), dict(nz=65),
                   dict(nx=0), dict(vy=0.0), dict(sigma2=nan), dict(sigma2=0.0), dict(n_max=-1), dict(nx=1 << 15, ny=1 << 15),
                   dict(points=off4(fine["points"])), dict(d_points=off4(fine["d_points"])), dict(d_canvas=up.ctypes.data + 2)]:
        rc, arg = host_backward(host, a, full, up, **change)
        assert rc == -1, change
        if not isinstance(arg["d_points"], (int, type(None))):
            assert (arg["d_points"] == SENTINEL).all(), change


def test_workspace_formula(host):
    import mcav.lib as L
    import pseudo_lidar  # noqa: F401
    B, n_max, nz, ny, nx = 3, 5000, 35, 800, 700
    up = lambda v: (v + 255) // 256 * 256
    M = B * ny * nx
    want = up(4 * (M + 1)) + up(4 * ((M + 1023) // 1024)) + up(8 * n_max) + 2 * up(4 * n_max)
    assert host.quant_host_workspace_bytes(B, n_max, nz, ny, nx) == want == L.lib().mcav_cloud_occupancy_workspace_bytes(B, n_max, nz, ny, nx)
    for refused in ((0, 1, 1, 1, 1), (1, -1, 1, 1, 1), (1, 1, 65, 1, 1), (1, 1, 0, 1, 1), (4, 1, 64, 4096, 4096), (65536, 1, 1, 1, 1)):
        assert host.quant_host_workspace_bytes(*refused) == 0 == L.lib().mcav_cloud_occupancy_workspace_bytes(*refused)


# ---------------------------------------------------------------------------------------------- the stand-alone program
def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the hardest case (a cut last image, rows that
    are no multiple of 4, every neighbour term alive) with and without the record: every buffer is exactly as large as the call may
    touch, and a finding ends the program with a non-zero status."""
    exe = str(tmp_path / "quant_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      "-DQUANT_STANDALONE"]) + ["-o", exe])
    a, want = C.build(C.HARDEST), C.reference(C.HARDEST)
    g, B, n_max = a["grid"], len(a["offsets"]) - 1, len(a["points"])
    up = lambda v: (v + 255) // 256 * 256
    M = B * g.ny * g.nx
    nbytes = up(4 * (M + 1)) + up(4 * ((M + 1023) // 1024)) + up(8 * n_max) + 2 * up(4 * n_max)
    for record in (1, 0):
        head = np.array([B, n_max, g.nx, g.ny, g.nz, record, nbytes, 0], np.int64)
        with open(str(tmp_path / "in.bin"), "wb") as f:
            for part in (head, np.array(list(g[:6]) + [a["sigma2"], 0], F), a["offsets"], a["points"], C.upstream(C.HARDEST)):
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        raw = open(str(tmp_path / "out.bin"), "rb").read()
        assert np.frombuffer(raw, np.int32, 2).tolist() == [0, 0]
        canvas = np.frombuffer(raw, F, want["canvas"].size, 8).reshape(want["canvas"].shape)
        at = 8 + 4 * canvas.size
        count = np.frombuffer(raw, np.int32, n_max, at)
        d_points = np.frombuffer(raw, F, 4 * n_max, at + 4 * n_max).reshape(n_max, 4)
        assert at + 20 * n_max == len(raw)
        C.same_bits(canvas, want["canvas"])
        if record:
            assert np.array_equal(count, want["point_count"])
            C.same_bits(d_points, C.reference_bwd(C.HARDEST))
        else:
            assert (count == -1).all() and (d_points.view(np.uint32) == 0xffffffff).all()


# ---------------------------------------------------------------------------------------------- exported, declared, bound
def test_new_entries_are_exported_declared_and_bound():
    import mcav.lib as L
    import pseudo_lidar  # noqa: F401
    header = open(os.path.join(REPO, "include", "mcav_depth.h")).read()
    handle = ctypes.CDLL(os.path.join(PKG, "mcav", "libmcav_depth.so"))
    for name in ENTRIES:
        assert name + "(" in header and hasattr(handle, name) and name in L._SIGNATURES, name
        assert hasattr(L.lib(), name)
    assert len(L._SIGNATURES["mcav_cloud_occupancy"][1]) == 19 and len(L._SIGNATURES["mcav_cloud_occupancy_bwd"][1]) == 18


# ---------------------------------------------------------------------------------------------- the Python side without a GPU
def test_voxel_grid_refuses_bad_ranges():
    import mcav.lib as L
    from pseudo_lidar import VoxelGrid
    g, ref = VoxelGrid(), R.make_grid()
    assert (g.nx, g.ny, g.nz) == (700, 800, 35) == (ref.nx, ref.ny, ref.nz)
    small = VoxelGrid(x=(-1.0, 16.375), y=(-1.0, 1.75), z=(-1.0, 0.25), size=(0.125, 0.25, 0.25))
    assert (small.nx, small.ny, small.nz) == (139, 11, 5) and small.scalars() == (-1.0, -1.0, -1.0, 0.125, 0.25, 0.25, 139, 11, 5)
    for kw in (dict(x=(1.0, 1.0)), dict(x=(2.0, 1.0)), dict(y=(0.0, float("nan"))), dict(z=(1.0, -3.0)), dict(z=(0.0, float("inf"))),
               dict(size=(0.0, 0.1, 0.1)), dict(size=(0.1, -1.0, 0.1)), dict(size=(0.1, 0.1, float("nan"))), dict(size=(0.1, 0.1)),
               dict(size=0.1), dict(x=(0.0, 1e39)), dict(x=(0.0, 70.0, 1.0)), dict(z=(-2.5, 4.0)), dict(z=(0.0, 0.01)),
               dict(x=(0.0, 7000.0), y=(-4000.0, 4000.0), size=(0.01, 0.01, 0.1))):
        with pytest.raises(L.MCAVError):
            VoxelGrid(**kw)


def test_occupancy_refuses_bad_arguments_without_a_gpu():
    import torch
    import inference
    import mcav.lib as L
    from pseudo_lidar import CloudBatch, OccupancyBatch, PillarGrid, occupancy, occupancy_backward
    pts, off = torch.zeros(8, 4), torch.zeros(2, dtype=torch.int32)
    bad = [dict(points=pts, offsets=off),                                             # CPU tensors
           dict(points=np.zeros((8, 4), F), offsets=off),
           dict(points=torch.zeros(8, 3), offsets=off), dict(points=torch.zeros(8), offsets=off),
           dict(points=pts, offsets=torch.zeros(1, 2, dtype=torch.int32)), dict(points=pts, offsets=torch.zeros(1, dtype=torch.int32)),
           dict(points=pts, offsets=off, sigma2=0.0), dict(points=pts, offsets=off, sigma2=float("nan")),
           dict(points=pts, offsets=off, grid=PillarGrid())]
    for kw in bad:
        with pytest.raises(L.MCAVError):
            occupancy(**kw)
    for record in (None, {}, OccupancyBatch.__new__(OccupancyBatch)):
        if isinstance(record, OccupancyBatch):
            record._fwd = None
        with pytest.raises(L.MCAVError):
            occupancy_backward(record, torch.zeros(1, 1, 1, 1))
    assert callable(CloudBatch.occupancy) and callable(inference.Inference.occupancy)
