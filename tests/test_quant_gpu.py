"""GPU: the soft-occupancy grid (include/mcav_depth.h: mcav_cloud_occupancy, mcav_cloud_occupancy_bwd; pseudo_lidar.occupancy,
occupancy_backward) against the restatement (tests/quant_ref.py), bit for bit, on the cases of tests/quant_cases.py: canvas, point_count
and d_points with sentinels around and behind every buffer, a second run, the call without provenance; graph capture and replay on new
contents of the raw calls and of the autograd path; the whole chain disparity -> project_batch -> occupancy -> a weighted sum ->
disp.grad against the chained restatements; the C ABI's refusals."""
import numpy as np
import pytest
import torch

import pl_bwd_cases as PC
import pl_bwd_ref as BR
import quant_cases as C
import quant_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -7.0
COUNT_SENTINEL = -12345
GUARD = 64                                                   # elements in front of and behind a guarded buffer: 256 bytes


def dev(v, dtype=None):
    return torch.from_numpy(np.array(v, dtype or v.dtype)).to(DEV)


def guarded(shape, dtype, fill):
    """-> (a contiguous view of `shape` inside a buffer with GUARD elements of `fill` on either side, the whole buffer)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n].view(shape), whole


def guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def voxel_grid(g):
    from pseudo_lidar import VoxelGrid
    lo = [float(g.x0), float(g.y0), float(g.z0)]
    size = [float(g.vx), float(g.vy), float(g.vz)]
    vg = VoxelGrid(x=(lo[0], lo[0] + g.nx * size[0]), y=(lo[1], lo[1] + g.ny * size[1]), z=(lo[2], lo[2] + g.nz * size[2]), size=size)
    assert (vg.nx, vg.ny, vg.nz) == (g.nx, g.ny, g.nz)
    return vg


def holder(a, canvas_fill=SENTINEL):
    """an OccupancyBatch whose canvas and point_count sit between guards, full of sentinels"""
    from pseudo_lidar import OccupancyBatch
    g, B = a["grid"], len(a["offsets"]) - 1
    ob = OccupancyBatch(B, voxel_grid(g), DEV)
    ob.canvas, whole_canvas = guarded((B, g.nz, g.ny, g.nx), torch.float32, canvas_fill)
    ob.point_count, whole_count = guarded((len(a["points"]),), torch.int32, COUNT_SENTINEL)
    return ob, whole_canvas, whole_count


# ---------------------------------------------------------------------------------------------- every case, forward and backward
@pytest.mark.parametrize("case", C.CASES)
def test_canvas_counts_and_gradient_match_restatement(case):
    from pseudo_lidar import occupancy, occupancy_backward
    a, want, want_bwd = C.build(case), C.reference(case), C.reference_bwd(case)
    C.check_non_trivial(case)
    n, n_max = len(want["point_count"]), len(a["points"])
    pts, off = dev(a["points"]), dev(a["offsets"])
    kw = dict(grid=voxel_grid(a["grid"]), sigma2=a["sigma2"])
    ob, whole_canvas, whole_count = holder(a)
    count = ob.point_count
    canvas = occupancy(pts, off, out=ob, provenance=True, **kw)
    assert canvas is ob.canvas and canvas.grad_fn is None and ob.point_count is count
    C.same_bits(canvas.cpu().numpy(), want["canvas"])        # every element written: no sentinel is left
    assert np.array_equal(count[:n].cpu().numpy(), want["point_count"]) and bool((count[n:] == COUNT_SENTINEL).all())
    assert guards_intact(whole_canvas, SENTINEL) and guards_intact(whole_count, COUNT_SENTINEL)

    d_points, whole_d = guarded((n_max, 4), torch.float32, SENTINEL)
    got = occupancy_backward(ob, dev(C.upstream(case)), out=d_points)
    assert got is d_points
    C.same_bits(d_points.cpu().numpy(), want_bwd)            # every row written, +0.0 behind the count
    assert guards_intact(whole_d, SENTINEL)
    again = occupancy_backward(ob._fwd, dev(C.upstream(case)))
    assert again.data_ptr() != d_points.data_ptr() and torch.equal(again.view(torch.int32), d_points.view(torch.int32))

    # a second run into other buffers (NaN-filled this time) and the call without provenance: the same bytes
    second, whole_second, _ = holder(a, canvas_fill=float("nan"))
    occupancy(pts, off, out=second, provenance=True, **kw)
    assert torch.equal(second.canvas.view(torch.int32), canvas.view(torch.int32)) and torch.equal(second.point_count[:n], count[:n])
    plain = occupancy(pts, off, **kw)
    assert plain.data_ptr() != canvas.data_ptr() and torch.equal(plain.view(torch.int32), canvas.view(torch.int32))
    third, _, whole_third = holder(a)
    occupancy(pts, off, out=third, **kw)
    assert third.point_count is None and third._fwd is None and bool((whole_third == COUNT_SENTINEL).all())
    assert torch.equal(third.canvas.view(torch.int32), canvas.view(torch.int32))


def test_python_side_refusals_on_the_gpu():
    from mcav import lib as L
    from pseudo_lidar import OccupancyBatch, occupancy, occupancy_backward
    g = voxel_grid(C.grid_of("wide", 5))
    pts, off = torch.zeros(8, 4, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    canvas = occupancy(pts, off, grid=g, sigma2=0.02)              # no live row: written, all +0.0
    assert tuple(canvas.shape) == (3, g.nz, g.ny, g.nx) and not bool(canvas.view(torch.int32).any())
    plain = OccupancyBatch(3, g, DEV)
    occupancy(pts, off, grid=g, out=plain)
    for call in (lambda: occupancy(torch.empty(0, 4, device=DEV), off, grid=g),                       # no rows
                 lambda: occupancy(pts, off.to(torch.int64), grid=g),
                 lambda: occupancy(pts, off, grid=g, out=OccupancyBatch(2, g, DEV)),                  # another batch size
                 lambda: occupancy(pts, off, grid=g, out=canvas),
                 lambda: occupancy_backward(plain, torch.zeros_like(canvas)),                          # no provenance
                 lambda: occupancy(pts[:, :3], off, grid=g)):
        with pytest.raises(L.MCAVError):
            call()


# ---------------------------------------------------------------------------------------------- capture and replay
def shifted(a):
    """the case's cloud moved by a fraction of a cell: other cells, other counts, the same offsets"""
    pts = a["points"].copy()
    pts[:, 0] += F(0.3)
    pts[:, 1] -= F(0.1)
    pts[:, 2] += F(0.05)
    return dict(a, points=pts)


def test_raw_calls_capture_and_replay_on_new_contents():
    from pseudo_lidar import occupancy, occupancy_backward
    case = "pair-wide-z5-sharp"
    a = C.build(case)
    b = dict(shifted(a), sigma2=a["sigma2"])
    kw = dict(grid=voxel_grid(a["grid"]), sigma2=a["sigma2"])
    pts, off, up = dev(a["points"]), dev(a["offsets"]), dev(C.upstream(case))
    ob, whole_canvas, whole_count = holder(a)
    d_points, whole_d = guarded((len(a["points"]), 4), torch.float32, SENTINEL)

    def chain():
        occupancy(pts, off, out=ob, provenance=True, **kw)
        occupancy_backward(ob, up, out=d_points)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()                                                    # warm-up: the workspace exists
    torch.cuda.current_stream().wait_stream(s)
    first = ob.canvas.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    pts.copy_(dev(b["points"]))
    other_up = np.random.RandomState(8).standard_normal(C.upstream(case).shape).astype(F)
    up.copy_(dev(other_up))
    ob.canvas.fill_(SENTINEL); d_points.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    want = R.occupancy(**b)
    n = len(want["point_count"])
    assert not torch.equal(ob.canvas, first)
    C.same_bits(ob.canvas.cpu().numpy(), want["canvas"])
    assert np.array_equal(ob.point_count[:n].cpu().numpy(), want["point_count"])
    C.same_bits(d_points.cpu().numpy(), R.occupancy_bwd(b["points"], b["offsets"], want["point_count"], other_up, b["grid"], b["sigma2"]))
    assert guards_intact(whole_canvas, SENTINEL) and guards_intact(whole_count, COUNT_SENTINEL) and guards_intact(whole_d, SENTINEL)


def test_autograd_path_captures_and_replays():
    """points that require a gradient -> occupancy(out=) -> (canvas * fixed).sum().backward(), captured once and replayed after the points
    changed in place: points.grad holds the restatement's bytes for the new contents"""
    from pseudo_lidar import occupancy
    case = "mixed-odd-z5-cell"
    a = C.build(case)
    b = shifted(a)
    kw = dict(grid=voxel_grid(a["grid"]), sigma2=a["sigma2"])
    off, fixed = dev(a["offsets"]), dev(C.upstream(case))
    ob, _, _ = holder(a)

    def step(points):
        (occupancy(points, off, out=ob, **kw) * fixed).sum().backward()

    pts = dev(a["points"]).requires_grad_(True)
    warm = pts.detach().clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm)
    torch.cuda.current_stream().wait_stream(s)
    C.same_bits(warm.grad.cpu().numpy(), C.reference_bwd(case))
    assert pts.grad is None and ob.canvas.grad_fn is not None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(pts)
    with torch.no_grad():
        pts.copy_(dev(b["points"]))
    pts.grad.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    want = R.occupancy(**b)
    C.same_bits(ob.canvas.detach().cpu().numpy(), want["canvas"])
    C.same_bits(pts.grad.cpu().numpy(), R.occupancy_bwd(b["points"], b["offsets"], want["point_count"], C.upstream(case), b["grid"], b["sigma2"]))


def test_stale_backward_is_refused_and_plain_calls_carry_no_graph():
    from mcav import lib as L
    from pseudo_lidar import occupancy
    a = C.build("mixed-wide-z1-cell")
    kw = dict(grid=voxel_grid(a["grid"]), sigma2=a["sigma2"])
    pts, off = dev(a["points"]), dev(a["offsets"])
    ob, _, _ = holder(a)
    ob.point_count = None
    live = pts.clone().requires_grad_(True)
    stale = occupancy(live, off, out=ob, **kw).sum()
    assert ob.point_count is not None and ob.canvas.grad_fn is not None
    occupancy(live, off, out=ob, **kw)
    with pytest.raises(L.MCAVError, match="again"):
        stale.backward()
    with torch.no_grad():
        quiet = occupancy(live, off, **kw)
    assert quiet.grad_fn is None and not quiet.requires_grad
    ptr = ob.canvas.data_ptr()
    occupancy(pts, off, out=ob, **kw)
    assert ob.canvas.grad_fn is None and ob._fwd is None and ob.canvas.data_ptr() == ptr


# ---------------------------------------------------------------------------------------------- disparity -> canvas under autograd
CHAIN_GRID = R.make_grid(x=(0.0, 48.0), y=(-16.0, 16.0), z=(-3.0, 1.0), size=(1.0, 1.0, 0.5))      # 48 x 32 x 8 cells over the scene
CHAIN_SIGMA2 = 1.0


def project(a, m):
    """pl_bwd_cases' arguments -> PseudoLiDAR.project_batch"""
    from pseudo_lidar import BeamTables, PseudoLiDAR
    assert a["scales"] is None
    pl = PseudoLiDAR.from_matrices(a["T"][0], a["P"][0], a["sparsity"])
    return pl.project_batch(m, sizes=a["sizes"], P=a["P"], T=a["T"], input=a["input"], scale=a["scale"], max_height=a["max_height"],
                            max_depth=None if np.isinf(a["max_depth"]) else a["max_depth"],
                            beams=None if a["beams"] is None else BeamTables(*a["beams"]), padded=(a["Hg"], a["Wg"]))


@pytest.mark.parametrize("case", ["odd-dense", "odd-beams8x16"])
def test_disparity_gradient_through_the_whole_chain(case):
    """a leaf disparity -> project_batch -> .occupancy() -> (canvas * fixed).sum().backward(): disp.grad is quant_ref's backward chained
    into pl_bwd_ref's projection backward, bit for bit"""
    a = PC.project_build(case)
    B, h, w = a["m"].shape
    disp = dev(a["m"])[:, None].clone().requires_grad_(True)
    cloud = project(a, disp)
    assert cloud.points.grad_fn is not None and cloud.pixels is not None
    canvas = cloud.occupancy(grid=voxel_grid(CHAIN_GRID), sigma2=CHAIN_SIGMA2)
    assert canvas.grad_fn is not None and tuple(canvas.shape) == (B, CHAIN_GRID.nz, CHAIN_GRID.ny, CHAIN_GRID.nx)
    fixed = np.random.RandomState(77).standard_normal(tuple(canvas.shape)).astype(F)
    (canvas * dev(fixed)).sum().backward()
    assert disp.grad is not None and tuple(disp.grad.shape) == (B, 1, h, w)

    fwd = BR.project_forward(**a)
    n = len(fwd["pixels"])
    cap = cloud.points.shape[0]
    C.same_bits(cloud.points[:n].detach().cpu().numpy(), fwd["cloud"])
    rows = np.zeros((cap, 4), F)
    rows[:n] = fwd["cloud"]
    occ = R.occupancy(rows, fwd["offsets"], CHAIN_GRID, CHAIN_SIGMA2)
    C.same_bits(canvas.detach().cpu().numpy(), occ["canvas"])
    d_points = R.occupancy_bwd(rows, fwd["offsets"], occ["point_count"], fixed, CHAIN_GRID, CHAIN_SIGMA2)
    want = BR.project_bwd(d_points, fwd, **a)["d_m"]
    assert (occ["point_count"] > 0).sum() >= 100 and (d_points[:n, :3] != 0).any() and (want != 0).reshape(B, -1).any(axis=1).all()
    C.same_bits(disp.grad[:, 0].cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_refuses_bad_arguments():
    """return codes only, nothing launched: the sentinels stay"""
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401
    hl = L.lib()
    B, n_max, nx, ny, nz = 2, 16, 70, 9, 3
    nan, inf = float("nan"), float("inf")
    nbytes = hl.mcav_cloud_occupancy_workspace_bytes(B, n_max, nz, ny, nx)
    assert nbytes > 0
    t = dict(points=torch.zeros(n_max + 1, 4, device=DEV), offsets=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
             canvas=torch.full((B * nz * ny * nx + 4,), SENTINEL, device=DEV), count=torch.full((n_max + 1,), COUNT_SENTINEL, dtype=torch.int32, device=DEV),
             ws=torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV), d_canvas=torch.zeros(B * nz * ny * nx + 1, device=DEV),
             d_points=torch.full((n_max + 1, 4), SENTINEL, device=DEV))
    base = dict({k: L.ptr(v) for k, v in t.items()}, B=B, n_max=n_max, x0=0.0, y0=0.0, z0=0.0, vx=1.0, vy=1.0, vz=1.0, nx=nx, ny=ny, nz=nz,
                sigma2=1.0, nbytes=nbytes)
    grid = ("x0", "y0", "z0", "vx", "vy", "vz", "nx", "ny", "nz", "sigma2")

    def forward(**kw):
        arg = dict(base, **kw)
        return hl.mcav_cloud_occupancy(*[arg[k] for k in ("points", "offsets", "B", "n_max") + grid + ("canvas", "count", "ws", "nbytes")], L.stream())

    def backward(**kw):
        arg = dict(base, **kw)
        return hl.mcav_cloud_occupancy_bwd(*[arg[k] for k in ("points", "offsets", "count", "d_canvas", "B", "n_max") + grid + ("d_points",)],
                                           L.stream())

    shift = lambda name, by: L.c_p(t[name].data_ptr() + by)
    shared = [dict(points=L.c_p(0)), dict(offsets=L.c_p(0)), dict(B=0), dict(B=65536), dict(n_max=-1), dict(n_max=1 << 31), dict(nx=0), dict(ny=0),
              dict(nz=0), dict(nz=65), dict(vx=0.0), dict(vy=-1.0), dict(vz=nan), dict(vx=inf), dict(x0=nan), dict(z0=inf), dict(sigma2=0.0),
              dict(sigma2=nan), dict(sigma2=inf), dict(sigma2=-1.0), dict(nx=1 << 15, ny=1 << 15), dict(nx=1 << 13, ny=1 << 13, nz=17),
              dict(points=shift("points", 4)), dict(offsets=shift("offsets", 2))]
    for kw in shared + [dict(canvas=L.c_p(0)), dict(ws=L.c_p(0)), dict(canvas=shift("canvas", 4)), dict(ws=shift("ws", 8)), dict(count=shift("count", 2))]:
        assert forward(**kw) == -1, kw
    assert forward(nbytes=nbytes - 1) == -2
    for kw in shared + [dict(count=L.c_p(0)), dict(d_canvas=L.c_p(0)), dict(d_points=L.c_p(0)), dict(d_points=shift("d_points", 4)),
                        dict(d_canvas=shift("d_canvas", 2)), dict(count=shift("count", 2))]:
        assert backward(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((t["canvas"] == SENTINEL).all()) and bool((t["count"] == COUNT_SENTINEL).all()) and bool((t["d_points"] == SENTINEL).all())
    assert forward() == 0 and forward(count=L.c_p(0)) == 0 and backward() == 0      # an empty cloud: every element and row written, +0.0
    torch.cuda.synchronize()
    assert not bool(t["canvas"][:-4].view(torch.int32).any()) and bool((t["canvas"][-4:] == SENTINEL).all())
    assert not bool(t["d_points"][:n_max].view(torch.int32).any()) and bool((t["d_points"][n_max:] == SENTINEL).all())
    assert bool((t["count"] == COUNT_SENTINEL).all())              # offsets[B] = 0: no row is live, none is written
