"""GPU: the pillar voxeliser (include/mcav_depth.h: mcav_pillarize, pseudo_lidar.pillarize, CloudBatch.pillars, Inference.pillars) against
its restatement (tests/pillar_ref.py), bit for bit and with nothing left out, on the cases of tests/pillar_cases.py; sentinels in the rows
that must stay unwritten; repeatability; graph capture and replay on new contents; the real shape behind project_batch; the export."""
import os

import numpy as np
import pytest
import torch

import pillar_cases as C
import pillar_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -7.0


def product_grid(g):
    from pseudo_lidar import PillarGrid
    pg = PillarGrid(x=(float(g.x0), float(g.x0) + float(g.vx) * g.nx), y=(float(g.y0), float(g.y0) + float(g.vy) * g.ny),
                    z=(float(g.z0), float(g.z1)), size=(float(g.vx), float(g.vy)))
    assert (pg.nx, pg.ny) == (g.nx, g.ny) and tuple(F(v) for v in pg.scalars()) == tuple(g[:6])
    return pg


def sentinel_batch(B, capacity, N, Cc):
    from pseudo_lidar import PillarBatch
    pb = PillarBatch(B, capacity, N, Cc, DEV)
    pb.voxels.fill_(SENTINEL); pb.coords.fill_(int(SENTINEL)); pb.num_points.fill_(int(SENTINEL)); pb.offsets.fill_(int(SENTINEL))
    return pb


def run(a, capacity=None, points=None, offsets=None, out=None):
    from pseudo_lidar import pillarize
    points = torch.from_numpy(np.ascontiguousarray(a["points"])).to(DEV) if points is None else points
    offsets = torch.from_numpy(np.ascontiguousarray(a["offsets"])).to(DEV) if offsets is None else offsets
    g, B = a["grid"], len(a["offsets"]) - 1
    if out is None:
        cap = min(points.shape[0], B * g.ny * g.nx) if capacity is None else capacity
        out = sentinel_batch(B, cap, a["max_points"], 9 if a["decorate"] else 4)
    got = pillarize(points, offsets, grid=product_grid(g), max_points=a["max_points"], decorate=a["decorate"], out=out)
    assert got is out
    return out


def check(pb, want, total=None):
    """every output against the restatement (`want` may be clipped to a capacity; total: the unclipped pillar count), bit for bit: the
    used rows of voxels with their zero padding, coords, num_points, offsets; every row behind them still holds the sentinel"""
    P = len(want["coords"])
    assert pb.offsets.dtype == pb.coords.dtype == pb.num_points.dtype == torch.int32 and pb.voxels.dtype == torch.float32
    assert np.array_equal(pb.offsets.cpu().numpy(), want["offsets"])
    assert pb.counts().tolist() == want["offsets"].tolist()
    assert P == min(int(want["offsets"][-1]) if total is None else total, pb.voxels.shape[0])
    vox = pb.voxels.cpu().numpy()
    assert vox[:P].shape == want["voxels"].shape
    assert np.array_equal(vox[:P].view(np.uint32), want["voxels"].view(np.uint32))
    assert np.array_equal(pb.coords.cpu().numpy()[:P], want["coords"])
    num = pb.num_points.cpu().numpy()
    assert np.array_equal(num[:P], want["num_points"])
    pad = np.arange(vox.shape[1])[None, :] >= num[:P, None]
    assert (vox[:P].view(np.uint32)[pad] == 0).all()                                       # +0.0, every column
    assert (vox[P:] == SENTINEL).all() and bool((pb.coords[P:] == int(SENTINEL)).all()) and (num[P:] == int(SENTINEL)).all()


@pytest.mark.parametrize("case", C.CASES)
def test_kernels_match_restatement(case):
    C.check_non_trivial(case)
    want = C.reference(case)
    pb = run(C.build(case))
    assert pb.voxels.shape[0] > len(want["coords"])          # there are rows that must stay unwritten
    check(pb, want)
    parts = pb.split()
    assert len(parts) == len(want["offsets"]) - 1
    for b, (v, c, k) in enumerate(parts):
        lo, hi = want["offsets"][b], want["offsets"][b + 1]
        assert np.array_equal(v.cpu().numpy().view(np.uint32), want["voxels"][lo:hi].view(np.uint32))
        assert np.array_equal(c.cpu().numpy(), want["coords"][lo:hi]) and np.array_equal(k.cpu().numpy(), want["num_points"][lo:hi])


@pytest.mark.parametrize("case", C.TILE_CASES)
def test_more_tiles_than_one_scan_pass(case):
    """1047 tiles of 1024 cells: the scan of the tile sums takes a second pass with a carry, and every tile but the first starts its
    segments and pillar ranks at the sums of the tiles before it"""
    C.check_non_trivial(case)
    check(run(C.build(case)), C.reference(case))


@pytest.mark.parametrize("case", ["pair-N5-c9", "over-N64-c4"])
def test_capacity_below_the_count(case):
    """offsets stay exact, the rows that fit are written, nothing behind them is touched -- in buffers that go on behind the capacity"""
    from pseudo_lidar import PillarBatch
    a, full = C.build(case), C.reference(case)
    cap = int(full["offsets"][1]) + 3                        # ends inside the second image
    total = int(full["offsets"][-1])
    assert cap < total
    N, Cc = a["max_points"], 9 if a["decorate"] else 4
    big = sentinel_batch(len(full["offsets"]) - 1, cap + 40, N, Cc)
    small = PillarBatch(len(full["offsets"]) - 1, 1, N, Cc, DEV)
    small.voxels, small.coords, small.num_points, small.offsets = big.voxels[:cap], big.coords[:cap], big.num_points[:cap], big.offsets
    run(a, out=small)
    want = R.pillarize(capacity=cap, **a)
    assert np.array_equal(want["offsets"], full["offsets"]) and len(want["coords"]) == cap
    big._host = None
    check(big, want, total=cap)                              # the 40 rows behind the capacity kept their sentinel
    assert [tuple(v.shape) for v, _, _ in small.split()][:2] == [(int(full["offsets"][1]), N, Cc), (3, N, Cc)]


def test_row_view_of_the_output_buffers():
    """N * C = 45 floats per pillar: the blocks go out in dword stores, so a view that starts one row into a buffer (180 bytes, a multiple
    of 4 and not of 16) is taken; with N * C a multiple of 4 the same view of 16-byte blocks stays aligned.  The row in front is untouched."""
    from pseudo_lidar import PillarBatch
    for case in ("pair-N5-c9", "pair-N32-c4"):
        a, want = C.build(case), C.reference(case)
        N, Cc, P = a["max_points"], 9 if a["decorate"] else 4, int(want["offsets"][-1])
        big = sentinel_batch(3, P + 11, N, Cc)
        view = PillarBatch(3, 1, N, Cc, DEV)
        view.voxels, view.coords, view.num_points, view.offsets = big.voxels[1:], big.coords[1:], big.num_points[1:], big.offsets
        assert (view.voxels.data_ptr() % 16 != 0) == (case == "pair-N5-c9")
        run(a, out=view)
        assert bool((big.voxels[0] == SENTINEL).all()) and bool((big.coords[0] == int(SENTINEL)).all()) and int(big.num_points[0]) == int(SENTINEL)
        check(view, want)


def test_two_runs_give_the_same_bytes():
    """the case with 65, 130 and 300 points in a cell, where the atomics' arrival order decides where a point waits in its segment"""
    a = C.build("pair-N32-c9")
    first, second = run(a), run(a)
    for x, y in ((first.voxels, second.voxels), (first.coords, second.coords), (first.num_points, second.num_points),
                 (first.offsets, second.offsets)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    check(first, C.reference("pair-N32-c9"))


def test_capture_and_replay_on_new_contents():
    """pillarize(out=pb) captured on one stream, replayed after the cloud and its offsets changed in place: other points, another count,
    stale in-range rows left behind the new count"""
    a, b = C.build("pair-N32-c9"), C.build("mixed-N32-c9")
    assert len(b["points"]) < len(a["points"])
    pts = torch.from_numpy(np.ascontiguousarray(a["points"])).to(DEV)
    off = torch.from_numpy(np.ascontiguousarray(a["offsets"])).to(DEV)
    pb = sentinel_batch(3, len(a["points"]), 32, 9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(a, points=pts, offsets=off, out=pb)              # warm-up outside the capture: the workspace exists
    torch.cuda.current_stream().wait_stream(s)
    check(pb, C.reference("pair-N32-c9"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(a, points=pts, offsets=off, out=pb)
    host = a["points"].copy()
    host[:len(b["points"])] = b["points"]
    pts.copy_(torch.from_numpy(host))
    off.copy_(torch.from_numpy(np.ascontiguousarray(b["offsets"])))
    for t in (pb.voxels, pb.coords, pb.num_points, pb.offsets):
        t.fill_(SENTINEL)
    pb._host = None
    g.replay()
    torch.cuda.synchronize()
    want = R.pillarize(host, b["offsets"], b["grid"], 32, True)
    assert not np.array_equal(want["offsets"], C.reference("pair-N32-c9")["offsets"])
    check(pb, want)


def test_scan_past_its_first_pass():
    """5 images of the KITTI grid: 1,071,360 cells = 1047 tiles, more than the 1024 the tile scan takes per pass; points in the first and
    the last cells of every image and around the tile boundaries"""
    g = R.make_grid()
    rng = np.random.RandomState(8)
    per = 3000
    pts = np.stack([rng.uniform(-1.0, 70.5, 5 * per), rng.uniform(-40.5, 40.5, 5 * per), rng.uniform(-3.5, 1.5, 5 * per), rng.rand(5 * per)],
                   axis=1).astype(F)
    corners = np.array([[0.01, -39.67, 0, 1], [69.11, 39.67, 0, 1], [0.01, 39.67, 0, 1], [69.11, -39.67, 0, 1]], F)
    for b in range(5):
        pts[b * per:b * per + 4] = corners
    off = (np.arange(6) * per).astype(np.int32)
    a = dict(points=pts, offsets=off, grid=g, max_points=4, decorate=True)
    want = R.pillarize(**a)
    assert (np.diff(want["offsets"]) > 1500).all() and want["coords"][0].tolist() == [0, 0, 0, 0] and want["coords"][-1].tolist() == [4, 0, 495, 431]
    check(run(a), want)


def real_shape_cloud(beams):
    import pl_batch_cases as PC
    from pseudo_lidar import PseudoLiDAR, beam_tables
    h, w, H, W = 192, 640, 375, 1242
    m = torch.from_numpy(np.stack([PC.network_map(h, w, 40 + b, "disparity") for b in range(2)])).to(DEV)
    pl = PseudoLiDAR.from_matrices(PC.velo_T(PC.DATES[0]), PC.scaled_P(PC.DATES[0], H, W), 0)
    return pl.project_batch(m, sizes=[(H, W)] * 2, beams=beam_tables(64, 512) if beams else None)


@pytest.mark.parametrize("beams,decorate", [(False, True), (True, False)])
def test_project_batch_into_pillars_at_the_real_shape(beams, decorate):
    """2 x 192x640 -> 375x1242, dense (and decorated) and 64 x 512 beams, the KITTI grid, N = 32: the cloud stays on the device, its pillars
    are the restatement's of the same cloud"""
    cb = real_shape_cloud(beams)
    pb = cb.pillars(max_points=32, decorate=decorate)
    n = cb.counts()
    assert (np.diff(n) > (100000 if not beams else 3000)).all()
    want = R.pillarize(cb.points.cpu().numpy(), cb.offsets.cpu().numpy(), R.make_grid(), 32, decorate)
    P = int(want["offsets"][-1])
    assert (np.diff(want["offsets"]) > 1000).all() and (decorate or (want["num_points"] < 32).any())
    assert beams or (want["num_points"] == 32).sum() > 100                                 # dense: many cells hold more than N points
    assert np.array_equal(pb.offsets.cpu().numpy(), want["offsets"])
    assert np.array_equal(pb.voxels[:P].cpu().numpy().view(np.uint32), want["voxels"].view(np.uint32))
    assert np.array_equal(pb.coords[:P].cpu().numpy(), want["coords"]) and np.array_equal(pb.num_points[:P].cpu().numpy(), want["num_points"])


def test_c_abi_refuses_bad_arguments_untouched():
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401  (registers the signatures)
    h = L.lib()
    a = C.build("mixed-N4-c4")
    g, B, n = a["grid"], 3, len(a["points"])
    pts = torch.from_numpy(np.ascontiguousarray(a["points"])).to(DEV)
    off = torch.from_numpy(np.ascontiguousarray(a["offsets"])).to(DEV)
    pb = sentinel_batch(B, 100, 4, 4)
    need = h.mcav_pillarize_workspace_bytes(B, n, g.ny, g.nx)
    assert need > 0
    for args in ((0, n, 9, 7), (65536, n, 9, 7), (B, -1, 9, 7), (B, 1 << 31, 9, 7), (B, n, 0, 7), (B, n, 9, 0), (4, n, 1 << 15, 1 << 14)):
        assert h.mcav_pillarize_workspace_bytes(*args) == 0, args
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    good = dict(points=L.ptr(pts), offsets=L.ptr(off), B=B, n_max=n, x0=g.x0, y0=g.y0, z0=g.z0, z1=g.z1, vx=g.vx, vy=g.vy, nx=g.nx, ny=g.ny,
                N=4, flags=0, voxels=L.ptr(pb.voxels), coords=L.ptr(pb.coords), num=L.ptr(pb.num_points), cap=100, poff=L.ptr(pb.offsets),
                ws=L.ptr(ws), nws=need)
    call = lambda **kw: h.mcav_pillarize(*[dict(good, **kw)[k] for k in good], L.stream())
    nan, inf = float("nan"), float("inf")
    bad = [dict(points=L.c_p(0)), dict(offsets=L.c_p(0)), dict(voxels=L.c_p(0)), dict(coords=L.c_p(0)), dict(num=L.c_p(0)), dict(poff=L.c_p(0)),
           dict(ws=L.c_p(0)), dict(B=0), dict(B=65536), dict(n_max=-1), dict(n_max=1 << 31), dict(nx=1 << 16, ny=1 << 14), dict(nx=0), dict(ny=-1),
           dict(N=0), dict(N=65), dict(cap=-1), dict(vx=0.0), dict(vx=-0.5), dict(vx=nan), dict(vy=inf), dict(vy=0.0), dict(x0=nan), dict(x0=inf),
           dict(y0=-inf), dict(z0=1.0, z1=1.0), dict(z0=1.0, z1=-1.0), dict(z1=nan), dict(z0=nan), dict(flags=2), dict(flags=1 << 30),
           dict(points=L.c_p(pts.data_ptr() + 4)), dict(voxels=L.c_p(pb.voxels.data_ptr() + 4)), dict(coords=L.c_p(pb.coords.data_ptr() + 8))]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(nws=need - 1) == -2
    torch.cuda.synchronize()
    assert bool((pb.voxels == SENTINEL).all()) and bool((pb.offsets == int(SENTINEL)).all()) and bool((pb.coords == int(SENTINEL)).all())
    assert call() == 0
    check(pb, C.reference("mixed-N4-c4"))
    from pseudo_lidar import pillarize
    with pytest.raises(L.MCAVError):
        pillarize(pts, off.to(torch.int64))
    with pytest.raises(L.MCAVError):
        pillarize(pts, off, out=sentinel_batch(B, 100, 5, 4), max_points=4)                # out with other slots
    for spoil in (lambda o: setattr(o, "coords", o.coords.to(torch.int64)), lambda o: setattr(o, "num_points", o.num_points.float()),
                  lambda o: setattr(o, "coords", torch.zeros((100, 8), dtype=torch.int32, device=DEV)[:, ::2]),
                  lambda o: setattr(o, "voxels", torch.zeros((100, 4, 8), device=DEV)[:, :, ::2]),
                  lambda o: setattr(o, "num_points", o.num_points[:50]), lambda o: setattr(o, "offsets", o.offsets[:B])):
        out = sentinel_batch(B, 100, 4, 4)
        spoil(out)
        with pytest.raises(L.MCAVError):
            pillarize(pts, off, grid=product_grid(g), max_points=4, out=out)               # a wrongly typed, strided or sized buffer


def test_inference_pillars_on_the_synthetic_tree(tmp_path, monkeypatch):
    """Inference.pillars on every batch of the synthetic KITTI tree against the restatement of its own cloud; export(pillars=...) writes
    one .npz per frame beside the .bin, holding that frame's rows."""
    from inference import Inference
    from kitti_velo_tree import make_velo_tree, velo_config
    from pseudo_lidar import PillarGrid
    from trainer import Trainer
    monkeypatch.chdir(tmp_path)
    split, rows, _ = make_velo_tree(str(tmp_path), frames=4, sweep=100, extra=10)
    cfg = velo_config(split, str(tmp_path), 64, 128, batch=3)
    cfg["action"].update(from_scratch=True)
    torch.manual_seed(4)
    t = Trainer(cfg)
    t.save_chkpnt()
    inf = Inference(cfg, checkpoint=t.save_path)
    first = next(iter(inf.loader()))
    kw = dict(scale=float(6.0 / (1.0 / (10.0 * inf.disparity(first["tgt"]) + 0.01)).median()), max_height=4.0, max_depth=80.0)
    # the tree's small images cover about a metre of road each: 5 cm pillars, so that an image has many and some are full
    grid = PillarGrid(x=(0.0, 16.0), y=(-8.0, 8.0), z=(-3.0, 4.0), size=(0.05, 0.05))
    ref_grid = R.make_grid(x=grid.x, y=grid.y, z=grid.z, size=grid.size)
    out = str(tmp_path / "export")
    assert inf.export(out, pillars=dict(grid=grid, max_points=8, decorate=True), **kw) == len(rows) == 4
    found = sorted(os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs)
    assert found == sorted([inf.cloud_path(out, r[0]) for r in rows] + [inf.pillar_path(out, r[0]) for r in rows])
    seen = 0
    for samples in inf.loader():
        pb = inf.pillars(samples, grid=grid, max_points=8, decorate=True, **kw)
        want = R.pillarize(pb.cloud.points.cpu().numpy(), pb.cloud.offsets.cpu().numpy(), ref_grid, 8, True)
        P = int(want["offsets"][-1])
        print("points per image %s, pillars per image %s" % (np.diff(pb.cloud.counts()).tolist(), np.diff(want["offsets"]).tolist()))
        assert (np.diff(want["offsets"]) >= 10).all(), want["offsets"].tolist()
        assert (want["num_points"] == 8).any() and (want["num_points"] < 8).any()
        assert np.array_equal(pb.counts(), want["offsets"])
        assert np.array_equal(pb.voxels[:P].cpu().numpy().view(np.uint32), want["voxels"].view(np.uint32))
        assert np.array_equal(pb.coords[:P].cpu().numpy(), want["coords"]) and np.array_equal(pb.num_points[:P].cpu().numpy(), want["num_points"])
        for b, path in enumerate(samples["path"]):
            lo, hi = want["offsets"][b], want["offsets"][b + 1]
            z = np.load(inf.pillar_path(out, path))
            assert sorted(z.files) == ["coords", "num_points", "voxels"]
            assert np.array_equal(z["voxels"].view(np.uint32), want["voxels"][lo:hi].view(np.uint32))
            assert np.array_equal(z["coords"], want["coords"][lo:hi]) and np.array_equal(z["num_points"], want["num_points"][lo:hi])
            seen += 1
    assert seen == 4
    t.set_train()
