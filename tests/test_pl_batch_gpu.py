"""GPU: the batch pseudo-LiDAR projection (include/mcav_depth.h: mcav_pl_batch_project, PseudoLiDAR.project_batch, inference.py) against
its restatement (tests/pl_batch_ref.py), bit for bit, on the cases of tests/pl_batch_cases.py; against project_PL on the golden depths;
repeatability and graph capture; a round trip through the Velodyne ground-truth path; the export of a drive."""
import os

import numpy as np
import pytest
import torch

import pl_batch_cases as C
import pl_batch_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits_equal(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


_TABLES = {}


def tables_of(beams):
    """one BeamTables (and one device copy) per grid: a captured call must not build another"""
    from pseudo_lidar import BeamTables
    key = (len(beams[0]), len(beams[1]))
    if key not in _TABLES:
        _TABLES[key] = BeamTables(*beams)
    assert np.array_equal(_TABLES[key].elev, beams[0]) and np.array_equal(_TABLES[key].azim, beams[1])
    return _TABLES[key]


def run(a, out=None, m=None):
    from pseudo_lidar import PseudoLiDAR
    pl = PseudoLiDAR.from_matrices(a["T"][0], a["P"][0], a["sparsity"])
    return pl.project_batch(torch.from_numpy(a["m"]).to(DEV) if m is None else m, sizes=a["sizes"], P=a["P"], T=a["T"], input=a["input"],
                            scale=a["scale"], intensity=None if a["intensity"] is None else torch.from_numpy(a["intensity"]).to(DEV),
                            max_height=a["max_height"], max_depth=None if np.isinf(a["max_depth"]) else a["max_depth"],
                            beams=None if a["beams"] is None else tables_of(a["beams"]), out=out, padded=(a["Hg"], a["Wg"]))


@pytest.mark.parametrize("case", C.CASES)
def test_kernels_match_restatement(case):
    C.check_non_trivial(case)
    want, woff = C.reference(case)
    cb = run(C.build(case))
    assert cb.offsets.dtype == torch.int32 and np.array_equal(cb.offsets.cpu().numpy(), woff)
    assert cb.counts().tolist() == woff.tolist()
    bits_equal(cb.points[:int(woff[-1])], want)
    parts = cb.split()
    assert len(parts) == len(woff) - 1
    for b, part in enumerate(parts):
        bits_equal(part, want[woff[b]:woff[b + 1]])


def test_instance_calibration_is_broadcast():
    from pseudo_lidar import PseudoLiDAR
    a = C.build("direct-dense")
    want, woff = C.reference("direct-dense")
    m = torch.from_numpy(np.concatenate([a["m"], a["m"]])).to(DEV)
    cb = PseudoLiDAR.from_matrices(a["T"][0], a["P"][0], 0).project_batch(m[:, None])          # [B, 1, h, w], sizes = (h, w)
    assert cb.counts().tolist() == [0, int(woff[1]), 2 * int(woff[1])]
    for part in cb.split():
        bits_equal(part, want)


@pytest.mark.parametrize("case", ["odd-dense", "odd-beams8x16", "chunks-sparse3"])
def test_capacity_below_the_count(case):
    """offsets stay exact, the rows that fit are written, nothing beyond the buffer's used part is touched"""
    from pseudo_lidar import CloudBatch
    a = C.build(case)
    want, woff = C.reference(case)
    cap = int(woff[1]) + 5                               # ends inside the second image
    cb = CloudBatch(len(woff) - 1, cap + 64, DEV)
    cb.points.fill_(-7.0)
    small = CloudBatch(len(woff) - 1, cap, DEV)
    small.points = cb.points[:cap]                       # a view: the 64 rows behind it must stay as they are
    run(a, out=small)
    assert np.array_equal(small.offsets.cpu().numpy(), woff)
    bits_equal(cb.points[:cap], want[:cap])
    assert bool((cb.points[cap:] == -7.0).all())
    assert [tuple(p.shape) for p in small.split()][:2] == [(int(woff[1]), 4), (5, 4)]


def test_equals_project_PL_on_the_golden_depths():
    """the same pl_point on the same device: project_batch(input="depth") == project_PL(...)[:, :3].float(), bit for bit"""
    from pseudo_lidar import PseudoLiDAR
    g = np.load(os.path.join(GOLDEN, "pseudo_lidar.npz"))
    for name in "abc":
        pl = PseudoLiDAR.from_matrices(g["T"], g["P_" + name], int(g["sparsity_" + name]))
        d = torch.from_numpy(g["depth_" + name]).to(DEV)
        old = pl.project_PL(d)
        cb = pl.project_batch(d[None], input="depth")
        assert cb.counts().tolist() == [0, old.shape[0]] and old.shape[0] == g["cloud_" + name].shape[0]
        new = cb.split()[0]
        assert torch.equal(new[:, :3].view(torch.int32), old[:, :3].float().view(torch.int32)) and not bool(new[:, 3].any())


@pytest.mark.parametrize("case", ["odd-dense", "chunks-beams64x512"])
def test_repeat_and_capture(case):
    """Two calls agree bit for bit; project_batch(out=cb) captured on one stream replays on new contents of the same input tensor."""
    from pseudo_lidar import CloudBatch
    a = C.build(case)
    want, woff = C.reference(case)
    first, second = run(a), run(a)
    n = int(woff[-1])
    assert torch.equal(first.offsets, second.offsets) and torch.equal(first.points[:n].view(torch.int32), second.points[:n].view(torch.int32))
    bits_equal(first.points[:n], want)

    other = dict(a, m=np.stack([C.network_map(a["m"].shape[1], a["m"].shape[2], 900 + b, a["input"]) for b in range(a["m"].shape[0])]))
    assert not np.array_equal(other["m"], a["m"], equal_nan=True)
    m = torch.from_numpy(a["m"]).to(DEV)
    cb = CloudBatch(len(woff) - 1, first.points.shape[0], DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(a, out=cb, m=m)                              # warm-up outside the capture: the calibration table and the workspace exist
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(a, out=cb, m=m)
    m.copy_(torch.from_numpy(other["m"]))
    cb.points.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    eager = run(other)
    k = int(eager.counts()[-1])
    assert k != n or not torch.equal(eager.points[:k], first.points[:k])
    assert torch.equal(cb.offsets, eager.offsets) and torch.equal(cb.points[:k].view(torch.int32), eager.points[:k].view(torch.int32))
    wother, wooff = R.project_batch(**other)
    assert np.array_equal(cb.offsets.cpu().numpy(), wooff)
    bits_equal(cb.points[:k], wother)


def test_round_trip_through_the_velodyne_path(tmp_path):
    """A dense cloud of a 375 x 1242 depth map (2..60 m), saved with save_bin, reloaded and projected by geometry.velodyne.depth_maps with
    P_rect @ T, reproduces depth[r, c] at [r-1, c-1] (that function's documented - 1) within 4 * 2**-24 * range -- three rounded coordinates
    and one rounded result -- for every surviving pixel with r, c >= 1, and nothing else is non-zero.
    P_rect is KITTI's P_rect_02 with P[2, 3] = 0: pl_point, as the reference's project_PL, un-projects with cu, cv, fu, fv, bx, by only,
    which inverts the projection exactly when the third row has no translation (KITTI's 0.0027 m would move column 1241 at 2 m by 1.7 px)."""
    from geometry.velodyne import depth_maps, load_velodyne_points
    from pseudo_lidar import PseudoLiDAR
    H, W = 375, 1242
    P = C.scaled_P(C.DATES[0], H, W)
    P[2, 3] = 0.0
    T = C.velo_T(C.DATES[0])
    rng = np.random.RandomState(11)
    depth = (2.0 + 58.0 * rng.rand(H, W)).astype(np.float32)
    cb = PseudoLiDAR.from_matrices(T, P, 0).project_batch(torch.from_numpy(depth).to(DEV)[None], input="depth")
    path = str(tmp_path / "cloud.bin")
    cb.save_bin([path])
    pts = load_velodyne_points(path)
    bits_equal(cb.split()[0], pts)                       # the file holds the device rows
    want, woff = R.project_batch(depth[None], P=P, T=T, input="depth")
    bits_equal(pts, want)
    assert 4 * len(pts) >= H * W
    back = depth_maps(torch.from_numpy(pts), [0, len(pts)], np.dot(P, T)[None], [(H, W)])[0, 0].cpu().numpy()
    q = R.points(depth, P, T)
    keep = R.kept(q, depth)
    rng64 = np.sqrt((q ** 2).sum(-1))
    expect = np.zeros((H, W), bool)
    expect[:-1, :-1] = keep[1:, 1:]
    assert np.array_equal(back != 0, expect)
    err = np.abs(back[:-1, :-1].astype(np.float64) - depth[1:, 1:].astype(np.float64))[keep[1:, 1:]]
    bound = (4 * 2.0 ** -24 * rng64[1:, 1:])[keep[1:, 1:]]
    print("round trip: %d pixels, max error / bound = %.3f" % (err.size, float((err / bound).max())))
    assert (err <= bound).all()


def test_c_abi_refuses_bad_arguments_untouched():
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401  (registers the signatures)
    h = L.lib()
    B, hh, ww = 2, 8, 16
    m = torch.full((B, hh, ww), 0.05, device=DEV)
    sizes = torch.tensor([hh, ww] * B, dtype=torch.int32, device=DEV)
    a = C.build("direct-dense")
    calib = torch.from_numpy(np.tile(np.concatenate([a["P"][0].reshape(-1), a["T"][0].reshape(-1)]), B)).to(DEV)
    elev, azim = (torch.from_numpy(t).to(DEV) for t in C.uniform_tables(8, 16))
    cloud = torch.full((B * hh * ww, 4), -7.0, device=DEV)
    offsets = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
    need = h.mcav_pl_batch_workspace_bytes(B, hh, ww, 8, 16)
    assert need > 0 and h.mcav_pl_batch_workspace_bytes(0, hh, ww, 0, 0) == 0 and h.mcav_pl_batch_workspace_bytes(B, hh, ww, 8, 0) == 0
    assert h.mcav_pl_batch_workspace_bytes(4, 1 << 15, 1 << 15, 0, 0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    good = dict(m=L.ptr(m), B=B, h=hh, w=ww, Hg=hh, Wg=ww, sizes=L.ptr(sizes), calib=L.ptr(calib), inten=L.c_p(0), elev=L.c_p(0),
                azim=L.c_p(0), nb=0, na=0, scale=1.0, mh=1.0, md=float("inf"), sparsity=0, flags=0, cloud=L.ptr(cloud),
                cap=cloud.shape[0], offsets=L.ptr(offsets), ws=L.ptr(ws), nws=need)
    call = lambda **kw: h.mcav_pl_batch_project(*[dict(good, **kw)[k] for k in good], L.stream())
    bad = [dict(flags=2), dict(flags=1 << 30), dict(m=L.c_p(0)), dict(sizes=L.c_p(0)), dict(calib=L.c_p(0)), dict(cloud=L.c_p(0)),
           dict(offsets=L.c_p(0)), dict(ws=L.c_p(0)), dict(B=0), dict(h=0), dict(Wg=-1), dict(sparsity=-1), dict(elev=L.ptr(elev)),
           dict(elev=L.ptr(elev), azim=L.ptr(azim)), dict(nb=8, na=16), dict(scale=float("nan")), dict(md=float("nan")),
           dict(cloud=L.c_p(cloud.data_ptr() + 4))]
    for kw in bad:
        assert call(**kw) == -1, kw
    dense_need = h.mcav_pl_batch_workspace_bytes(B, hh, ww, 0, 0)
    assert 0 < dense_need < need and call(nws=dense_need - 1) == -2
    assert call(elev=L.ptr(elev), azim=L.ptr(azim), nb=8, na=16, nws=need - 1) == -2
    torch.cuda.synchronize()
    assert bool((cloud == -7.0).all()) and bool((offsets == -7).all())
    assert call() == 0 and call(elev=L.ptr(elev), azim=L.ptr(azim), nb=8, na=16) == 0 and call(flags=1) == 0
    torch.cuda.synchronize()
    assert int(offsets[0]) == 0 and int(offsets[-1]) > 0
    from pseudo_lidar import PseudoLiDAR
    with pytest.raises(L.MCAVError):
        PseudoLiDAR.from_matrices(a["T"][0], a["P"][0], 3).project_batch(m, beams=C.uniform_tables(8, 16))      # sparsity with beams
    with pytest.raises(L.MCAVError):
        PseudoLiDAR.from_matrices(a["T"][0], a["P"][0], 0).project_batch(m, sizes=[(hh, ww), (hh + 1, ww)], padded=(hh, ww))


def test_inference_exports_a_drive(tmp_path, monkeypatch):
    """A randomly initialised net saved by Trainer.save_chkpnt: the file count and names, every file equal to clouds()'s slice, the
    disparity bit-equal to the trainer's evaluation forward on the same weights."""
    from geometry.velodyne import load_velodyne_points
    from inference import Inference
    from kitti_velo_tree import make_velo_tree, velo_config
    from pseudo_lidar import beam_tables
    from trainer import Trainer
    monkeypatch.chdir(tmp_path)
    split, rows, _ = make_velo_tree(str(tmp_path), frames=4, sweep=100, extra=10)          # 2 samples per date, two image sizes
    cfg = velo_config(split, str(tmp_path), 64, 128, batch=3)
    cfg["action"].update(from_scratch=True)
    torch.manual_seed(4)
    t = Trainer(cfg)
    t.save_chkpnt()
    inf = Inference(cfg, checkpoint=t.save_path)
    assert not inf.depth_model.training and not hasattr(inf, "pose_model") and not hasattr(inf, "model_optimizer")
    # the tree's images are 1/8 of the size its P_rect_02 describes, so every pixel lies far up and left of the principal point, and a
    # random net's disparity means ~0.2 m: scale the depths to ~6 m and raise the height cut, so that most pixels survive (checked below)
    first = next(iter(inf.loader()))
    kw = dict(scale=float(6.0 / (1.0 / (10.0 * inf.disparity(first["tgt"]) + 0.01)).median()), max_height=4.0, max_depth=80.0)
    out = str(tmp_path / "clouds")
    n = inf.export(out, **kw)
    assert n == len(rows) == 4
    names = [inf.cloud_path(out, r[0]) for r in rows]
    for r, p in zip(rows, names):
        date = [x for x in r[0].split("/") if x.startswith("2011_") and "drive" not in x][0]
        frame = os.path.splitext(os.path.basename(r[0]))[0]
        assert p == os.path.join(out, date, date + "_drive_0001_sync", "pseudo_velodyne", "data", frame + ".bin") and os.path.exists(p)
    found = sorted(os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs)
    assert found == sorted(names)
    t.depth_model.eval()
    seen = 0
    for samples in inf.loader():
        with torch.no_grad():
            want_disp = t.depth_model(samples["tgt"])[0]
        disp = inf.disparity(samples["tgt"])
        assert torch.equal(disp.view(torch.int32), want_disp.view(torch.int32))
        cb = inf.clouds(samples, **kw)
        sizes = samples["native_size"].numpy()
        want, woff = R.project_batch(disp[:, 0].cpu().numpy(), sizes=sizes, P=samples["P_rect"].numpy(), T=samples["T_velo_cam"].numpy(), **kw)
        assert np.array_equal(cb.counts(), woff)
        assert all(4 * k >= H * W for k, (H, W) in zip(np.diff(woff), sizes)), (np.diff(woff).tolist(), sizes.tolist())
        for b, part in enumerate(cb.split()):
            pts = load_velodyne_points(inf.cloud_path(out, samples["path"][b]))
            bits_equal(part, pts)
            bits_equal(pts, want[woff[b]:woff[b + 1]])
            assert tuple(sizes[b]) in ((47, 156), (46, 153))
            seen += 1
        grid = beam_tables(8, 16, elevation=(-10.0, 40.0))
        beams = inf.clouds(samples, beams=grid, **kw)
        bwant, bwoff = R.project_batch(disp[:, 0].cpu().numpy(), sizes=sizes, P=samples["P_rect"].numpy(), T=samples["T_velo_cam"].numpy(),
                                       beams=(grid.elev, grid.azim), **kw)
        assert np.array_equal(beams.counts(), bwoff) and (np.diff(bwoff) > 0).all()
        bits_equal(beams.points[:int(bwoff[-1])], bwant)
    assert seen == 4
    t.set_train()


def test_calibration_upload_and_workspace_are_kept():
    """project_batch, ground_scale and gdc with out=: equal calibration leaves the device table and the workspace where they are (nothing
    is copied or allocated: what a capture's warm-up relies on); one changed matrix entry replaces the table, the workspace stays, and the
    result is a fresh object's, bit for bit (and not the first call's)."""
    import gdc_cases as DC
    import ground_scale_cases as GC
    from pseudo_lidar import gdc, ground_scale
    a, g, d = C.build("direct-dense"), GC.build("flat"), DC.build("full")          # the smallest case of each module's list
    gm, depth, sparse = torch.tensor(g["m"], device=DEV), torch.tensor(d["depth"], device=DEV), torch.tensor(d["sparse"], device=DEV)
    gkw = dict(sizes=g["sizes"], camera_height=g["camera_height"], max_angle_deg=g["max_angle_deg"], box=g["boxes"],
               min_ground=g["min_ground"], fallback=g["fallback"], input=g["input"], keep_mask=True)

    def cloud(P, out):
        cb = run(dict(a, P=P), out=out)
        return cb, (cb.offsets, cb.points[:int(cb.counts()[-1])].view(torch.int32))

    def scale(P, out):
        gs = ground_scale(gm, P=P, out=out, **gkw)
        return gs, (gs.rows.view(torch.int32), gs.mask)

    def corrected(K, out):
        res = gdc(depth, sparse, K, min_known=d["min_known"], out=out, **d["params"])
        return res, (res.depth.view(torch.int32), res.info.view(torch.int32), res.nbr, res.weights.view(torch.int32))

    for stage, calib, entry in ((cloud, a["P"], (0, 0, 2)), (scale, g["P"], (0, 0, 0)), (corrected, d["K"], (0, 0))):
        changed = np.array(calib)
        changed[entry] *= 1.5
        out, first = stage(calib, None)
        first = [t.clone() for t in first]
        table, ws = out._uploaded, out._ws
        at = table.data_ptr(), ws.data_ptr()
        again, second = stage(np.array(calib), out)                                # equal values in another array
        assert again is out and out._uploaded is table and out._ws is ws and (table.data_ptr(), ws.data_ptr()) == at
        assert all(torch.equal(x, y) for x, y in zip(first, second))
        _, third = stage(changed, out)
        assert out._uploaded is not table and out._uploaded.data_ptr() != at[0]          # (the old one is still alive here)
        assert out._ws is ws and ws.data_ptr() == at[1]
        fresh = stage(changed, None)[1]
        assert all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(third, fresh)), stage.__name__
        assert not all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(third, first)), stage.__name__
