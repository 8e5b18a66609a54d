"""GPU: the ground-plane scale estimator (include/mcav_depth.h: mcav_ground_scale; pseudo_lidar.ground_scale) against its restatement
tests/ground_scale_ref.py, bit for bit, on the scenes of tests/ground_scale_cases.py; repeatability, graph capture, a dirty workspace,
rejected arguments; the per-image device scale in PseudoLiDAR.project_batch and evaluate.evaluate_depth against the existing calls image
by image; scale="ground" end to end, in Inference.clouds and in Trainer.validate."""
import os

import numpy as np
import pytest
import torch

import ground_scale_cases as C
import ground_scale_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits_equal(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


def run(a, m=None, out=None, keep_mask=True):
    from pseudo_lidar import ground_scale
    return ground_scale(torch.from_numpy(a["m"]).to(DEV) if m is None else m, sizes=a["sizes"], P=a["P"], camera_height=a["camera_height"],
                        max_angle_deg=a["max_angle_deg"], box=a["boxes"], min_ground=a["min_ground"], fallback=a["fallback"],
                        input=a["input"], keep_mask=keep_mask, out=out)


@pytest.mark.parametrize("case", C.CASES)
def test_kernels_match_restatement(case):
    want_rows, want_mask, want_hgt = C.reference(case)[:3]
    assert want_rows[:, 2].max() >= 100
    gs = run(C.build(case))
    assert gs.mask.dtype == torch.uint8 and np.array_equal(gs.mask.cpu().numpy(), want_mask)
    bits_equal(gs.rows, want_rows)
    # every pixel's key in the workspace: the bits of the restatement's height on a ground pixel, 0xFFFFFFFF elsewhere (the median alone
    # would not show a height that is an ulp off)
    B, h, w = want_mask.shape
    keys = gs._ws[:4 * B * (h - 2) * (w - 2)].cpu().numpy().view(np.uint32).reshape(B, h - 2, w - 2)
    want_keys = np.where(want_mask[:, 1:-1, 1:-1] == 1, want_hgt[:, 1:-1, 1:-1].view(np.uint32), np.uint32(0xFFFFFFFF))
    assert np.array_equal(keys, want_keys), int((keys != want_keys).sum())
    assert gs.scales.data_ptr() == gs.rows.data_ptr() and tuple(gs.scales.shape) == (len(want_rows),)       # a view: column 0
    bits_equal(gs.scales.contiguous(), np.ascontiguousarray(want_rows[:, 0]))


@pytest.mark.parametrize("case", ["odd", "full"])
def test_same_call_twice_gives_identical_bits(case):
    a = C.build(case)
    first, second = run(a), run(a)
    assert torch.equal(first.rows.view(torch.int32), second.rows.view(torch.int32)) and torch.equal(first.mask, second.mask)
    nomask = run(a, keep_mask=False)
    assert nomask.mask is None and torch.equal(first.rows.view(torch.int32), nomask.rows.view(torch.int32))


def test_capture_replays_on_new_contents_and_a_dirty_workspace():
    """ground_scale(out=gs) captured on one stream replays on new contents of the same input tensor; the workspace needs no zero-fill: one
    filled with 0xFF bytes gives the same bits."""
    from mcav import lib as L
    from pseudo_lidar import GroundScale
    a = C.build("flat")
    B, h, w = a["m"].shape
    other = np.array(C.build("special")["m"])
    assert other.shape == a["m"].shape
    want_rows, want_mask = C.reference("flat")[:2]
    other_rows, other_mask = G.ground_scale(other, **C.call_kw(a))[:2]
    assert not np.array_equal(other_mask, want_mask)
    m = torch.from_numpy(a["m"]).to(DEV)
    gs = GroundScale(B, DEV, (B, h, w))
    gs._ws = torch.full((L.lib().mcav_ground_scale_workspace_bytes(B, h, w),), 0xFF, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(a, m=m, out=gs)                              # warm-up outside the capture: the calibration table exists
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    bits_equal(gs.rows, want_rows)                       # (the dirty workspace)
    assert np.array_equal(gs.mask.cpu().numpy(), want_mask)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(a, m=m, out=gs)
    m.copy_(torch.from_numpy(other))
    gs.rows.fill_(-7.0)
    gs.mask.fill_(9)
    gs._ws.fill_(0xFF)
    g.replay()
    torch.cuda.synchronize()
    bits_equal(gs.rows, other_rows)
    assert np.array_equal(gs.mask.cpu().numpy(), other_mask)


def test_c_abi_refuses_bad_arguments_untouched():
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401  (registers the signatures)
    hl = L.lib()
    a = C.build("flat")
    B, h, w = a["m"].shape
    m = torch.from_numpy(a["m"]).to(DEV)
    sizes = torch.tensor(a["sizes"], dtype=torch.int32, device=DEV)
    calib = torch.from_numpy(np.concatenate([a["P"].reshape(B, 12), a["T"].reshape(B, 16)], axis=1)).to(DEV)
    rows = torch.full((B, 4), -7.0, device=DEV)
    mask = torch.full((B, h, w), 9, dtype=torch.uint8, device=DEV)
    need = hl.mcav_ground_scale_workspace_bytes(B, h, w)
    assert need > 0 and hl.mcav_ground_scale_workspace_bytes(B, 2, w) == 0 and hl.mcav_ground_scale_workspace_bytes(0, h, w) == 0
    assert hl.mcav_ground_scale_workspace_bytes(1 << 15, 256, 256) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    good = dict(m=L.ptr(m), B=B, h=h, w=w, sizes=L.ptr(sizes), calib=L.ptr(calib), boxes=L.c_p(0), ch=1.65, cos=float(G.cos_max_of(5.0)),
                ming=100, fallback=float("nan"), flags=0, rows=L.ptr(rows), mask=L.ptr(mask), ws=L.ptr(ws), nws=need)
    call = lambda **kw: hl.mcav_ground_scale(*[dict(good, **kw)[k] for k in good], L.stream())
    bad = [dict(m=L.c_p(0)), dict(sizes=L.c_p(0)), dict(calib=L.c_p(0)), dict(rows=L.c_p(0)), dict(ws=L.c_p(0)), dict(h=2), dict(w=2),
           dict(B=0), dict(B=-3), dict(B=1 << 15, h=256, w=256), dict(ch=0.0), dict(ch=-1.65), dict(ch=float("nan")), dict(ch=float("inf")),
           dict(cos=0.0), dict(cos=-0.5), dict(cos=1.5), dict(cos=float("nan")), dict(ming=0), dict(ming=-1), dict(flags=2),
           dict(flags=1 << 30)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(nws=need - 1) == -2
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and bool((mask == 9).all())
    assert call() == 0 and call(mask=L.c_p(0)) == 0 and call(cos=1.0) == 0
    torch.cuda.synchronize()
    assert bool((rows[:, 2] == 0).all()) and bool((rows[:, 3] == 0).all())           # no normal lies exactly along y
    assert call() == 0
    torch.cuda.synchronize()
    bits_equal(rows, C.reference("flat")[0])


# ---------------------------------------------------------------------------------------------- the per-image scale on the device
def projector(a):
    from pseudo_lidar import PseudoLiDAR
    return PseudoLiDAR.from_matrices(a["T"][0], a["P"][0], 0)


@pytest.mark.parametrize("form", ["dense", "beams"])
def test_project_batch_with_device_scales_is_the_float_call_per_image(form):
    from pl_batch_cases import uniform_tables
    from pseudo_lidar import BeamTables
    a = C.build("odd")
    B = len(a["sizes"])
    beams = BeamTables(*uniform_tables(8, 16)) if form == "beams" else None
    m = torch.from_numpy(a["m"]).to(DEV)
    kw = dict(input=a["input"], max_height=1.0, max_depth=80.0, beams=beams)
    pl = projector(a)
    for values in ([1.0, 0.37, 5.3], [2.5, float("nan"), 1.0], [-1.0, float("inf"), 0.0]):
        t = torch.tensor(values, dtype=torch.float32, device=DEV)
        cb = pl.project_batch(m, sizes=a["sizes"], P=a["P"], T=a["T"], scale=t, **kw)
        parts = cb.split()
        for b in range(B):
            s = float(t[b])
            if not (np.isfinite(s) and s > 0):
                assert parts[b].shape[0] == 0, (values, b)
                continue
            one = pl.project_batch(m[b:b + 1], sizes=[a["sizes"][b]], P=a["P"][b], T=a["T"][b], scale=s, **kw)
            want = one.split()[0]
            assert want.shape[0] > 30 and parts[b].shape == want.shape, (values, b, parts[b].shape, want.shape)
            assert torch.equal(parts[b].view(torch.int32), want.view(torch.int32)), (values, b)
    plain = pl.project_batch(m, sizes=a["sizes"], P=a["P"], T=a["T"], scale=1.0, **kw)          # a float: the old entry, and a tensor of ones
    ones = pl.project_batch(m, sizes=a["sizes"], P=a["P"], T=a["T"], scale=torch.ones(B, device=DEV), **kw)
    assert torch.equal(plain.offsets, ones.offsets)
    n = int(plain.counts()[-1])
    assert torch.equal(plain.points[:n].view(torch.int32), ones.points[:n].view(torch.int32))


@pytest.mark.parametrize("median_scaling", [True, False])
def test_evaluate_depth_with_device_scales_is_the_float_call_per_image(median_scaling):
    from evaluate import evaluate_depth
    from test_eval_depth_gpu import kitti_batch
    sizes = [(375, 1242), (370, 1226), (188, 620)]
    gt, disp = kitti_batch(sizes, 375, 1242, 23, 37, seed=5)
    gt, disp = torch.from_numpy(gt).to(DEV), torch.from_numpy(disp).to(DEV)
    t = torch.tensor([1.0, 0.37, 5.3], dtype=torch.float32, device=DEV)
    _, rows = evaluate_depth(gt, disp, sizes, median_scaling=median_scaling, scales=t, per_image=True)
    _, plain = evaluate_depth(gt, disp, sizes, median_scaling=median_scaling, per_image=True)
    _, ones = evaluate_depth(gt, disp, sizes, median_scaling=median_scaling, scales=torch.ones(3, device=DEV), per_image=True)
    assert torch.equal(plain.view(torch.int32), ones.view(torch.int32))
    assert not torch.equal(rows[1:, 10 if median_scaling else 1], plain[1:, 10 if median_scaling else 1])
    for b, (Hb, Wb) in enumerate(sizes):
        _, want = evaluate_depth(gt[b:b + 1], disp[b:b + 1], [sizes[b]], median_scaling=median_scaling, scale=float(t[b]), per_image=True)
        assert want[0, 9] > 0 and torch.equal(rows[b].view(torch.int32), want[0].view(torch.int32)), (b, rows[b], want[0])
    if not median_scaling:
        assert bool((rows[:, 10] == 1.0).all())
    # a column of the estimator's rows (a strided view) is taken as it is
    packed = torch.zeros(3, 4, device=DEV)
    packed[:, 0] = t
    _, again = evaluate_depth(gt, disp, sizes, median_scaling=median_scaling, scales=packed[:, 0], per_image=True)
    assert torch.equal(again.view(torch.int32), rows.view(torch.int32))


@pytest.mark.parametrize("form", ["dense", "beams"])
def test_project_batch_scale_ground_is_the_estimator_then_the_tensor_path(form):
    from pl_batch_cases import uniform_tables
    from pseudo_lidar import BeamTables
    a = C.build("noground" if form == "dense" else "odd")
    beams = BeamTables(*uniform_tables(8, 16)) if form == "beams" else None
    m = torch.from_numpy(a["m"]).to(DEV)
    pl = projector(a)
    gkw = dict(camera_height=a["camera_height"], max_angle_deg=a["max_angle_deg"], min_ground=a["min_ground"])
    kw = dict(sizes=a["sizes"], P=a["P"], T=a["T"], max_depth=80.0, beams=beams)
    cb = pl.project_batch(m, scale="ground", ground=gkw, **kw)
    gs = run(a)
    bits_equal(cb.ground.rows, gs.rows.cpu().numpy())
    bits_equal(cb.ground.rows, C.reference("noground" if form == "dense" else "odd")[0])
    want = pl.project_batch(m, scale=gs.scales.contiguous(), **kw)
    assert torch.equal(cb.offsets, want.offsets)
    n = int(want.counts()[-1])
    assert n > 0 and torch.equal(cb.points[:n].view(torch.int32), want.points[:n].view(torch.int32))
    counts = np.diff(cb.counts())
    if form == "dense":
        assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0                  # the image without ground: NaN scale, empty cloud
    from mcav.lib import MCAVError
    with pytest.raises(MCAVError):
        pl.project_batch(m, scale="road", **kw)
    with pytest.raises(MCAVError):
        pl.project_batch(m, scale=2.0, ground=gkw, **kw)
    for key, value in (("input", "depth"), ("sizes", a["sizes"]), ("P", a["P"]), ("out", None), ("angle", 5.0)):
        with pytest.raises(MCAVError, match="ground="):
            pl.project_batch(m, scale="ground", ground=dict(gkw, **{key: value}), **kw)
    masked = pl.project_batch(m, scale="ground", ground=dict(gkw, keep_mask=True), out=cb, **kw)      # cb.ground was made without a mask
    assert masked is cb and np.array_equal(cb.ground.mask.cpu().numpy(), gs.mask.cpu().numpy())
    assert torch.equal(cb.offsets, want.offsets) and torch.equal(cb.points[:n].view(torch.int32), want.points[:n].view(torch.int32))


# ---------------------------------------------------------------------------------------------- inference and validation
class RoadNet(torch.nn.Module):
    """Stands in for the depth network: whatever the image, the disparity of a flat road 1.65 m below a camera with P (for a native size),
    its depths divided by s_true -- a monocular prediction with an unknown scale."""

    def __init__(self, P, size, s_true):
        super().__init__()
        self.P, self.size, self.s_true = np.asarray(P, np.float64), size, float(s_true)
        self.bias = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        B, _, h, w = x.shape
        xn = G.rays(self.size[1], w, self.P[0, 2], self.P[0, 0], np.float64)[None, :]
        yn = G.rays(self.size[0], h, self.P[1, 2], self.P[1, 1], np.float64)[:, None]
        slope = yn + 0.0 * xn + 0.01
        d = np.where(slope > 1.65 / 80.0, 1.65 / np.maximum(slope, 1e-9), 80.0 - 20.0 * xn) / self.s_true
        disp = torch.from_numpy(((1.0 / d - 0.01) / 10.0).astype(np.float32)).to(x.device)
        return [disp[None, None].expand(B, 1, h, w).contiguous()]


def road_tree(root, frames):
    """tests/kitti_velo_tree.py's tree with P_rect_02 brought to the size of its (1/8-size) images: the principal point lies inside them, so
    the lower half of every image looks at the road"""
    from kitti_tree import P_RECT
    from kitti_velo_tree import make_velo_tree
    split, rows, _ = make_velo_tree(root, frames=frames, sweep=4000, extra=300)
    P = {}
    for date, vals in P_RECT.items():
        P[date] = np.array(vals, np.float64).reshape(3, 4)
        P[date][:2] /= 8.0
        path = os.path.join(root, "KITTI", date, "calib_cam_to_cam.txt")
        lines = open(path).read().splitlines()
        lines = [("P_rect_02: " + " ".join("%.6e" % v for v in P[date].reshape(-1))) if ln.startswith("P_rect_02:") else ln for ln in lines]
        open(path, "w").write("\n".join(lines) + "\n")
    return split, rows, P


def test_inference_clouds_with_ground_scale(tmp_path, monkeypatch):
    from inference import Inference
    from kitti_tree import SIZES
    from kitti_velo_tree import velo_config
    monkeypatch.chdir(tmp_path)
    split, rows, P = road_tree(str(tmp_path), frames=4)
    cfg = velo_config(split, str(tmp_path), 64, 128, batch=3)
    torch.manual_seed(4)
    inf = Inference(cfg)
    inf.depth_model = RoadNet(P["2011_09_26"], SIZES["2011_09_26"], s_true=4.0).to(DEV)
    seen = 0
    for samples in inf.loader():
        cb = inf.clouds(samples, scale="ground", ground=dict(camera_height=1.65), max_depth=80.0)
        g = cb.ground.rows.cpu().numpy()
        assert (g[:, 3] == 1).all() and (g[:, 2] >= 100).all() and np.abs(g[:, 0] / 4.0 - 1.0).max() < 0.1, g
        counts = np.diff(cb.counts())
        sizes = samples["native_size"].numpy()
        assert all(4 * k >= H * W for k, (H, W) in zip(counts, sizes)), (counts.tolist(), sizes.tolist())
        pts = cb.split()[0].cpu().numpy()
        near = pts[pts[:, 0] < 10.0]                    # the road in metres: about 1.65 + 0.08 m below the velodyne (its frame is tilted
        assert len(near) > 100 and np.abs(near[:, 2] + 1.73).max() < 0.4              # by a degree, and the net knows one calibration only)
        seen += len(counts)
    assert seen == len(rows) == 4
    out = str(tmp_path / "clouds")
    assert inf.export(out, scale="ground", max_depth=80.0) == 4


def test_trainer_validation_with_ground_scaling(tmp_path):
    import eval_protocol_ref as R
    from kitti_tree import SIZES
    from kitti_velo_tree import velo_config
    from trainer import Trainer
    split, _, P = road_tree(str(tmp_path), frames=6)     # 8 samples, two image sizes
    cfg = velo_config(split, str(tmp_path), 64, 128, batch=3)
    cfg["action"]["split"] = [0.5, 0.5]
    cfg["validation"] = {"crop": "garg", "scaling": "ground", "camera_height": 1.65}
    with pytest.raises(ValueError, match="calibration"):
        Trainer(cfg)
    cfg["datasets"]["calibration"] = True
    t = Trainer(cfg)
    t.depth_model = RoadNet(P["2011_09_26"], SIZES["2011_09_26"], s_true=4.0).to(DEV)
    got = t.validate()
    assert set(got) == set(R.KEYS) | {"images", "count", "ratio_median", "ratio_std", "ground_scale_mean", "ground_scale_std",
                                      "ground_fallbacks"}
    assert got["images"] == 4 and got["count"] > 0 and all(np.isfinite(got[k]) for k in R.KEYS)
    assert got["ground_fallbacks"] == 0 and abs(got["ground_scale_mean"] / 4.0 - 1.0) < 0.1 and 0 <= got["ground_scale_std"] < 0.4
    assert got["ratio_median"] == 1.0                   # scored without median scaling
    cfg["validation"] = {"crop": "garg", "scaling": "median"}
    t2 = Trainer(cfg)
    t2.depth_model = t.depth_model
    plain = t2.validate()
    assert "ground_scale_mean" not in plain and plain["ratio_median"] != 1.0 and plain["count"] == got["count"]
