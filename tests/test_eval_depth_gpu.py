"""GPU: the KITTI depth evaluation protocol (include/mcav_depth.h: mcav_eval_depth; evaluate.evaluate_depth) against its restatement
tests/eval_protocol_ref.py: parity at KITTI sizes, exact medians, padding independence, reproducibility, hipGraph capture, argument
rejection, the loader's native ground truth and Trainer.validate with the `validation` key."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eval_protocol_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KITTI_SIZES = [(375, 1242), (370, 1226), (375, 1242), (370, 1226)]


def kitti_batch(sizes, Hg, Wg, h, w, seed, density=0.3, pad=0.0):
    """Sparse ground truth in metres quantised to 1/256 m, zero beyond each true size (or `pad`), and sigmoid disparities that follow it."""
    rng = np.random.RandomState(seed)
    gt = np.full((len(sizes), Hg, Wg), pad, np.float32)
    for b, (H, W) in enumerate(sizes):
        g = (np.round(rng.uniform(0.5, 85.0, (H, W)) * 256) / 256).astype(np.float32)
        g[rng.rand(H, W) > density] = 0
        gt[b, :H, :W] = g
    disp = rng.uniform(0.005, 0.5, (len(sizes), h, w)).astype(np.float32)
    return gt, disp


def check_rows(got, want, label=""):
    got = got.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:, 9], want[:, 9]), (label, got[:, 9], want[:, 9])
    for b in range(want.shape[0]):
        n = want[b, 9]
        if n == 0:
            assert np.isnan(got[b, :9]).all() and np.isnan(got[b, 10]), label
            continue
        assert abs(got[b, 10] - want[b, 10]) <= 2e-6 * abs(want[b, 10]), (label, b, got[b, 10], want[b, 10])
        for i, k in enumerate(R.KEYS):
            tol = 2.0 / n if k in ("d1", "d2", "d3") else 1e-5 * abs(want[b, i])
            assert abs(got[b, i] - want[b, i]) <= tol, (label, b, k, got[b, i], want[b, i])


def run(gt, disp, sizes, **kw):
    from evaluate import evaluate_depth
    return evaluate_depth(torch.from_numpy(gt).to(DEV), torch.from_numpy(disp).to(DEV)[:, None], sizes, per_image=True, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(median_scaling=False, scale=5.4), dict(crop=None), dict(crop="eigen"),
                                dict(crop=(100, 360, 30, 1190))])
def test_parity_at_kitti_sizes(kw):
    gt, disp = kitti_batch(KITTI_SIZES, 375, 1242, 192, 640, seed=11)
    got, rows = run(gt, disp, KITTI_SIZES, **kw)
    want, want_rows = R.evaluate(gt, disp, KITTI_SIZES, **kw)
    check_rows(rows, want_rows, str(kw))
    assert got["images"] == want["images"] == 4 and got["count"] == want["count"]
    for k in R.KEYS:
        tol = 2.0 / min(want_rows[:, 9]) if k in ("d1", "d2", "d3") else 1e-5 * abs(want[k])
        assert abs(got[k] - want[k]) <= tol, k
    assert abs(got["ratio_median"] - want["ratio_median"]) <= 2e-6 * abs(want["ratio_median"])
    if not kw.get("median_scaling", True):
        assert np.all(rows[:, 10].cpu().numpy() == 1.0)


def test_exact_median_at_identity_resolution():
    """h = Hg, w = Wg: up == disp, so pred is the float32 depth of each disparity and the ratio must be bit-equal to np.median's."""
    H, W = 24, 40
    rng = np.random.RandomState(4)
    cases = []
    def img(gvals, dvals):
        g = np.zeros((H, W), np.float32)
        d = rng.uniform(0.01, 0.5, (H, W)).astype(np.float32)
        idx = rng.choice(H * W, len(gvals), replace=False)
        g.flat[idx] = gvals
        if dvals is not None:
            d.flat[idx] = dvals
        return g, d
    cases.append(img(rng.uniform(1, 79, 301).astype(np.float32), None))                    # odd count
    cases.append(img(rng.uniform(1, 79, 500).astype(np.float32), None))                    # even count
    cases.append(img(np.array([17.25], np.float32), None))                                  # count 1
    cases.append(img(np.array([3.5, 60.0], np.float32), np.array([0.3, 0.02], np.float32)))  # count 2
    cases.append(img(np.full(200, 12.5, np.float32), np.full(200, 0.125, np.float32)))      # all equal
    cases.append(img((rng.randint(256 * 10, 256 * 11, 640) / 256).astype(np.float32),      # many duplicates (1/256 m steps)
                     rng.choice(np.array([0.1, 0.11, 0.12, 0.125], np.float32), 640)))
    dneg = rng.uniform(0.01, 0.5, 401).astype(np.float32)
    dneg[:7] = -rng.uniform(1e-4, 5e-4, 7)                                                  # a few negative disparities
    cases.append(img(rng.uniform(1, 79, 401).astype(np.float32), dneg))
    cases.append(img(np.zeros(0, np.float32), None))                                         # no valid pixel
    gt = np.stack([c[0] for c in cases])
    disp = np.stack([c[1] for c in cases])
    got, rows = run(gt, disp, None, crop=None)
    r = rows.cpu().numpy()
    for b in range(len(cases)):
        want, (mg, mp) = R.image_row(gt[b], disp[b], (0, H, 0, W), with_medians=True)
        assert r[b, 9] == want[9], b
        if want[9] == 0:
            assert np.isnan(r[b]).sum() == 10
            continue
        assert mg == np.median(gt[b][gt[b] > np.float32(1e-3)])
        assert np.float32(r[b, 10]).view(np.uint32) == np.float32(want[10]).view(np.uint32), (b, r[b, 10], want[10])
    assert got["images"] == len(cases) - 1 and got["count"] == int(r[:-1, 9].sum())
    assert [int(c) for c in r[:4, 9]] == [301, 500, 1, 2]
    assert r[7, 9] == 0 and got["abs_rel"] == pytest.approx(float(np.mean(r[:-1, 1].astype(np.float64))), rel=1e-12)


def test_padding_is_never_read_and_rows_reproduce():
    sizes = [(370, 1226), (360, 1200), (375, 1242)]
    gt0, disp = kitti_batch(sizes, 375, 1242, 192, 640, seed=21)
    gt1, _ = kitti_batch(sizes, 375, 1242, 192, 640, seed=21, pad=42.0)
    gt2 = gt1.copy()
    for b, (H, W) in enumerate(sizes):                  # garbage of every kind in the padding
        gt2[b, H:, :] = np.nan
        gt2[b, :, W:] = -np.inf
    _, a = run(gt0, disp, sizes)
    _, b_ = run(gt1, disp, sizes)
    _, c = run(gt2, disp, sizes)
    _, d = run(gt0, disp, sizes)
    for x in (b_, c, d):
        assert torch.equal(a.view(torch.int32), x.view(torch.int32))


def test_capture_replays_on_new_contents():
    import evaluate as E
    from mcav import lib as L
    sizes = KITTI_SIZES[:2]
    gtA, disp = kitti_batch(sizes, 375, 1242, 192, 640, seed=31)
    gtB, _ = kitti_batch(sizes, 375, 1242, 192, 640, seed=32)
    B = len(sizes)
    gt = torch.from_numpy(gtA).to(DEV)
    d = torch.from_numpy(disp).to(DEV)
    boxes = [R.crop_box(H, W, "garg") for H, W in sizes]
    meta = torch.tensor([v for s in sizes for v in s] + [v for bx in boxes for v in bx], dtype=torch.int32, device=DEV)
    h = L.lib()
    ws = torch.empty(h.mcav_eval_depth_workspace_bytes(B, 375, 1242), dtype=torch.uint8, device=DEV)
    rows = torch.full((B, 11), -1.0, device=DEV)
    call = lambda: L.check(h.mcav_eval_depth(L.ptr(gt), L.ptr(d), B, 375, 1242, 192, 640, L.ptr(meta), L.c_p(meta.data_ptr() + 8 * B),
                                             1e-3, 80.0, 1.0, E.EVAL_MEDIAN_SCALING, L.ptr(rows), L.ptr(ws), ws.numel(), L.stream()),
                           "mcav_eval_depth")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    gt.copy_(torch.from_numpy(gtB))
    g.replay()
    torch.cuda.synchronize()
    replayed = rows.clone()
    _, eager = run(gtB, disp, sizes)
    assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32))
    _, want = R.evaluate(gtB, disp, sizes)
    check_rows(replayed, want)


def test_invalid_arguments_are_rejected_untouched():
    from mcav import lib as L
    h = L.lib()
    B, Hg, Wg, hh, ww = 2, 32, 48, 16, 24
    gt = torch.ones(B, Hg, Wg, device=DEV)
    d = torch.full((B, hh, ww), 0.1, device=DEV)
    meta = torch.tensor([Hg, Wg] * B + [0, Hg, 0, Wg] * B, dtype=torch.int32, device=DEV)
    rows = torch.full((B, 11), 7.0, device=DEV)
    need = h.mcav_eval_depth_workspace_bytes(B, Hg, Wg)
    assert need > 0 and h.mcav_eval_depth_workspace_bytes(0, Hg, Wg) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    good = dict(gt=L.ptr(gt), disp=L.ptr(d), B=B, Hg=Hg, Wg=Wg, h=hh, w=ww, sizes=L.ptr(meta), boxes=L.c_p(meta.data_ptr() + 8 * B),
                lo=1e-3, hi=80.0, scale=1.0, flags=1, rows=L.ptr(rows), ws=L.ptr(ws), nws=need)
    def call(**kw):
        a = dict(good, **kw)
        return h.mcav_eval_depth(a["gt"], a["disp"], a["B"], a["Hg"], a["Wg"], a["h"], a["w"], a["sizes"], a["boxes"], a["lo"], a["hi"],
                                 a["scale"], a["flags"], a["rows"], a["ws"], a["nws"], L.stream())
    null = L.c_p(0)
    bad = [dict(gt=null), dict(disp=null), dict(sizes=null), dict(boxes=null), dict(rows=null), dict(ws=null),
           dict(B=0), dict(Hg=0), dict(Wg=-1), dict(h=0), dict(w=-3), dict(flags=2), dict(flags=-1), dict(lo=0.0), dict(lo=-1.0),
           dict(lo=float("nan")), dict(hi=1e-3), dict(hi=1e-4), dict(hi=float("nan")), dict(scale=float("inf")),
           dict(scale=float("nan"))]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(nws=need - 1) == -2
    torch.cuda.synchronize()
    assert bool((rows == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    ratio = np.float32(1.0) / (np.float32(1.0) / (np.float32(10) * np.float32(0.1) + np.float32(0.01)))      # gt 1 m, pred 1 / 1.01 m
    assert float(rows[0, 9]) == Hg * Wg and float(rows[0, 10]) == ratio


def test_loader_native_ground_truth(tmp_path):
    from PIL import Image
    from dataloaders import PrefetchLoader, UnSupKittiDataset, raw_collate
    from kitti_tree import SIZES, config_for, make_tree
    split, rows = make_tree(str(tmp_path))
    H, W = 24, 80
    cfg = config_for(split, str(tmp_path), H, W)
    default = UnSupKittiDataset(cfg)
    cfg["datasets"]["groundtruth"] = "native"
    native = UnSupKittiDataset(cfg)
    order = [0, 3, 4, 1, 5, 2]                            # batches (26, 28), (28, 26), (28, 26)
    mk = lambda ds, nat: PrefetchLoader(torch.utils.data.DataLoader(ds, batch_size=2, sampler=order, collate_fn=raw_collate), H, W, DEV,
                                        native_groundtruth=nat)
    seen = 0
    for bi, (a, b) in enumerate(zip(mk(native, True), mk(default, False))):
        assert torch.equal(a["tgt"], b["tgt"]) and all(torch.equal(x, y) for x, y in zip(a["ref_imgs"], b["ref_imgs"]))
        assert "groundtruth_size" not in b and tuple(b["groundtruth"].shape) == (2, 1, H, W)
        sz = a["groundtruth_size"]
        assert sz.dtype == torch.int32 and not sz.is_cuda and tuple(sz.shape) == (2, 2)
        gt = a["groundtruth"].cpu().numpy()
        assert gt.shape == (2, 1, 47, 156)
        for j in range(2):
            i = order[2 * bi + j]
            hw = SIZES["2011_09_26" if i < 3 else "2011_09_28"]
            assert tuple(sz[j].tolist()) == hw
            want = np.zeros((47, 156), np.float32)
            want[:hw[0], :hw[1]] = np.asarray(Image.open(rows[i][3]), dtype=np.float32) / 256
            assert np.array_equal(gt[j, 0], want)
            seen += 1
    assert seen == 6


def test_trainer_validation_protocol(tmp_path):
    from evaluate import evaluate_depth, reduce_rows, eval_depth_rows
    from kitti_tree import config_for, make_tree
    from trainer import Trainer
    split, _ = make_tree(str(tmp_path), frames=6)        # 8 samples, two image sizes
    cfg = config_for(split, str(tmp_path), 64, 128, batch=3)
    cfg["action"]["split"] = [0.5, 0.5]
    cfg["datasets"]["groundtruth"] = "native"
    cfg["validation"] = {"crop": "garg", "median_scaling": True}
    t = Trainer(cfg)
    got = t.validate()
    assert set(got) == set(R.KEYS) | {"images", "count", "ratio_median", "ratio_std"}
    assert got["images"] == 4 and got["count"] > 0 and all(np.isfinite(got[k]) for k in R.KEYS)
    assert t.depth_model.training
    t.depth_model.eval()                                # by hand: the same loader, depth predictions collected, then the protocol
    rows, n = [], 0
    with torch.no_grad():
        for s in t.validation_loader:
            disp = t.depth_model(s["tgt"])
            rows.append(evaluate_depth(s["groundtruth"], disp, s["groundtruth_size"], per_image=True)[1])
            n += s["tgt"].shape[0]
    t.set_train()
    assert n == 4
    want = reduce_rows(rows)
    for k in want:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), k
    cfg.pop("validation")
    assert Trainer(cfg).validation is None
    cfg["validation"] = {}
    cfg["datasets"].pop("groundtruth")
    with pytest.raises(ValueError, match="native"):
        Trainer(cfg).validate()
