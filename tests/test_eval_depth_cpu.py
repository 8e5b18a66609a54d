"""CPU: the KITTI depth evaluation protocol (include/mcav_depth.h: mcav_eval_depth, evaluate.evaluate_depth).  The restatement
(tests/eval_protocol_ref.py) against a literal per-image transcription of monodepth2's evaluation loop; the per-pixel header
csrc/eval_math.h compiled for the host (depth conversion, order-preserving key, bilinear sample, median of two); the host side of
evaluate.py and the native ground truth of the KITTI reader."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import eval_protocol_ref as R
from conftest import PKG, REPO

MIN_DEPTH, MAX_DEPTH = 1e-3, 80


def literal(gt_depths, pred_disps, crop="garg", median_scaling=True, scale=1.0):
    """monodepth2 evaluate_depth.py's loop, transcribed: per image resize the disparity to the ground truth's size (torch's bilinear, as
    cv2 is not available), this repository's disp -> depth, crop mask, median scaling, clip, errors; then the mean over images."""
    errors, ratios = [], []
    for i in range(len(pred_disps)):
        gt_depth = gt_depths[i]
        gt_height, gt_width = gt_depth.shape[:2]
        pred_disp = torch.nn.functional.interpolate(torch.from_numpy(pred_disps[i])[None, None], size=(gt_height, gt_width),
                                                    mode="bilinear", align_corners=False)[0, 0].numpy()
        pred_depth = 1 / (10 * pred_disp + 0.01)
        mask = np.logical_and(gt_depth > MIN_DEPTH, gt_depth < MAX_DEPTH)
        if crop is not None:
            f = {"garg": [0.40810811, 0.99189189, 0.03594771, 0.96405229], "eigen": [0.3324324, 0.91351351, 0.0359477, 0.96405229]}[crop]
            c = np.array([f[0] * gt_height, f[1] * gt_height, f[2] * gt_width, f[3] * gt_width]).astype(np.int32)
            crop_mask = np.zeros(mask.shape)
            crop_mask[c[0]:c[1], c[2]:c[3]] = 1
            mask = np.logical_and(mask, crop_mask)
        pred_depth = pred_depth[mask]
        gt_depth = gt_depth[mask]
        pred_depth *= scale
        if median_scaling:
            ratio = np.median(gt_depth) / np.median(pred_depth)
            ratios.append(ratio)
            pred_depth *= ratio
        pred_depth[pred_depth < MIN_DEPTH] = MIN_DEPTH
        pred_depth[pred_depth > MAX_DEPTH] = MAX_DEPTH
        g, p = gt_depth.astype(np.float64), pred_depth.astype(np.float64)
        thresh = np.maximum(g / p, p / g)
        err = np.log(p) - np.log(g)
        errors.append([np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100, np.mean(np.abs(g - p) / g),
                       np.mean(np.abs(np.log10(p) - np.log10(g))), np.sqrt(((g - p) ** 2).mean()), np.mean((g - p) ** 2 / g),
                       np.sqrt(((np.log(g) - np.log(p)) ** 2).mean()), (thresh < 1.25).mean(), (thresh < 1.25 ** 2).mean(),
                       (thresh < 1.25 ** 3).mean()])
    return np.array(errors).mean(0), np.array(ratios)


def kitti_like(sizes, h, w, seed, density=0.3):
    """Sparse metric ground truth quantised to 1/256 m (KITTI's PNG units) at each image's own size, and sigmoid disparities."""
    rng = np.random.RandomState(seed)
    gts, disps = [], []
    for (H, W) in sizes:
        gt = (np.round(rng.uniform(1.0, 90.0, (H, W)) * 256) / 256).astype(np.float32)
        gt[rng.rand(H, W) > density] = 0
        gts.append(gt)
        disps.append(rng.uniform(0.01, 0.6, (h, w)).astype(np.float32))
    return gts, disps


@pytest.mark.parametrize("crop", ["garg", "eigen", None])
@pytest.mark.parametrize("median_scaling,scale", [(True, 1.0), (False, 5.4)])
def test_restatement_is_monodepth2_loop(crop, median_scaling, scale):
    sizes = [(75, 248), (74, 245), (75, 248), (61, 203)]
    gts, disps = kitti_like(sizes, 24, 80, seed=3)
    want, want_ratios = literal(gts, disps, crop, median_scaling, scale)
    Hg, Wg = max(s[0] for s in sizes), max(s[1] for s in sizes)
    padded = np.zeros((len(sizes), Hg, Wg), np.float32)
    for b, g in enumerate(gts):
        padded[b, :g.shape[0], :g.shape[1]] = g
    got, rows = R.evaluate(padded, np.stack(disps), sizes, crop, median_scaling=median_scaling, scale=scale)
    for i, k in enumerate(R.KEYS):
        assert abs(got[k] - want[i]) <= 1e-12 * max(1.0, abs(want[i])), k
    counts = rows[:, 9]
    assert got["images"] == len(sizes) and got["count"] == counts.sum()
    assert len(set(int(c) % 2 for c in counts)) == 2, "the case covers odd and even counts"
    if median_scaling:
        assert np.array_equal(rows[:, 10].astype(np.float32), want_ratios.astype(np.float32))
        assert got["ratio_median"] == np.median(rows[:, 10])
        assert abs(got["ratio_std"] - np.std(rows[:, 10] / np.median(rows[:, 10]))) <= 1e-15


def test_restatement_empty_image_and_medians():
    gts, disps = kitti_like([(20, 30)] * 3, 10, 15, seed=4)
    gts[1][:] = 0                                        # no return at all
    got, rows = R.evaluate(np.stack(gts), np.stack(disps), crop=None)
    assert rows[1, 9] == 0 and np.isnan(rows[1, :9]).all() and np.isnan(rows[1, 10])
    assert got["images"] == 2
    assert got["abs_rel"] == np.mean(rows[[0, 2], 1])
    for n in (1, 2, 7, 8):                              # the medians are np.median's, odd and even counts
        g = np.zeros((20, 30), np.float32)
        g.flat[:n] = np.arange(1, n + 1, dtype=np.float32) * 1.5
        row, med = R.image_row(g, disps[0], (0, 20, 0, 30), with_medians=True)
        assert row[9] == n and med[0] == np.median(g.flat[:n])


def test_crop_boxes():
    import evaluate as E
    for Hb, Wb in ((375, 1242), (370, 1226), (374, 1238), (376, 1241), (1, 1)):
        for crop in ("garg", "eigen", None, (3, 9, 2, 11)):
            assert E.crop_box(Hb, Wb, crop) == R.crop_box(Hb, Wb, crop)
    assert R.crop_box(375, 1242, "garg") == (153, 371, 44, 1197)
    with pytest.raises(Exception):
        E.crop_box(375, 1242, "kitti")


def test_reduce_rows_matches_restatement():
    import evaluate as E
    rng = np.random.RandomState(1)
    rows = rng.rand(7, 11).astype(np.float32)
    rows[:, 9] = [5, 0, 3, 9, 1, 2, 0]
    rows[[1, 6], :9] = np.nan
    rows[[1, 6], 10] = np.nan
    got = E.reduce_rows([torch.from_numpy(rows[:3]), torch.from_numpy(rows[3:])])
    want = R.reduce_rows(rows)
    assert set(got) == set(want) == set(R.KEYS) | {"images", "count", "ratio_median", "ratio_std"}
    for k in want:
        assert got[k] == want[k], k


# ---------------------------------------------------------------------------------------------- csrc/eval_math.h on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("eval_hostcheck") / "libeval_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(REPO, "tests", "eval_hostcheck", "eval_hostcheck.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    P = ctypes.c_void_p
    lib.ev_depth.argtypes = [P, ctypes.c_float, P, ctypes.c_int]
    lib.ev_keys.argtypes = [P, P, P, ctypes.c_int]
    lib.ev_resize.argtypes = [P] + [ctypes.c_int] * 4 + [P]
    lib.ev_median.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_uint]
    lib.ev_median.restype = ctypes.c_float
    return lib


def p_(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("scale", [1.0, 5.4, 0.37])
def test_depth_conversion_is_numpy_float32(host, scale):
    rng = np.random.RandomState(2)
    d = np.concatenate([rng.rand(20000), -rng.rand(2000) * 1e-3, rng.rand(2000) * 1e-6, [0.0, 1.0, -0.0009, 1e-30]]).astype(np.float32)
    out = np.empty_like(d)
    host.ev_depth(p_(d), scale, p_(out), d.size)
    want = R.depth_of(d, scale)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_float_key_preserves_order(host):
    rng = np.random.RandomState(5)
    specials = np.array([np.inf, -np.inf, 0.0, -0.0, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny,
                         -np.finfo(np.float32).tiny, 1e-45, -1e-45, 1.0, -1.0], np.float32)
    x = np.concatenate([specials, (rng.randn(5000) * 10.0 ** rng.randint(-30, 30, 5000)).astype(np.float32)])
    keys = np.empty(x.size, np.uint32)
    back = np.empty_like(x)
    host.ev_keys(p_(x), p_(keys), p_(back), x.size)
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))          # the key is a bijection
    o = np.argsort(keys, kind="stable")
    xs, ks = x[o], keys[o]
    assert np.all(xs[1:] >= xs[:-1])                                        # sorting by key sorts the values
    lt = x[:, None] < x[None, :]
    ka, kb = np.broadcast_arrays(keys[:, None], keys[None, :])
    assert np.all(ka[lt] < kb[lt])                                          # a < b => key(a) < key(b), every pair
    k = keys[:12]              # inf, -inf, +0, -0, max, -max, tiny, -tiny, +denorm, -denorm, 1, -1
    assert k[1] < k[5] < k[11] < k[7] < k[9] < k[3] < k[2] < k[8] < k[6] < k[10] < k[4] < k[0]
    assert ks[0] == k[1] and ks[-1] == k[0]


@pytest.mark.parametrize("h,w,H,W", [(24, 80, 75, 248), (192, 640, 375, 1242), (192, 640, 370, 1226), (7, 9, 7, 9), (10, 12, 5, 30)])
def test_bilinear_sample_matches_interpolate(host, h, w, H, W):
    rng = np.random.RandomState(h + W)
    disp = rng.rand(h, w).astype(np.float32)
    out = np.empty((H, W), np.float32)
    host.ev_resize(p_(disp), h, w, H, W, p_(out))
    want = R.upsample(disp, H, W)
    ulp = np.abs(out.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp.max() <= 2, ulp.max()
    if (h, w) == (H, W):
        assert np.array_equal(out, disp)


def test_median_of_two_is_numpy(host):
    rng = np.random.RandomState(8)
    for _ in range(2000):
        a, b = np.sort(rng.randn(2).astype(np.float32) * np.float32(10.0 ** rng.randint(-5, 5)))
        assert host.ev_median(a, b, 2) == np.median(np.array([a, b], np.float32))
        assert host.ev_median(a, a, 3) == a


# ---------------------------------------------------------------------------------------------- the reader's native ground truth
def test_native_ground_truth_is_png_over_256(tmp_path):
    from PIL import Image
    from dataloaders import UnSupKittiDataset
    from kitti_tree import SIZES, config_for, make_tree
    split, rows = make_tree(str(tmp_path))
    cfg = config_for(split, str(tmp_path))
    default = UnSupKittiDataset(cfg, transforms=None)
    cfg["datasets"]["groundtruth"] = "native"
    ds = UnSupKittiDataset(cfg, transforms=None)
    for idx in (0, 5):
        s, d = ds[idx], default[idx]
        png = np.asarray(Image.open(rows[idx][3]), dtype=np.float32)
        assert tuple(png.shape) == SIZES["2011_09_26" if idx < 3 else "2011_09_28"]
        assert s["groundtruth"].dtype == torch.float32 and tuple(s["groundtruth"].shape) == (1,) + png.shape
        assert np.array_equal(s["groundtruth"][0].numpy(), png / 256)
        assert torch.equal(s["tgt"], d["tgt"]) and torch.equal(s["intrinsics"], d["intrinsics"])
        assert tuple(d["groundtruth"].shape) == (1, 24, 80)                 # the default is unchanged
    cfg["datasets"]["groundtruth"] = "metres"
    with pytest.raises(ValueError, match="groundtruth"):
        UnSupKittiDataset(cfg, transforms=None)
