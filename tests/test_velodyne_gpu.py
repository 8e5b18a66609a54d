"""GPU: KITTI Eigen ground truth from raw Velodyne scans (include/mcav_depth.h: mcav_velo_depth_map, geometry/velodyne.py), bit-exact
against the restatement tests/velo_ref.py: padded batches, constructed cases, flips, determinism, graph capture, rejected arguments,
generate_depth_map, the velodyne ground truth of PrefetchLoader and Trainer.validate() on it."""
import numpy as np
import pytest
import torch

import velo_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HG, WG = 375, 1242


def bits_equal(got, want):
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%d pixels differ, first %s: %r vs %r" % (int(bad.sum()), np.argwhere(bad)[0].tolist(), got[bad][:4], want[bad][:4])


def run(scans, Ps, sizes, Hg=None, Wg=None, flip=None, depth_from_x=False):
    from geometry.velodyne import depth_maps
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(scans)).to(DEV)
    out = depth_maps(pts, offsets, np.stack(Ps), sizes, Hg, Wg, flip=flip, depth_from_x=depth_from_x)
    assert out.dtype == torch.float32 and out.is_cuda
    return out[:, 0].cpu().numpy()


def test_parity_padded_batch():
    dates = ["2011_09_26", "2011_09_28", "2011_09_28", "2011_09_26"]
    scans = [V.scan(40 + i, n) for i, n in enumerate((120000, 97000, 131000, 64000))]
    Ps = [V.kitti_P(d) for d in dates]
    sizes = [V.KITTI_SIZES[d] for d in dates]
    got = run(scans, Ps, sizes)
    assert got.shape == (4, HG, WG)
    want = V.restated_batch(Ps, scans, sizes, HG, WG)
    assert all((want[b] > 0).sum() > 5000 for b in range(4))
    bits_equal(got, want)
    got2 = run(scans, Ps, sizes, 400, 1300)             # a larger padding is zero too
    bits_equal(got2, V.restated_batch(Ps, scans, sizes, 400, 1300))


def constructed():
    P26, P28 = V.kitti_P("2011_09_26"), V.kitti_P("2011_09_28")
    H, W = 375, 1242
    rng = np.random.RandomState(5)
    near = np.stack([np.array([rng.uniform(0.0, 0.2), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 0.5], np.float32)
                     for _ in range(200)])
    borders = np.stack([V.point_at(P26, W - 1, 100, 12.0), V.point_at(P26, 600, H - 1, 13.0), V.point_at(P26, W, 120, 14.0),
                        V.point_at(P26, 600, H, 15.0), V.point_at(P26, -1, 100, 16.0)])
    return [("edges", P26, V.edge_aliasing_case(P26, (H, W)), (H, W)),
            ("negative", P26, near, (H, W)),
            ("ties", V.P_DYADIC, V.tie_points(), (8, 8)),
            ("special", P28, np.concatenate([V.scan(7, 5000), V.special_points()]), (370, 1226)),
            ("overflow", V.P_OVERFLOW, np.array([[1e38, 2e38, 2e38, 0], [1, 1, 1, 0]], np.float32), (4, 4)),
            ("borders", P26, borders, (H, W))]


@pytest.mark.parametrize("depth_from_x", [False, True])
def test_constructed_cases(depth_from_x):
    cases = constructed()
    for name, P, pts, (H, W) in cases:
        got = run([pts], [P], [(H, W)], depth_from_x=depth_from_x)[0]
        bits_equal(got, V.restated(P, pts, (H, W), depth_from_x=depth_from_x))
        if name == "edges" and not depth_from_x:
            a = V.monodepth2(P, pts, (H, W)).astype(np.float32)
            assert np.array_equal(a[:, 1:-1], got[:, 1:-1]) and (a != got).any()
        if name == "overflow" and not depth_from_x:
            assert got[0, 0] == np.inf
        if name == "ties":
            assert sorted(map(tuple, np.argwhere(got > 0).tolist())) == [(1, 1), (1, 3)]
        if name == "borders":
            assert (got > 0).sum() == 2 and got[100, W - 1] > 0 and got[H - 1, 600] > 0
    # all of them in one padded batch
    Hg, Wg = max(c[3][0] for c in cases), max(c[3][1] for c in cases)
    got = run([c[2] for c in cases], [c[1] for c in cases], [c[3] for c in cases], Hg, Wg, depth_from_x=depth_from_x)
    bits_equal(got, V.restated_batch([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], Hg, Wg,
                                     depth_from_x=depth_from_x))


def test_flip_mirrors_within_true_width():
    dates = ["2011_09_28", "2011_09_26", "2011_09_28"]
    scans = [V.scan(60 + i, 50000) for i in range(3)]
    Ps = [V.kitti_P(d) for d in dates]
    sizes = [V.KITTI_SIZES[d] for d in dates]
    flips = [True, False, True]
    plain = run(scans, Ps, sizes)
    got = run(scans, Ps, sizes, flip=flips)
    bits_equal(got, V.restated_batch(Ps, scans, sizes, HG, WG, flips))
    for b, (H, W) in enumerate(sizes):
        want = np.zeros((HG, WG), np.float32)
        want[:H, :W] = plain[b, :H, :W][:, ::-1] if flips[b] else plain[b, :H, :W]
        bits_equal(got[b], want)


def test_deterministic_and_order_independent():
    dates = ["2011_09_26", "2011_09_28"]
    rng = np.random.RandomState(9)
    scans = [np.concatenate([V.scan(70 + i, 80000), V.edge_aliasing_case(V.kitti_P(d), V.KITTI_SIZES[d], seed=i)])
             for i, d in enumerate(dates)]
    Ps = [V.kitti_P(d) for d in dates]
    sizes = [V.KITTI_SIZES[d] for d in dates]
    first = run(scans, Ps, sizes)
    for _ in range(3):
        bits_equal(run(scans, Ps, sizes), first)
    shuffled = [s[rng.permutation(len(s))] for s in scans]
    bits_equal(run(shuffled, Ps, sizes), first)
    bits_equal(first, V.restated_batch(Ps, scans, sizes, HG, WG))


def raw_call(h, L, pts, offs, P, sizes, flip, B, Hg, Wg, max_points, flags, out):
    return h.mcav_velo_depth_map(L.ptr(pts), L.ptr(offs), L.ptr(P), L.ptr(sizes), L.ptr(flip), B, Hg, Wg, max_points, flags, L.ptr(out),
                                 L.stream())


def test_capture_replays_on_new_batch():
    from mcav import lib as L
    import geometry.velodyne  # noqa: F401  (registers the signature)
    h = L.lib()
    cap = 120000
    B = 3
    pts = torch.zeros((B * cap, 4), dtype=torch.float32, device=DEV)
    offs = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    P = torch.zeros((B, 12), dtype=torch.float64, device=DEV)
    sizes = torch.zeros((B, 2), dtype=torch.int32, device=DEV)
    flip = torch.zeros(B, dtype=torch.uint8, device=DEV)
    out = torch.full((B, HG, WG), 7.0, device=DEV)

    def load(seed, dates, ns, flips):
        scans = [V.scan(seed + i, n) for i, n in enumerate(ns)]
        Ps = [V.kitti_P(d) for d in dates]
        szs = [V.KITTI_SIZES[d] for d in dates]
        o = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        pts[:o[-1]].copy_(torch.from_numpy(np.concatenate(scans)))
        offs.copy_(torch.from_numpy(o))
        P.copy_(torch.from_numpy(np.stack(Ps).reshape(B, 12)))
        sizes.copy_(torch.tensor(szs, dtype=torch.int32))
        flip.copy_(torch.tensor(flips, dtype=torch.uint8))
        return V.restated_batch(Ps, scans, szs, HG, WG, flips)

    wantA = load(80, ["2011_09_26", "2011_09_28", "2011_09_26"], [100000, 120000, 90000], [0, 1, 0])
    call = lambda: L.check(raw_call(h, L, pts, offs, P, sizes, flip, B, HG, WG, cap, 0, out), "mcav_velo_depth_map")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    bits_equal(out.cpu().numpy(), wantA)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    wantB = load(90, ["2011_09_28", "2011_09_26", "2011_09_28"], [120000, 50000, 110000], [1, 0, 1])
    out.fill_(-3.0)
    g.replay()
    torch.cuda.synchronize()
    bits_equal(out.cpu().numpy(), wantB)


def test_invalid_arguments_are_rejected_untouched():
    from mcav import lib as L
    import geometry.velodyne  # noqa: F401
    h = L.lib()
    B, Hg, Wg = 2, 32, 48
    pts = torch.from_numpy(V.scan(3, 1000)).to(DEV)
    offs = torch.tensor([0, 500, 1000], dtype=torch.int64, device=DEV)
    P = torch.from_numpy(np.stack([V.kitti_P("2011_09_26")] * B).reshape(B, 12)).to(DEV)
    sizes = torch.tensor([[Hg, Wg]] * B, dtype=torch.int32, device=DEV)
    flip = torch.zeros(B, dtype=torch.uint8, device=DEV)
    out = torch.full((B, Hg, Wg), 7.0, device=DEV)
    good = dict(pts=pts, offs=offs, P=P, sizes=sizes, flip=flip, B=B, Hg=Hg, Wg=Wg, mp=500, flags=0)

    def call(**kw):
        a = dict(good, **kw)
        return raw_call(h, L, a["pts"], a["offs"], a["P"], a["sizes"], a["flip"], a["B"], a["Hg"], a["Wg"], a["mp"], a["flags"], out)
    bad = [dict(pts=None), dict(offs=None), dict(P=None), dict(sizes=None), dict(B=0), dict(B=-1), dict(Hg=0), dict(Wg=-2),
           dict(mp=-1), dict(flags=2), dict(flags=-1), dict(B=70000), dict(Hg=1 << 30, Wg=1 << 30)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert h.mcav_velo_depth_map(L.ptr(pts), L.ptr(offs), L.ptr(P), L.ptr(sizes), L.ptr(flip), B, Hg, Wg, 500, 0, L.c_p(0), L.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(flip=None) == 0 and call(mp=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())                      # no point taken: every pixel +0.0
    assert call() == 0
    torch.cuda.synchronize()
    scans = [V.scan(3, 1000)[:500], V.scan(3, 1000)[500:]]
    bits_equal(out.cpu().numpy(), V.restated_batch([V.kitti_P("2011_09_26")] * B, scans, [(Hg, Wg)] * B, Hg, Wg))


def test_generate_depth_map_on_tree(tmp_path):
    import os
    from geometry.velodyne import generate_depth_map, load_velodyne_points, velo_to_image
    from kitti_tree import SIZES
    from kitti_velo_tree import make_velo_tree
    _, _, scans = make_velo_tree(str(tmp_path), frames=3)
    for img, path in scans.items():
        date = "2011_09_26" if "2011_09_26" in img else "2011_09_28"
        calib = os.path.join(str(tmp_path), "KITTI", date)
        got = generate_depth_map(calib, path)
        assert got.dtype == np.float32 and got.shape == SIZES[date]
        P, hw = velo_to_image(calib)
        velo = load_velodyne_points(path)
        bits_equal(got, V.restated(P, velo, hw))
        assert (got > 0).sum() > 200
        a = V.monodepth2(P, velo, hw).astype(np.float32)
        assert np.array_equal(a[:, 1:-1], got[:, 1:-1])
        bits_equal(generate_depth_map(calib, path, vel_depth=True), V.restated(P, velo, hw, depth_from_x=True))


def test_loader_velodyne_ground_truth(tmp_path):
    from dataloaders import PrefetchLoader, UnSupKittiDataset, raw_collate
    from geometry.velodyne import load_velodyne_points
    from kitti_tree import SIZES, config_for
    from kitti_velo_tree import make_velo_tree, tree_P, velo_config
    split, rows, scans = make_velo_tree(str(tmp_path))
    H, W = 24, 80
    default = UnSupKittiDataset(config_for(split, str(tmp_path), H, W))
    velo = UnSupKittiDataset(velo_config(split, str(tmp_path), H, W))
    order = [0, 3, 4, 1, 5, 2]                            # batches (26, 28), (28, 26), (28, 26)
    mk = lambda ds, nat: PrefetchLoader(torch.utils.data.DataLoader(ds, batch_size=2, sampler=order, collate_fn=raw_collate), H, W, DEV,
                                        native_groundtruth=nat)
    seen = 0
    for bi, (a, b) in enumerate(zip(mk(velo, True), mk(default, False))):
        assert torch.equal(a["tgt"], b["tgt"]) and all(torch.equal(x, y) for x, y in zip(a["ref_imgs"], b["ref_imgs"]))
        sz = a["groundtruth_size"]
        assert sz.dtype == torch.int32 and not sz.is_cuda and tuple(sz.shape) == (2, 2)
        gt = a["groundtruth"]
        assert gt.is_cuda and gt.dtype == torch.float32
        gt = gt.cpu().numpy()
        assert gt.shape == (2, 1, 47, 156)
        for j in range(2):
            i = order[2 * bi + j]
            date = "2011_09_26" if i < 3 else "2011_09_28"
            hw = SIZES[date]
            assert tuple(sz[j].tolist()) == hw
            want = np.zeros((47, 156), np.float32)
            want[:hw[0], :hw[1]] = V.restated(tree_P(date), load_velodyne_points(scans[rows[i][0]]), hw)
            assert (want > 0).sum() > 200
            bits_equal(gt[j, 0], want)
            seen += 1
    assert seen == 6


def test_loader_velodyne_flip(tmp_path):
    from dataloaders import Augmentation, PrefetchLoader, UnSupKittiDataset, raw_collate
    from geometry.velodyne import load_velodyne_points
    from kitti_tree import SIZES
    from kitti_velo_tree import make_velo_tree, tree_P, velo_config
    split, rows, scans = make_velo_tree(str(tmp_path))
    H, W = 24, 80
    ds = UnSupKittiDataset(velo_config(split, str(tmp_path), H, W))
    order = [0, 3, 4, 1, 5, 2]
    aug = Augmentation(p_color=0.0, p_flip=0.5, seed=2)            # 3 of the 6 samples flipped
    loader = PrefetchLoader(torch.utils.data.DataLoader(ds, batch_size=2, sampler=order, collate_fn=raw_collate), H, W, DEV,
                            native_groundtruth=True, augment=aug)
    flips = 0
    for bi, a in enumerate(loader):
        gt = a["groundtruth"].cpu().numpy()
        f = (a["augment_records"]["flags"] & 1) != 0
        for j in range(2):
            i = order[2 * bi + j]
            date = "2011_09_26" if i < 3 else "2011_09_28"
            hw = SIZES[date]
            want = np.zeros(gt.shape[2:], np.float32)
            want[:hw[0], :hw[1]] = V.restated(tree_P(date), load_velodyne_points(scans[rows[i][0]]), hw, flip=bool(f[j]))
            bits_equal(gt[j, 0], want)
            flips += int(f[j])
    assert 0 < flips < 6


def test_trainer_validation_on_velodyne(tmp_path):
    import eval_protocol_ref as R
    from evaluate import evaluate_depth, reduce_rows
    from kitti_velo_tree import make_velo_tree, velo_config
    from trainer import Trainer
    split, _, _ = make_velo_tree(str(tmp_path), frames=6)     # 8 samples, two image sizes
    cfg = velo_config(split, str(tmp_path), 64, 128, batch=3)
    cfg["action"]["split"] = [0.5, 0.5]
    cfg["validation"] = {"crop": "garg"}
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
