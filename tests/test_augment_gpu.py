"""GPU: the augmentation kernels (include/mcav_depth.h: mcav_image_preprocess_augment) bit for bit against tests/augment_ref.py and the
pinned Pillow fixture, the plain output against GpuImageTransform, reproducibility, PrefetchLoader with an Augmentation on a KITTI-shaped
tree, the flip equivariance of the loss that fixes the intrinsics rule, and the trainer with augmentation on."""
import itertools

import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def frames_of(n, H0, W0, seed):
    """Noise over smooth ramps: both flat regions (ties, grey pixels) and every byte value."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H0, 0:W0]
    out = np.empty((n, H0, W0, 3), np.uint8)
    for i in range(n):
        ramp = np.stack([(xx * (i + 1)) % 256, (yy * 3 + i * 17) % 256, ((xx + yy) // 2) % 256], -1)
        noise = rng.randint(0, 256, (H0, W0, 3))
        out[i] = np.where(rng.rand(H0, W0, 1) < 0.3, noise, ramp).astype(np.uint8)
    return out


def coverage_records():
    """36 records: all 24 orders (flip alternating, factors 0.8 / 1.2, hue +-0.1 / +-0.5), colour off with and without flip, identity
    colour (aug == plain) with and without flip, and six drawn by Augmentation."""
    from dataloaders import AUGMENT_RECORD, AUG_OP_NONE, Augmentation
    rec = np.zeros(36, AUGMENT_RECORD)
    for k, order in enumerate(itertools.permutations(range(4))):
        rec[k]["flags"] = R.COLOUR | (R.FLIP if k % 2 else 0)
        rec[k]["order"] = order
        lo, hi = np.float32(0.8), np.float32(1.2)
        rec[k]["brightness"], rec[k]["contrast"], rec[k]["saturation"] = (lo, hi, lo) if k % 3 else (hi, lo, hi)
        rec[k]["hue_shift"] = R.hue_shift_of([0.1, -0.1, 0.5, -0.5][k % 4])
    rec[24]["flags"], rec[25]["flags"] = 0, R.FLIP
    for i in (26, 27):
        rec[i]["flags"] = R.COLOUR | (R.FLIP if i == 27 else 0)
        rec[i]["order"] = (2, 0, AUG_OP_NONE, 1)
        rec[i]["brightness"] = rec[i]["contrast"] = rec[i]["saturation"] = 1.0
    a = Augmentation(p_color=0.8, p_flip=0.5, seed=5)
    rec[28:] = a.draw(a.generator(0), 8)
    return rec


def run_kernel(frames, records, h, w):
    from dataloaders import GpuImageTransform
    t = GpuImageTransform(h, w, DEV)
    plain, aug = t.augmented(torch.from_numpy(frames), records)
    torch.cuda.synchronize()
    return plain, aug


@pytest.mark.parametrize("H0,W0", [(375, 1242), (370, 1226)])
def test_kernel_matches_restatement_at_kitti_sizes(H0, W0):
    from dataloaders import GpuImageTransform
    h, w = 192, 640
    frames = frames_of(36, H0, W0, seed=H0)
    rec = coverage_records()
    plain, aug = run_kernel(frames, rec, h, w)
    want_plain, want_aug = R.expected(frames, rec, h, w)
    got_plain, got_aug = plain.cpu().numpy(), aug.cpu().numpy()
    bad = [i for i in range(36) if not np.array_equal(got_plain[i], want_plain[i])]
    assert not bad, ("plain", bad)
    bad = [i for i in range(36) if not np.array_equal(got_aug[i], want_aug[i])]
    assert not bad, ("aug", bad, [rec[i] for i in bad[:3]])
    for i in (26, 27):                                              # identity colour: aug == plain
        assert torch.equal(aug[i], plain[i])
    # the plain output is today's transform, mirrored where the record flips
    base = GpuImageTransform(h, w, DEV)(torch.from_numpy(frames))
    flip = torch.from_numpy((rec["flags"] & R.FLIP) != 0).to(DEV)
    assert torch.equal(plain, torch.where(flip[:, None, None, None], base.flip(-1), base))
    # reproducible from run to run
    plain2, aug2 = run_kernel(frames, rec, h, w)
    assert torch.equal(plain, plain2) and torch.equal(aug, aug2)


def test_kernel_matches_pinned_pillow_fixture(golden):
    from dataloaders import AUGMENT_RECORD
    g = golden("augment.npz")
    h, w = (int(v) for v in g["size"])
    rec = g["records"].reshape(-1).view(AUGMENT_RECORD)
    plain, aug = run_kernel(g["frames"], rec, h, w)
    want_plain = np.stack([R.normalise(p) for p in g["plain"]])
    want_aug = np.stack([R.normalise(a) for a in g["aug"]])
    assert np.array_equal(plain.cpu().numpy(), want_plain)
    assert np.array_equal(aug.cpu().numpy(), want_aug)


def test_invalid_arguments_are_rejected():
    import mcav.lib as L
    from dataloaders import AUGMENT_RECORD, GpuImageTransform
    t = GpuImageTransform(24, 80, DEV)
    x = torch.zeros(2, 47, 156, 3, dtype=torch.uint8)
    with pytest.raises(L.MCAVError):
        t.augmented(x, np.zeros(3, AUGMENT_RECORD))
    with pytest.raises(L.MCAVError):
        t.augmented(x.float(), np.zeros(2, AUGMENT_RECORD))
    h = L.lib()
    assert h.mcav_image_preprocess_augment(None, 2, 47, 156, 24, 80, None, None, 3, None, None, 3, None, None, None, None, None, None, 0,
                                           None) == -1
    assert h.mcav_image_augment_workspace_bytes(0, 47, 24, 80) == 0


# ---------------------------------------------------------------------------------------------------- PrefetchLoader
def _aug_config(split, root, H, W, batch=2):
    from kitti_tree import config_for
    cfg = config_for(split, root, H, W, batch)
    cfg["datasets"]["augmentation"].update(color_jitter={"brightness": 0.2, "contrast": 0.2, "saturation": 0.2, "hue": 0.1, "p": 0.5},
                                           flip=0.5)
    return cfg


def test_loader_batches(tmp_path):
    from PIL import Image
    from dataloaders import AUG_FLIP, Augmentation, PrefetchLoader, UnSupKittiDataset, raw_collate
    from kitti_tree import make_tree
    split, rows = make_tree(str(tmp_path), frames=6)
    H, W = 24, 80
    cfg = _aug_config(split, str(tmp_path), H, W)
    ds = UnSupKittiDataset(cfg)
    aug = Augmentation(p_color=0.7, p_flip=0.5, seed=11)
    order = list(range(len(ds)))
    mk = lambda nw, a: PrefetchLoader(torch.utils.data.DataLoader(ds, batch_size=2, sampler=order, collate_fn=raw_collate, num_workers=nw),
                                      H, W, DEV, augment=a)
    plain_loader = mk(0, None)
    runs = []
    for nw in (0, 2):
        ld = mk(nw, aug)
        ld.set_epoch(3)
        runs.append(ld_iter(ld))
    a0, a2 = runs
    assert len(a0) == len(a2) == len(order) // 2
    flips = 0
    for (b0, b2, p) in zip(a0, a2, plain_loader):
        assert set(b0) == {"tgt", "ref_imgs", "intrinsics", "groundtruth", "tgt_aug", "ref_imgs_aug", "augment_records"}
        assert set(p) == {"tgt", "ref_imgs", "intrinsics", "groundtruth"}
        assert np.array_equal(b0["augment_records"], b2["augment_records"])
        for k in ("tgt", "tgt_aug", "intrinsics", "groundtruth"):
            assert torch.equal(b0[k], b2[k]), k
        recs = b0["augment_records"]
        for j in range(2):
            flip = bool(recs[j]["flags"] & AUG_FLIP)
            flips += flip
            Kp, Ka = p["intrinsics"][j].cpu(), b0["intrinsics"][j].cpu()
            if flip:
                assert float(Ka[0, 2]) == (W - 1) - float(Kp[0, 2])
                Ka = Ka.clone()
                Ka[0, 2], Ka[0, 1] = Kp[0, 2], -Ka[0, 1]
                assert torch.equal(b0["groundtruth"][j], p["groundtruth"][j].flip(-1))
            else:
                assert torch.equal(b0["groundtruth"][j], p["groundtruth"][j])
            assert torch.equal(Ka, Kp)
    assert 0 < flips < len(order)
    # the frames: the reference chain on the decoded files with the batch's records
    b0 = a0[0]
    recs = b0["augment_records"]
    for key, col in (("tgt", 0), ("ref_imgs", 1), ("ref_imgs", 2)):
        src = np.stack([np.asarray(Image.open(rows[i][col]).convert("RGB")) for i in order[:2]])
        want_plain, want_aug = R.expected(src, recs, H, W)
        got_p = b0[key] if key == "tgt" else b0[key][col - 1]
        got_a = b0[key + "_aug"] if key == "tgt" else b0["ref_imgs_aug"][col - 1]
        assert np.array_equal(got_p.cpu().numpy(), want_plain) and np.array_equal(got_a.cpu().numpy(), want_aug), key
    # a new epoch draws new records
    ld = mk(0, aug)
    ld.set_epoch(4)
    assert not all(np.array_equal(x["augment_records"], y["augment_records"]) for x, y in zip(ld_iter(ld), a0))


def ld_iter(ld):
    out = []
    for b in ld:
        c = dict(b)
        for k in ("tgt", "tgt_aug", "intrinsics", "groundtruth"):
            c[k] = b[k].clone()
        c["ref_imgs"] = [x.clone() for x in b["ref_imgs"]]
        c["ref_imgs_aug"] = [x.clone() for x in b["ref_imgs_aug"]]
        out.append(c)
    torch.cuda.synchronize()
    return out


def test_native_ground_truth_is_mirrored_within_its_size(tmp_path):
    from dataloaders import AUG_FLIP, Augmentation, PrefetchLoader, UnSupKittiDataset, raw_collate
    from kitti_tree import make_tree
    split, _ = make_tree(str(tmp_path))
    cfg = _aug_config(split, str(tmp_path), 24, 80)
    cfg["datasets"]["groundtruth"] = "native"
    ds = UnSupKittiDataset(cfg)
    order = [0, 3, 4, 1, 5, 2]                                     # mixed sizes in every batch: zero padding on the right
    mk = lambda a: PrefetchLoader(torch.utils.data.DataLoader(ds, batch_size=2, sampler=order, collate_fn=raw_collate), 24, 80, DEV,
                                  native_groundtruth=True, augment=a)
    a = Augmentation(p_color=0.0, p_flip=1.0)
    for x, y in zip(mk(a), mk(None)):
        assert (x["augment_records"]["flags"] & AUG_FLIP).all()
        for j, (Hb, Wb) in enumerate(y["groundtruth_size"].tolist()):
            gx, gy = x["groundtruth"][j, 0], y["groundtruth"][j, 0]
            assert torch.equal(gx[:Hb, :Wb], gy[:Hb, :Wb].flip(-1))
            assert not gx[:, Wb:].any() and not gx[Hb:].any()
            assert torch.equal(x["tgt_aug"][j], x["tgt"][j]) and torch.equal(x["tgt"][j], y["tgt"][j].flip(-1))


# ---------------------------------------------------------------------------------------------------- why cx' = w - 1 - cx
def test_loss_is_flip_equivariant_with_mirrored_intrinsics():
    from losses import Losses
    from oracle.step import synthetic_batch
    B, H, W = 2, 64, 128
    s = synthetic_batch(B, H, W, seed=21)
    tgt, refs = s["tgt"].to(DEV), [r.to(DEV) for r in s["ref_imgs"]]
    K = s["intrinsics"].to(DEV).clone()
    K[:, 0, 2] = 0.41 * W                                           # off-centre, as KITTI's P_rect_02 at 640 wide
    g = torch.Generator().manual_seed(4)
    disps = [[(0.05 + 0.2 * torch.rand(B, 1, H, W, generator=g)).to(DEV)] for _ in range(2)]
    poses = 0.02 * torch.randn(B, 2, 6, generator=g)
    poses[..., 5] += 0.15                                           # forward motion: the principal point matters
    poses[..., 1] += 0.05
    poses = poses.to(DEV)
    mirror_pose = torch.tensor([1.0, -1.0, -1.0, -1.0, 1.0, 1.0], device=DEV)       # (vx, -vy, -vz, -tx, ty, tz)
    Km = K.clone()
    Km[:, 0, 2] = (W - 1) - K[:, 0, 2]

    def loss(t, r, d, p, k):
        return [float(x) for x in Losses().forward(t, r, d, p, k, None)]
    base = loss(tgt, refs, disps, poses, K)
    fl = lambda x: x.flip(-1).contiguous()
    args = (fl(tgt), [fl(r) for r in refs], [[fl(d[0])] for d in disps], poses * mirror_pose)
    mirrored = loss(*args, Km)
    for a, b in zip(base, mirrored):
        assert abs(a - b) <= 1e-5 * abs(a), (base, mirrored)
    unmirrored = loss(*args, K)                                     # the principal point left where it was: a different loss
    d_ok, d_bad = abs(mirrored[0] - base[0]), abs(unmirrored[0] - base[0])
    assert d_bad > 1e-4 * abs(base[0]) and d_bad > 50 * max(d_ok, 1e-7 * abs(base[0])), (base, mirrored, unmirrored)


# ---------------------------------------------------------------------------------------------------- the trainer
def _trainer(tmp_path, graph, seed=42):
    import os

    import dp_worker as WK
    from kitti_tree import make_tree
    from trainer import Trainer
    root = str(tmp_path)
    if not os.path.exists(os.path.join(root, "split.txt")):
        make_tree(root, frames=8)                                   # 12 samples: 10 for training, 2 for validation
    cfg = _aug_config(os.path.join(root, "split.txt"), root, 64, 128, batch=2)
    cfg["action"].update(hipgraph=bool(graph), random_seed=seed, from_scratch=True)
    t = Trainer(cfg)
    WK.seed_models(t)
    t.set_train()
    return t


def test_trainer_nets_see_augmented_frames_and_loss_the_plain_ones(tmp_path):
    t = _trainer(tmp_path, graph=False)
    assert t.augmentation is not None and t.train_loader.augment is t.augmentation and t.validation_loader.augment is None
    t.train_loader.set_epoch(0)
    batch = next(iter(t.train_loader))
    assert "tgt_aug" in batch
    seen = 0
    for v in t.validation_loader:
        assert "tgt_aug" not in v and "augment_records" not in v
        seen += 1
    assert seen == 1
    (disps, poses), loss = t.process_batch(batch)
    with torch.no_grad():
        want_d = list(t.depth_model.forward_pair(batch["tgt_aug"], batch["ref_imgs_aug"][0]))
        want_p = t.pose_model(batch["tgt_aug"], batch["ref_imgs_aug"])
        want_l = t.criterion.forward(batch["tgt"], batch["ref_imgs"], want_d, want_p, batch["intrinsics"], None)
    torch.cuda.synchronize()
    assert torch.equal(poses.detach(), want_p)
    for a, b in zip(disps, want_d):
        assert all(torch.equal(x.detach(), y) for x, y in zip(a, b))
    assert [float(x.detach()) for x in loss] == [float(x) for x in want_l]
    with torch.no_grad():
        plain_d = list(t.depth_model.forward_pair(batch["tgt"], batch["ref_imgs"][0]))
    if not torch.equal(batch["tgt"], batch["tgt_aug"]):
        assert not torch.equal(plain_d[0][0], want_d[0][0])


def _three_steps(t):
    losses = []
    t.train_loader.set_epoch(0)
    for k, samples in enumerate(t.train_loader):
        if k == 3:
            break
        _, loss = t.train_step(samples)
        losses.append([float(l.detach()) for l in loss])
    torch.cuda.synchronize()
    return losses


def test_trainer_eager_and_hipgraph_agree_and_runs_reproduce(tmp_path):
    le = _three_steps(_trainer(tmp_path, graph=False))
    lg = _three_steps(_trainer(tmp_path, graph=True))
    le2 = _three_steps(_trainer(tmp_path, graph=False))
    assert len(le) == 3 and all(np.isfinite(l).all() for l in le)
    for a, b in zip(le, lg):
        assert all(abs(x - y) <= 1e-6 * abs(y) for x, y in zip(a, b)), (le, lg)
    assert le == le2


def test_trainer_runs_an_epoch_with_augmentation(tmp_path):
    t = _trainer(tmp_path, graph=False)
    w0 = t.model_optimizer.arena().flat.detach().clone()
    t.run_epoch()
    torch.cuda.synchronize()
    assert t.step == len(t.train_loader) > 0
    assert all(np.isfinite(float(l.detach())) for l in t.loss)
    assert not torch.equal(w0, t.model_optimizer.arena().flat.detach())
