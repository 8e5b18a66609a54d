"""GPU: the mono + stereo loss (include/mcav_depth.h: mcav_warp_loss_stereo_fwd_bwd) through losses.Losses(stereo=True), against the float64
restatement in tests/stereo_ref.py; the metric scale it exists to recover; flip equivariance; graph replay with a new baseline."""
import numpy as np
import pytest
import torch

import stereo_ref as R
from arbiter import Verdicts, perturb_tensor
from test_minreproj_gpu import check_selection, network_like

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = {"plain": {}, "min": dict(min_reprojection=True), "auto": dict(automask=True), "both": dict(min_reprojection=True, automask=True)}


def stereo_inputs(B, H, W, seed):
    tgt, refs, dt, dr, poses, K = network_like(B, H, W, seed)
    g = torch.Generator().manual_seed(seed + 2)
    # the stereo frame: tgt shifted by about a pixel plus noise (a plausible right view), baselines of both signs
    st = (0.9 * torch.roll(tgt, 1, dims=3) + 0.1 * torch.rand(tgt.shape, generator=g)).contiguous()
    b = (0.54 * torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0) * (0.9 + 0.2 * torch.rand(B, generator=g))).float()
    return tgt, refs, st, b, dt, dr, poses, K


def hip_run(tgt, refs, st, b, dt, dr, poses, K, ssim, upstream=None, **modes):
    from losses import Losses
    crit = Losses(ssim=ssim, keep_selection=True, stereo=True, **modes)
    multi = isinstance(dt, (list, tuple))
    x = [t.to(DEV).requires_grad_() for t in (dt if multi else [dt])]
    y = [t.to(DEV).requires_grad_() for t in (dr if multi else [dr])]
    z = poses.to(DEV).requires_grad_()
    out = crit.forward(tgt.to(DEV), [r.to(DEV) for r in refs], [x, y], z, K.to(DEV), None, stereo=st.to(DEV), stereo_baseline=b.to(DEV))
    if upstream is None:
        sum(out).backward()
    else:
        (upstream[0] * out[0] + upstream[1] * out[1]).backward()
    torch.cuda.synchronize()
    gx = [t.grad.cpu() for t in x]
    gy = [t.grad.cpu() for t in y]
    return ([float(out[0].detach()), float(out[1].detach())], (gx if multi else gx[0], gy if multi else gy[0], z.grad.cpu()),
            [s.cpu() for s in crit.selection])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("ssim", [False, True])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (2, 33, 65), (12, 192, 640)])
def test_parity_with_float64(B, H, W, ssim, mode):
    tgt, refs, st, b, dt, dr, poses, K = stereo_inputs(B, H, W, 7 * H + W)
    m = dict(ssim=ssim, **MODES[mode])
    loss, grads, sel = hip_run(tgt, refs, st, b, dt, dr, poses, K, **m)
    l64, g64, s64, gap64 = R.run(tgt, refs, st, b, dt, dr, poses, K, torch.float64, **m)
    _, g32, s32, _ = R.run(tgt, refs, st, b, dt, dr, poses, K, torch.float32, **m)
    for a, c in zip(loss, l64):
        assert abs(a - c) <= 5e-6 * abs(c) + 1e-12, (loss, l64)
    check_selection("%dx%dx%d %s %s" % (B, H, W, "ssim" if ssim else "l1", mode), sel, s64, gap64, s32)
    if mode in ("min", "both"):
        assert bool((sel[0][:, 0] == R.STEREO).any())              # the stereo warp wins somewhere
    envs = []
    for e in range(1 if B * H * W > 10 ** 6 else 2):
        pt = lambda t, k: perturb_tensor(t.double(), 1e-6, 1000 * (e + 1) + k)
        envs.append(R.run(pt(tgt, 3), [pt(r, 4 + i) for i, r in enumerate(refs)], pt(st, 6), b, pt(dt, 0), pt(dr, 1), pt(poses, 2), K,
                          torch.float64, **m)[1])
    v = Verdicts()
    for i, n in enumerate(("d disp_t", "d disp_r", "d poses")):
        v.add("%dx%dx%d %s %s" % (B, H, W, mode, n), grads[i], g32[i], g64[i], [env[i] for env in envs])
    v.check("test_parity_with_float64")


def _slanted_scene(B, H, W, b):
    """tgt(x, y) = S(x - fx b / D*(x, y), y), stereo = S, D* a slanted plane from 5 to 30 m.  -> tgt, stereo, D*, K (float32)."""
    K = torch.tensor([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], dtype=torch.float64).repeat(B, 1, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    ys = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    Dstar = (5.0 + 25.0 * (ys / (H - 1)) * 0.7 + 25.0 * 0.3 * (xs / (W - 1))).expand(B, 1, H, W)
    c = torch.arange(3, dtype=torch.float64).view(1, 3, 1, 1)
    S = lambda x: 0.5 + 0.2 * torch.sin(0.23 * x + 0.9 * c + 0.05 * ys) + 0.1 * torch.sin(0.071 * x * (c + 1) + 0.3 * ys)
    fx = float(K[0, 0, 0])
    tgt = S(xs - fx * b / Dstar)
    st = S(xs).expand(B, 3, H, W)
    return tgt.float().contiguous(), st.float().contiguous(), Dstar.float().contiguous(), K.float()


def _depth_loss(tgt, refs, st, b, D, poses, K, stereo):
    """loss_mam and d loss / d D through the fused kernels (depths as inputs: WL_INPUT_DEPTH)."""
    import losses as LS
    from mcav import lib as L
    flags = L.WL_INPUT_DEPTH | L.WL_NO_SMOOTH
    Dv = D.to(DEV).requires_grad_()
    args = (Dv, D.to(DEV), poses.to(DEV), tgt.to(DEV), refs[0].to(DEV), refs[1].to(DEV), K.to(DEV), flags)
    if stereo:
        l0, _ = LS._WarpLossFn.apply(*args, (0.0, 0.0, 0.0, 1.0), None, st.to(DEV), torch.full((D.shape[0],), b, device=DEV))
    else:
        l0, _ = LS._WarpLossFn.apply(*args, (1.0, 0.0, 0.0), None)
    l0.backward()
    torch.cuda.synchronize()
    return float(l0.detach()), Dv.grad.cpu()


def test_metric_scale_is_recovered():
    """The point of the feature: with a known baseline the stereo term is minimal at the TRUE metric depth.  Scanning a global factor s over
    depth s D*: the stereo loss is smallest at s = 1 (grid step 2 %), and its gradient points back towards D* on both sides.  The
    monocular term with the pose translation scaled by s is blind to s (a scale-free family: same loss to 1e-3 over the whole scan)."""
    B, H, W, b = 2, 96, 320, 0.54
    tgt, st, Dstar, K = _slanted_scene(B, H, W, b)
    scales = [0.8 + 0.02 * k for k in range(21)]
    losses = []
    for s in scales:
        l, g = _depth_loss(tgt, [st, st], st, b, s * Dstar, torch.zeros(B, 2, 6), K, True)
        losses.append(l)
        if abs(s - 1.0) > 0.05:
            inner = (slice(None), slice(None), slice(8, -8), slice(48, -8))
            mean_g = float(g[inner].mean())
            assert (mean_g > 0) == (s > 1.0), (s, mean_g)             # descent moves s D* towards D*
    best = scales[min(range(len(scales)), key=lambda k: losses[k])]
    assert abs(best - 1.0) < 0.011, (best, losses)
    # contrast: ref0 = the stereo frame seen through a POSE with translation (-b s, 0, 0) and depth s D*: the same warp for every s
    mono = []
    for s in (0.8, 1.0, 1.2):
        pose = torch.zeros(B, 2, 6)
        pose[:, 0, 3] = -b * s
        mono.append(_depth_loss(tgt, [st, st], st, b, s * Dstar, pose, K, False)[0])
    assert max(mono) - min(mono) <= 1e-3 * max(mono), mono


@pytest.mark.parametrize("ssim", [False, True])
def test_flip_equivariance(ssim):
    """Mirrored images and disparities, cx' = W - 1 - cx and a negated baseline: the same loss, mirrored disparity gradients."""
    B, H, W = 2, 48, 96
    tgt, refs, st, b, dt, dr, _, K = stereo_inputs(B, H, W, 23)
    poses = torch.zeros(B, 2, 6)                                       # (a mirrored pose is another pose; the stereo warp is the subject)
    Kf = K.clone()
    Kf[:, 0, 2] = W - 1 - K[:, 0, 2]
    fl = lambda t: t.flip(-1).contiguous()
    for mode in ("plain", "both"):
        m = dict(ssim=ssim, **MODES[mode])
        a = hip_run(tgt, refs, st, b, dt, dr, poses, K, **m)
        c = hip_run(fl(tgt), [fl(r) for r in refs], fl(st), -b, fl(dt), fl(dr), poses, Kf, **m)
        assert abs(a[0][0] - c[0][0]) <= 1e-5 * abs(a[0][0]), (a[0], c[0])
        gd = (a[1][0] - c[1][0].flip(-1)).norm() / a[1][0].norm()      # (an fp32 L1 sign may flip at a handful of near-zero residuals)
        assert float(gd) < 1e-2, float(gd)


@pytest.mark.parametrize("ssim", [False, True])
def test_non_unit_upstream_reruns_with_the_same_selection(ssim):
    tgt, refs, st, b, dt, dr, poses, K = stereo_inputs(2, 33, 65, 11)
    m = dict(ssim=ssim, min_reprojection=True, automask=True)
    _, grads, _ = hip_run(tgt, refs, st, b, dt, dr, poses, K, upstream=(0.7, 1.3), **m)
    _, g64, _, _ = R.run(tgt, refs, st, b, dt, dr, poses, K, torch.float64, upstream=(0.7, 1.3), **m)
    _, g32, _, _ = R.run(tgt, refs, st, b, dt, dr, poses, K, torch.float32, upstream=(0.7, 1.3), **m)
    v = Verdicts()
    for i, n in enumerate(("d disp_t", "d disp_r", "d poses")):
        v.add("upstream (0.7, 1.3) " + n, grads[i], g32[i], g64[i])
    v.check("test_non_unit_upstream_reruns_with_the_same_selection")


def test_two_runs_are_bit_identical():
    tgt, refs, st, b, dt, dr, poses, K = stereo_inputs(4, 96, 160, 19)
    for ssim in (False, True):
        x = hip_run(tgt, refs, st, b, dt, dr, poses, K, ssim=ssim, min_reprojection=True, automask=True)
        y = hip_run(tgt, refs, st, b, dt, dr, poses, K, ssim=ssim, min_reprojection=True, automask=True)
        assert x[0] == y[0]
        for p, q in zip(x[1], y[1]):
            assert torch.equal(p, q)
        assert torch.equal(x[2][0], y[2][0])


def test_entry_rejects_bad_arguments():
    from mcav import lib as L
    tgt, refs, st, b, dt, dr, poses, K = (t.to(DEV) if torch.is_tensor(t) else [r.to(DEV) for r in t]
                                          for t in stereo_inputs(2, 9, 13, 3))
    h = L.lib()
    B, _, H, W = tgt.shape
    ws = L.workspace(h.mcav_warp_loss_workspace_bytes(B, H, W), tgt.device, "stereo_test", zero=True)
    o = [torch.zeros(2, device=DEV), torch.zeros_like(dt), torch.zeros_like(dr), torch.zeros_like(poses)]
    sel = torch.zeros((B, 2, H, W), dtype=torch.uint8, device=DEV)
    args = [L.ptr(tgt), L.ptr(refs[0]), L.ptr(refs[1]), L.ptr(dt), L.ptr(dr), L.ptr(poses), L.ptr(K), B, H, W, L.WL_K_F64, None, None,
            *[L.ptr(t) for t in o], L.ptr(ws), ws.numel(), L.stream()]
    ok = args + [L.ptr(sel), sel.numel(), L.ptr(st), L.ptr(b)]
    assert h.mcav_warp_loss_stereo_fwd_bwd(*ok) == 0
    bad = list(ok)
    bad[10] = L.WL_K_F64 | 128
    assert h.mcav_warp_loss_stereo_fwd_bwd(*bad) == -1
    assert h.mcav_warp_loss_stereo_fwd_bwd(*(args + [L.ptr(sel), sel.numel(), L.ptr(None), L.ptr(b)])) == -1
    assert h.mcav_warp_loss_stereo_fwd_bwd(*(args + [L.ptr(sel), sel.numel(), L.ptr(st), L.ptr(None)])) == -1
    assert h.mcav_warp_loss_stereo_fwd_bwd(*(args + [L.ptr(sel), sel.numel() - 1, L.ptr(st), L.ptr(b)])) == -2
    small = list(ok)
    small[18] = 16
    assert h.mcav_warp_loss_stereo_fwd_bwd(*small) == -2
    torch.cuda.synchronize()


@pytest.mark.parametrize("ssim", [False, True])
def test_multiscale_dispnets(ssim):
    from models.depth.disp_net import DispNetS
    from oracle.step import synthetic_batch
    B, H, W = 2, 64, 128
    s = synthetic_batch(B, H, W, seed=31)
    torch.manual_seed(5)
    net = DispNetS().to(DEV).train()
    with torch.no_grad():
        dts = [d.detach().cpu() for d in net(s["tgt"].to(DEV))]
        drs = [d.detach().cpu() for d in net(s["ref_imgs"][0].to(DEV))]
    poses = 0.01 * torch.randn(B, 2, 6, generator=torch.Generator().manual_seed(6))
    st = torch.roll(s["tgt"], 2, dims=3).contiguous()
    b = torch.tensor([0.54, -0.54])
    m = dict(ssim=ssim, min_reprojection=True, automask=True)
    loss, grads, sel = hip_run(s["tgt"], s["ref_imgs"], st, b, dts, drs, poses, s["intrinsics"], **m)
    l64, g64, s64, gap64 = R.run(s["tgt"], s["ref_imgs"], st, b, dts, drs, poses, s["intrinsics"], torch.float64, **m)
    _, g32, s32, _ = R.run(s["tgt"], s["ref_imgs"], st, b, dts, drs, poses, s["intrinsics"], torch.float32, **m)
    assert len(sel) == 4
    for x, y in zip(loss, l64):
        assert abs(x - y) <= 2e-5 * abs(y)
    check_selection("DispNetS stereo", sel, s64, gap64, s32)
    envs = []
    for e in range(2):
        pt = lambda t, k: perturb_tensor(t.double(), 1e-6, 1000 * (e + 1) + k)
        envs.append(R.run(pt(s["tgt"], 3), [pt(r, 4 + i) for i, r in enumerate(s["ref_imgs"])], pt(st, 7), b,
                          [pt(d, 10 + i) for i, d in enumerate(dts)], [pt(d, 20 + i) for i, d in enumerate(drs)], pt(poses, 2),
                          s["intrinsics"], torch.float64, **m)[1])
    v = Verdicts()
    for k in range(4):
        v.add("scale %d d disp_t" % k, grads[0][k], g32[0][k], g64[0][k], [env[0][k] for env in envs])
        v.add("scale %d d disp_r" % k, grads[1][k], g32[1][k], g64[1][k], [env[1][k] for env in envs])
    v.add("d poses", grads[2], g32[2], g64[2], [env[2] for env in envs])
    v.check("test_multiscale_dispnets stereo")


def test_graph_replay_honours_a_new_baseline():
    """The loss and its backward captured in a hipGraph; replayed after stereo_baseline is overwritten in place (a flipped batch): the same
    losses and gradients as an eager run with the new baseline."""
    from losses import Losses
    tgt, refs, st, b, dt, dr, poses, K = stereo_inputs(2, 48, 96, 29)
    crit = Losses(stereo=True, min_reprojection=True, automask=True)
    T = [t.to(DEV) for t in (tgt, refs[0], refs[1], st, K)]
    bd = b.to(DEV)
    x, y, z = dt.to(DEV).requires_grad_(), dr.to(DEV).requires_grad_(), poses.to(DEV).requires_grad_()

    def step():
        for p in (x, y, z):
            p.grad = None
        out = crit.forward(T[0], [T[1], T[2]], [[x], [y]], z, T[4], None, stereo=T[3], stereo_baseline=bd)
        sum(out).backward()
        return torch.stack([o.detach() for o in out])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g = step()
        grads_g = [x.grad, y.grad, z.grad]
    bd.copy_(-bd * 0.9)
    g.replay()
    torch.cuda.synchronize()
    got = (out_g.cpu(), [t.detach().cpu().clone() for t in grads_g])
    want = hip_run(tgt, refs, st, (-b * 0.9), dt, dr, poses, K, ssim=False, min_reprojection=True, automask=True)
    assert torch.allclose(got[0], torch.tensor(want[0]), rtol=1e-6, atol=0)
    for a, c in zip(got[1], want[1]):
        assert torch.equal(a, c) or float((a - c).abs().max()) <= 1e-6 * float(c.abs().max())
    first = hip_run(tgt, refs, st, b, dt, dr, poses, K, ssim=False, min_reprojection=True, automask=True)
    assert first[0][0] != want[0][0]                                     # (the baseline does change the loss)


# ---------------------------------------------------------------------------------------------- loader and trainer (loss.stereo)
def test_prefetch_loader_stereo_frames(tmp_path):
    """'stereo' is the plain transform of the target's image_03 twin (never jittered), mirrored where the augmentation flips, and
    'stereo_baseline' the drive's baseline, negated there."""
    from PIL import Image
    from dataloaders import AUG_FLIP, Augmentation, PrefetchLoader, UnSupKittiDataset, find_calib_dir, raw_collate
    from kitti_stereo_tree import baseline_by_formula, make_stereo_tree, stereo_config
    from oracle import preprocess as op
    import os
    split, rows, twins = make_stereo_tree(str(tmp_path), frames=6)
    H, W = 24, 80
    ds = UnSupKittiDataset(stereo_config(split, str(tmp_path), H, W))
    order = list(range(len(ds)))
    flips = 0
    for aug in (None, Augmentation(p_color=0.7, p_flip=0.5, seed=11)):
        ld = PrefetchLoader(torch.utils.data.DataLoader(ds, batch_size=2, sampler=order, collate_fn=raw_collate, num_workers=0), H, W, DEV,
                            augment=aug)
        ld.set_epoch(3)
        for bi, batch in enumerate(ld):
            assert all(tuple(x.shape) == (2, 3, H, W) for x in [batch["tgt"], batch["stereo"]] + batch["ref_imgs"])
            assert batch["stereo_baseline"].is_cuda
            assert batch["stereo_baseline"].dtype == torch.float32
            for j in range(2):
                r = rows[order[2 * bi + j]]
                want = op.load_transform(np.asarray(Image.open(twins[r[0]])), H, W)
                b = baseline_by_formula(os.path.basename(os.path.normpath(find_calib_dir(r[0]))))
                flip = aug is not None and bool(batch["augment_records"][j]["flags"] & AUG_FLIP)
                flips += flip
                got = batch["stereo"][j].cpu().numpy()
                assert np.array_equal(got, want[..., ::-1] if flip else want)
                assert abs(float(batch["stereo_baseline"][j]) - (-b if flip else b)) < 1e-6
    assert flips > 0


def _stereo_trainer(split, root, graph):
    import dp_worker as WK
    from kitti_stereo_tree import stereo_config
    from trainer import Trainer
    cfg = stereo_config(split, root, 64, 128, batch=2)
    cfg["action"].update(hipgraph=bool(graph), from_scratch=True)
    t = Trainer(cfg)
    assert t.criterion.stereo
    WK.seed_models(t)
    t.set_train()
    return t


def test_trainer_stereo_eager_and_hipgraph(tmp_path):
    """trainer config `loss: {stereo: true}` on a KITTI-shaped tree: the same batches issued eagerly and replayed under action.hipgraph give
    the same losses and parameters; the baselines of the batches differ in sign (flips), which the replay takes as graph inputs."""
    from kitti_stereo_tree import make_stereo_tree
    split, _, _ = make_stereo_tree(str(tmp_path), frames=8)
    t0 = _stereo_trainer(split, str(tmp_path), 0)
    batches = []
    for batch in t0.train_loader:
        batches.append(batch)
        if len(batches) == 3:
            break
    assert all("stereo" in b and "stereo_baseline" in b for b in batches)
    batches[1]["stereo_baseline"] = -batches[1]["stereo_baseline"]
    batches[1]["stereo"] = batches[1]["stereo"].flip(-1).contiguous()
    results = []
    for t in (t0, _stereo_trainer(split, str(tmp_path), 1)):
        losses = []
        for b in batches:
            _, loss = t.train_step(b)
            losses.append([float(x.detach()) for x in loss])
        torch.cuda.synchronize()
        results.append((losses, t.model_optimizer.arena().flat.detach().clone()))
    (le, fe), (lg, fg) = results
    for a, c in zip(le, lg):
        assert all(abs(x - y) <= 1e-6 * abs(y) for x, y in zip(a, c)), (le, lg)
    assert all(np.isfinite(x) for l in le for x in l)
    assert float((fe - fg).abs().max()) <= 1e-6 * float(fe.abs().max())


def test_trainer_stereo_epoch(tmp_path):
    from kitti_stereo_tree import make_stereo_tree, stereo_config
    from trainer import Trainer
    split, _, _ = make_stereo_tree(str(tmp_path), frames=8)
    cfg = stereo_config(split, str(tmp_path), 64, 128, batch=2)
    cfg["action"]["num_workers"] = 2
    cfg["datasets"]["augmentation"].update(flip=0.5)
    t = Trainer(cfg)
    t.train()
    assert t.step >= 3 and torch.isfinite(sum(t.loss)).item()
