"""GPU: the masked loss modes (MCAV_WL_MIN_REPROJ / MCAV_WL_AUTOMASK) of the fused kernels, through the C ABI via losses.Losses, against the
float64 / float32 CPU restatement in tests/minreproj_ref.py."""
import ctypes

import pytest
import torch

import minreproj_ref as R
from arbiter import Verdicts, perturb_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = {"min": dict(min_reprojection=True), "auto": dict(automask=True), "both": dict(min_reprojection=True, automask=True)}


def network_like(B, H, W, seed):
    """tools/loss_bench.py's inputs: synthetic images, smooth disparities around 0.5, small poses."""
    from oracle.step import synthetic_batch
    s = synthetic_batch(B, H, W, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)

    def smooth_disp():
        z = torch.randn(B, 1, H // 8 + 2, W // 8 + 2, generator=g)
        return torch.sigmoid(0.3 * torch.nn.functional.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)).contiguous()
    dt, dr = smooth_disp(), smooth_disp()
    return s["tgt"], s["ref_imgs"], dt, dr, 0.01 * torch.randn(B, 2, 6, generator=g), s["intrinsics"]


def hip_run(tgt, refs, dt, dr, poses, K, ssim, upstream=None, **modes):
    from losses import Losses
    crit = Losses(ssim=ssim, keep_selection=True, **modes)
    multi = isinstance(dt, (list, tuple))
    x = [t.to(DEV).requires_grad_() for t in (dt if multi else [dt])]
    y = [t.to(DEV).requires_grad_() for t in (dr if multi else [dr])]
    z = poses.to(DEV).requires_grad_()
    out = crit.forward(tgt.to(DEV), [r.to(DEV) for r in refs], [x, y], z, K.to(DEV), None)
    if upstream is None:
        sum(out).backward()
    else:
        (upstream[0] * out[0] + upstream[1] * out[1]).backward()
    torch.cuda.synchronize()
    gx = [t.grad.cpu() for t in x]
    gy = [t.grad.cpu() for t in y]
    return ([float(out[0].detach()), float(out[1].detach())], (gx if multi else gx[0], gy if multi else gy[0], z.grad.cpu()),
            [s.cpu() for s in crit.selection])


def check_selection(name, got, want64, gaps64, want32):
    """Equal to the float64 selection except at near ties, or where the CPU float32 evaluation takes the same side as the kernel (a
    decision at rounding level of ANY fp32 evaluation).  Near tie: the two smallest float64 candidates within 2e-4 relative -- the value
    margin tests/test_loss_gpu.py allows an fp32 evaluation of the warp (the kernel's lean projection and the reference's fp32 chain both
    put sampling positions up to 1e-4 px from float64).  Measured at 12 x 192 x 640: 12 .. 41 of 2.9 M pixels differ, gaps <= 7.3e-5."""
    for s, (g, w, gap, w32) in enumerate(zip(got, want64, gaps64, want32)):
        g = g.long()
        diff = int((g != w).sum())
        bad = (g != w) & ~(gap <= 2e-4) & (g != w32)
        assert not bool(bad.any()), "%s scale %d: %d pixels selected differently from float64 without a tie (of %d that differ; gaps %s)" % (
            name, s, int(bad.sum()), diff, gap[bad][:5].tolist())
        assert diff <= max(16, 2e-5 * g.numel()), "%s scale %d: %d pixels selected differently from float64" % (name, s, diff)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("ssim", [False, True])
@pytest.mark.parametrize("B,H,W", [(1, 3, 3), (2, 5, 7), (2, 33, 65), (1, 31, 34), (12, 192, 640)])
def test_parity_with_float64(B, H, W, ssim, mode):
    tgt, refs, dt, dr, poses, K = network_like(B, H, W, 7 * H + W)
    m = dict(ssim=ssim, **MODES[mode])
    loss, grads, sel = hip_run(tgt, refs, dt, dr, poses, K, **m)
    l64, g64, s64, gap64 = R.run(tgt, refs, dt, dr, poses, K, torch.float64, **m)
    _, g32, s32, _ = R.run(tgt, refs, dt, dr, poses, K, torch.float32, **m)
    for a, b in zip(loss, l64):
        assert abs(a - b) <= 5e-6 * abs(b) + 1e-12, (loss, l64)
    check_selection("%dx%dx%d %s %s" % (B, H, W, "ssim" if ssim else "l1", mode), sel, s64, gap64, s32)
    envs = []
    for e in range(1 if B * H * W > 10 ** 6 else 2):
        pt = lambda t, k: perturb_tensor(t.double(), 1e-6, 1000 * (e + 1) + k)
        envs.append(R.run(pt(tgt, 3), [pt(r, 4 + i) for i, r in enumerate(refs)], pt(dt, 0), pt(dr, 1), pt(poses, 2), K, torch.float64, **m)[1])
    v = Verdicts()
    for i, n in enumerate(("d disp_t", "d disp_r", "d poses")):
        v.add("%dx%dx%d %s %s" % (B, H, W, mode, n), grads[i], g32[i], g64[i], [env[i] for env in envs])
    v.check("test_parity_with_float64")


@pytest.mark.parametrize("ssim", [False, True])
def test_non_unit_upstream_reruns_with_the_same_selection(ssim):
    tgt, refs, dt, dr, poses, K = network_like(2, 33, 65, 11)
    m = dict(ssim=ssim, min_reprojection=True, automask=True)
    _, grads, _ = hip_run(tgt, refs, dt, dr, poses, K, upstream=(0.7, 1.3), **m)
    _, g64, _, _ = R.run(tgt, refs, dt, dr, poses, K, torch.float64, upstream=(0.7, 1.3), **m)
    _, g32, _, _ = R.run(tgt, refs, dt, dr, poses, K, torch.float32, upstream=(0.7, 1.3), **m)
    v = Verdicts()
    for i, n in enumerate(("d disp_t", "d disp_r", "d poses")):
        v.add("upstream (0.7, 1.3) " + n, grads[i], g32[i], g64[i])
    v.check("test_non_unit_upstream_reruns_with_the_same_selection")


@pytest.mark.parametrize("ssim", [False, True])
def test_static_scene_is_all_identity(ssim):
    """ref0 = ref1 = tgt, zero poses: every pixel's identity error is 0, so every selection is identity, the loss is 0 and the photometric
    part of every gradient is exactly zero -- what is left is the smoothness gradient alone."""
    tgt, _, dt, dr, _, K = network_like(2, 33, 65, 13)
    poses = torch.zeros(2, 2, 6)
    for mode in ("auto", "both"):
        m = dict(ssim=ssim, **MODES[mode])
        loss, grads, sel = hip_run(tgt, [tgt.clone(), tgt.clone()], dt, dr, poses, K, **m)
        assert loss[0] == 0.0
        assert bool((sel[0] == R.IDENTITY).all())
        _, smooth, _ = hip_run(tgt, [tgt.clone(), tgt.clone()], dt, dr, poses, K, upstream=(0.0, 1.0), **m)
        assert torch.equal(grads[0], smooth[0])
        assert float(grads[1].abs().max()) == 0.0 and float(grads[2].abs().max()) == 0.0


@pytest.mark.parametrize("ssim", [False, True])
def test_masked_entry_with_modes_off_is_the_plain_entry(ssim):
    """mcav_warp_loss_masked_fwd_bwd without the new flags: bit-identical to mcav_warp_loss_fwd_bwd (and a zero selection)."""
    from mcav import lib as L
    tgt, refs, dt, dr, poses, K = (t.to(DEV) if torch.is_tensor(t) else [r.to(DEV) for r in t] for t in network_like(2, 33, 65, 17))
    h = L.lib()
    B, _, H, W = tgt.shape
    flags = L.WL_K_F64 | (L.WL_SSIM if ssim else 0)
    outs = []
    for masked in (False, True):
        ws = L.workspace(h.mcav_warp_loss_workspace_bytes(B, H, W), tgt.device, "minreproj_test", zero=True)
        o = [torch.full((2,), 7.0, device=DEV), torch.full_like(dt, 7.0), torch.full_like(dr, 7.0), torch.full_like(poses, 7.0)]
        sel = torch.full((B, 2, H, W), 9, dtype=torch.uint8, device=DEV)
        tw = (ctypes.c_float * 3)(0.25, 0.25, 0.5)
        args = [L.ptr(tgt), L.ptr(refs[0]), L.ptr(refs[1]), L.ptr(dt), L.ptr(dr), L.ptr(poses), L.ptr(K), B, H, W, flags, None, tw,
                *[L.ptr(t) for t in o], L.ptr(ws), ws.numel(), L.stream()]
        if masked:
            L.check(h.mcav_warp_loss_masked_fwd_bwd(*args, L.ptr(sel), sel.numel()), "masked")
            unknown = list(args)
            unknown[10] = flags | 128
            assert h.mcav_warp_loss_masked_fwd_bwd(*unknown, L.ptr(sel), sel.numel()) == -1          # MCAV_E_INVALID
            assert h.mcav_warp_loss_masked_fwd_bwd(*args, L.ptr(sel), sel.numel() - 1) == -2        # MCAV_E_WORKSPACE
        else:
            L.check(h.mcav_warp_loss_fwd_bwd(*args), "plain")
        torch.cuda.synchronize()
        outs.append([t.clone() for t in o])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert int(sel.sum()) == 0


def test_two_runs_are_bit_identical():
    tgt, refs, dt, dr, poses, K = network_like(4, 96, 160, 19)
    for ssim in (False, True):
        a = hip_run(tgt, refs, dt, dr, poses, K, ssim=ssim, min_reprojection=True, automask=True)
        b = hip_run(tgt, refs, dt, dr, poses, K, ssim=ssim, min_reprojection=True, automask=True)
        assert a[0] == b[0]
        for x, y in zip(a[1], b[1]):
            assert torch.equal(x, y)
        assert torch.equal(a[2][0], b[2][0])


@pytest.mark.parametrize("ssim", [False, True])
def test_multiscale_dispnets(ssim):
    """DispNetS's four disparity scales: every coarser depth resized to the image size, the masked modes per scale."""
    from models.depth.disp_net import DispNetS
    from oracle.step import synthetic_batch
    B, H, W = 2, 64, 128
    s = synthetic_batch(B, H, W, seed=31)
    torch.manual_seed(5)
    net = DispNetS().to(DEV).train()
    with torch.no_grad():
        dts = [d.detach().cpu() for d in net(s["tgt"].to(DEV))]
        drs = [d.detach().cpu() for d in net(s["ref_imgs"][0].to(DEV))]
    assert [d.shape[-1] for d in dts] == [W, W // 2, W // 4, W // 8]
    poses = 0.01 * torch.randn(B, 2, 6, generator=torch.Generator().manual_seed(6))
    m = dict(ssim=ssim, min_reprojection=True, automask=True)
    loss, grads, sel = hip_run(s["tgt"], s["ref_imgs"], dts, drs, poses, s["intrinsics"], **m)
    l64, g64, s64, gap64 = R.run(s["tgt"], s["ref_imgs"], dts, drs, poses, s["intrinsics"], torch.float64, **m)
    _, g32, s32, _ = R.run(s["tgt"], s["ref_imgs"], dts, drs, poses, s["intrinsics"], torch.float32, **m)
    # the envelope: a selection tie of a full-resolution pixel moves the four elements of a coarse map it reaches through the resize
    envs = []
    for e in range(2):
        pt = lambda t, k: perturb_tensor(t.double(), 1e-6, 1000 * (e + 1) + k)
        envs.append(R.run(pt(s["tgt"], 3), [pt(r, 4 + i) for i, r in enumerate(s["ref_imgs"])], [pt(d, 10 + i) for i, d in enumerate(dts)],
                          [pt(d, 20 + i) for i, d in enumerate(drs)], pt(poses, 2), s["intrinsics"], torch.float64, **m)[1])
    assert len(sel) == 4
    for a, b in zip(loss, l64):
        assert abs(a - b) <= 2e-5 * abs(b)
    check_selection("DispNetS", sel, s64, gap64, s32)
    v = Verdicts()
    for k in range(4):
        v.add("scale %d d disp_t" % k, grads[0][k], g32[0][k], g64[0][k], [env[0][k] for env in envs])
        v.add("scale %d d disp_r" % k, grads[1][k], g32[1][k], g64[1][k], [env[1][k] for env in envs])
    v.add("d poses", grads[2], g32[2], g64[2], [env[2] for env in envs])
    v.check("test_multiscale_dispnets")


def test_trainer_config_eager_and_hipgraph():
    """trainer config `loss: {min_reprojection: true, automask: true}`: synthetic steps issued eagerly and replayed under action.hipgraph
    (StepGraphs) give the same losses and parameters."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dp_worker as WK
    from oracle.step import synthetic_batch
    from trainer import Trainer
    results = []
    for graph in (0, 1):
        cfg = WK.build_config(64, 128, 2, graph)
        cfg["loss"] = dict(min_reprojection=True, automask=True)
        t = Trainer(cfg)
        assert t.criterion.min_reprojection and t.criterion.automask and not t.criterion.ssim
        WK.seed_models(t)
        t.set_train()
        losses = []
        for k in range(3):
            _, loss = t.train_step(synthetic_batch(2, 64, 128, seed=90 + k))
            losses.append([float(l.detach()) for l in loss])
        torch.cuda.synchronize()
        results.append((losses, t.model_optimizer.arena().flat.detach().clone()))
    (le, fe), (lg, fg) = results
    for a, b in zip(le, lg):
        assert all(abs(x - y) <= 1e-6 * abs(y) for x, y in zip(a, b)), (le, lg)
    assert float((fe - fg).abs().max()) <= 1e-6 * float(fe.abs().max())
