"""GPU: the edge-aware smoothness on mean-normalised disparity (mcav_edge_smooth_fwd / _bwd) through losses.Losses, against the float64 / float32
CPU restatement in tests/edge_smooth_ref.py, and its combination with the fused photometric kernel."""
import pytest
import torch

import edge_smooth_ref as R
from arbiter import Verdicts, perturb_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"


def image_and_disp(B, h, w, seed, f=1):
    """A synthetic (box low-passed) image and a smooth disparity around 0.5, as a depth network gives it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, h * f, w * f, generator=g)
    if h * f >= 2 and w * f >= 2:
        x = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), 3, 1)
    z = torch.randn(B, 1, h // 8 + 2, w // 8 + 2, generator=g)
    d = torch.sigmoid(0.3 * torch.nn.functional.interpolate(z, size=(h, w), mode="bilinear", align_corners=False))
    return x.contiguous(), d.contiguous()


def hip_edge(disp, img, weight=1e-3, upstream=1.0):
    """Losses.edge_aware_smooth_loss on the device -> (loss, [grad per scale] or grad)."""
    from losses import Losses
    crit = Losses(edge_aware_smoothness=True, edge_smoothness_weight=weight)
    multi = isinstance(disp, (list, tuple))
    x = [d.to(DEV).requires_grad_() for d in (disp if multi else [disp])]
    E = crit.edge_aware_smooth_loss(x if multi else x[0], img.to(DEV))
    (upstream * E).backward()
    torch.cuda.synchronize()
    g = [t.grad.cpu() for t in x]
    return float(E.detach()), (g if multi else g[0])


def envelopes(disp, img, n, **kw):
    out = []
    for e in range(n):
        pd = [perturb_tensor(d.double(), 1e-6, 1000 * (e + 1) + i) for i, d in enumerate(disp)] if isinstance(disp, list) else \
            perturb_tensor(disp.double(), 1e-6, 1000 * (e + 1))
        out.append(R.run(pd, perturb_tensor(img.double(), 1e-6, 1000 * (e + 1) + 99), **kw)[1])
    return out


@pytest.mark.parametrize("B,h,w", [(1, 1, 5), (2, 5, 1), (2, 5, 7), (1, 31, 34), (2, 33, 65), (12, 192, 640)])
def test_parity_with_float64(B, h, w):
    img, d = image_and_disp(B, h, w, 7 * h + w)
    loss, grad = hip_edge(d, img)
    l64, g64 = R.run(d, img)
    _, g32 = R.run(d, img, torch.float32)
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    v = Verdicts()
    v.add("%dx%dx%d d disp" % (B, h, w), grad, g32, g64, envelopes(d, img, 1 if B * h * w > 10 ** 6 else 2))
    v.check("test_parity_with_float64")


@pytest.mark.parametrize("f", [2, 4, 8])
def test_parity_of_a_coarse_scale(f):
    """A coarse map against the full-resolution image: the image taps are f x f box averages."""
    img, d = image_and_disp(2, 64 // f, 128 // f, 40 + f, f)
    loss, grad = hip_edge(d, img)
    l64, g64 = R.run(d, img)
    _, g32 = R.run(d, img, torch.float32)
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    v = Verdicts()
    v.add("f=%d d disp" % f, grad, g32, g64, envelopes(d, img, 2))
    v.check("test_parity_of_a_coarse_scale")


def test_invariance_on_the_device():
    img, d = image_and_disp(4, 96, 160, 3)
    E1, g = hip_edge(d, img, weight=1.0)
    E2, _ = hip_edge(0.5 * d, img, weight=1.0)
    assert abs(E2 - E1) <= 1e-5 * E1, (E1, E2)
    for b in range(4):
        s = float((g[b].double() * d[b].double()).sum())
        assert abs(s) <= 1e-4 * float((g[b].double().abs() * d[b].double().abs()).sum()), (b, s)
    E0, g0 = hip_edge(torch.full_like(d, 0.42), img, weight=1.0)
    assert E0 == 0.0 and float(g0.abs().max()) == 0.0


def test_wrong_shape_raises_without_a_launch():
    from mcav import lib as L
    from mcav import nn as N
    from losses import Losses
    img, _ = image_and_disp(2, 32, 64, 5)
    crit = Losses(edge_aware_smoothness=True)
    N.kernel_timer_begin()
    for shape in ((2, 1, 10, 20), (2, 1, 16, 16), (2, 1, 32, 48)):
        with pytest.raises(L.MCAVError):
            crit.edge_aware_smooth_loss(torch.rand(shape, device=DEV), img.to(DEV))
    torch.cuda.synchronize()
    assert N.kernel_timer_end() == []


def network_like(B, H, W, seed):
    from oracle.step import synthetic_batch
    s = synthetic_batch(B, H, W, seed=seed)
    _, dt = image_and_disp(B, H, W, seed + 1)
    _, dr = image_and_disp(B, H, W, seed + 2)
    return s["tgt"], s["ref_imgs"], dt, dr, 0.01 * torch.randn(B, 2, 6, generator=torch.Generator().manual_seed(seed)), s["intrinsics"]


def full_run(tgt, refs, dt, dr, poses, K, upstream=None, **opts):
    from losses import Losses
    crit = Losses(**opts)
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
    gy = [t.grad.cpu() if t.grad is not None else torch.zeros_like(t).cpu() for t in y]
    return [out[0].detach().cpu(), out[1].detach().cpu()], (gx if multi else gx[0], gy if multi else gy[0], z.grad.cpu())


MODES = {"plain": {}, "ssim": dict(ssim=True), "min+auto": dict(min_reprojection=True, automask=True)}


@pytest.mark.parametrize("mode", list(MODES))
def test_loss_mam_is_untouched(mode):
    """loss_mam, d disp_r and d poses are those of the same call without the option, bit for bit; loss_smooth is the standalone term."""
    tgt, refs, dt, dr, poses, K = network_like(2, 33, 65, 21)
    off, g_off = full_run(tgt, refs, dt, dr, poses, K, **MODES[mode])
    on, g_on = full_run(tgt, refs, dt, dr, poses, K, edge_aware_smoothness=True, **MODES[mode])
    assert torch.equal(off[0], on[0]), (float(off[0]), float(on[0]))
    assert torch.equal(g_off[1], g_on[1]) and torch.equal(g_off[2], g_on[2])
    E, _ = hip_edge(dt, tgt)
    assert float(on[1]) == E


def test_single_scale_is_the_fused_kernel_plus_the_term():
    """12 x 192 x 640: d disp_t of Losses(edge_aware_smoothness=True) is the NO_SMOOTH fused kernel's gradient plus the edge term's, bit for bit,
    and loss_smooth is the float64 restatement's within 1e-5."""
    import losses as LS
    from mcav import lib as L
    tgt, refs, dt, dr, poses, K = network_like(12, 192, 640, 23)
    loss, grads = full_run(tgt, refs, dt, dr, poses, K, edge_aware_smoothness=True)
    x, y, z = dt.to(DEV).requires_grad_(), dr.to(DEV).requires_grad_(), poses.to(DEV).requires_grad_()
    l0, l1 = LS._WarpLossFn.apply(x, y, z, tgt.to(DEV), refs[0].to(DEV), refs[1].to(DEV), K.to(DEV), L.WL_NO_SMOOTH, (0.25, 0.25, 0.5), None)
    (l0 + l1).backward()
    assert float(l1.detach()) == 0.0 and torch.equal(l0.detach().cpu(), loss[0])
    _, g_edge = hip_edge(dt, tgt)
    assert torch.equal(grads[0], x.grad.cpu() + g_edge)
    assert torch.equal(grads[2], z.grad.cpu())
    l64, _ = R.run(dt, tgt)
    assert abs(float(loss[1]) - l64) <= 1e-5 * l64


def test_upstream_weights():
    """(a l0 + c l1).backward(): c times the unit-upstream smoothness gradient plus a times the photometric one."""
    tgt, refs, dt, dr, poses, K = network_like(2, 33, 65, 25)
    a, c = 0.7, 1.9
    opts = dict(edge_aware_smoothness=True, min_reprojection=True, automask=True)
    _, g_ac = full_run(tgt, refs, dt, dr, poses, K, upstream=(a, c), **opts)
    _, g_ph = full_run(tgt, refs, dt, dr, poses, K, upstream=(1.0, 0.0), **opts)
    _, g_sm = full_run(tgt, refs, dt, dr, poses, K, upstream=(0.0, 1.0), **opts)
    _, g_unit = hip_edge(dt, tgt)
    assert torch.equal(g_sm[0], g_unit)
    want = a * g_ph[0].double() + c * g_sm[0].double()
    assert float((g_ac[0].double() - want).norm() / want.norm()) <= 1e-6
    for i in (1, 2):                    # the fused kernel's re-run folds a into its per-pixel weights: fp32 rounding apart
        want = a * g_ph[i].double()
        assert float((g_ac[i].double() - want).norm() / want.norm()) <= 1e-5
    _, g64 = R.full_losses(tgt, refs, dt, dr, poses, K, upstream=(a, c), min_reprojection=True, automask=True)
    assert float((g_ac[0].double() - g64[0]).norm() / g64[0].norm()) <= 1e-3


def test_multiscale_dispnets():
    """DispNetS's four disparity scales, B=2, 64x128: box-averaged images, weights 1e-3 / 4 * 2^-s, a gradient for every scale's map."""
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
    opts = dict(min_reprojection=True, automask=True)
    off, _ = full_run(s["tgt"], s["ref_imgs"], dts, drs, poses, s["intrinsics"], **opts)
    on, grads = full_run(s["tgt"], s["ref_imgs"], dts, drs, poses, s["intrinsics"], upstream=(0.0, 1.0), edge_aware_smoothness=True, **opts)
    assert torch.equal(off[0], on[0])
    l64, g64 = R.run(dts, s["tgt"])
    _, g32 = R.run(dts, s["tgt"], torch.float32)
    assert abs(float(on[1]) - l64) <= 1e-5 * l64, (float(on[1]), l64)
    want = 1e-3 / 4 * sum(2.0 ** -k * R.run(d, s["tgt"], weight=1.0)[0] for k, d in enumerate(dts))
    assert abs(l64 - want) <= 1e-12 * want
    envs = envelopes(dts, s["tgt"], 2)
    v = Verdicts()
    for k in range(4):
        assert float(grads[0][k].abs().max()) > 0
        v.add("scale %d d disp_t" % k, grads[0][k], g32[k], g64[k], [e[k] for e in envs])
    v.check("test_multiscale_dispnets")


def test_two_runs_are_bit_identical():
    tgt, refs, dt, dr, poses, K = network_like(4, 96, 160, 19)
    opts = dict(edge_aware_smoothness=True, min_reprojection=True, automask=True)
    a = full_run(tgt, refs, dt, dr, poses, K, **opts)
    b = full_run(tgt, refs, dt, dr, poses, K, **opts)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    img, ds = image_and_disp(3, 64, 128, 9)
    coarse = [ds] + [torch.nn.functional.avg_pool2d(ds, 2 ** k) for k in (1, 2, 3)]
    (la, ga), (lb, gb) = hip_edge(coarse, img), hip_edge(coarse, img)
    assert la == lb and all(torch.equal(x, y) for x, y in zip(ga, gb))


def test_trainer_config_eager_and_hipgraph():
    """trainer config `loss: {edge_aware_smoothness: true, min_reprojection: true, automask: true}`: synthetic steps issued eagerly and
    replayed under action.hipgraph (StepGraphs) give the same losses and parameters."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dp_worker as WK
    from oracle.step import synthetic_batch
    from trainer import Trainer
    results = []
    for graph in (0, 1):
        cfg = WK.build_config(64, 128, 2, graph)
        cfg["loss"] = dict(edge_aware_smoothness=True, min_reprojection=True, automask=True)
        t = Trainer(cfg)
        assert t.criterion.edge_aware_smoothness and t.criterion.edge_smoothness_weight == 1e-3 and t.criterion.min_reprojection
        WK.seed_models(t)
        t.set_train()
        losses = []
        for k in range(3):
            _, loss = t.train_step(synthetic_batch(2, 64, 128, seed=90 + k))
            losses.append([float(l.detach()) for l in loss])
        torch.cuda.synchronize()
        results.append((losses, t.model_optimizer.arena().flat.detach().clone()))
    (le, fe), (lg, fg) = results
    assert all(l[1] > 0 for l in le)
    for a, b in zip(le, lg):
        assert all(abs(x - y) <= 1e-6 * abs(y) for x, y in zip(a, b)), (le, lg)
    assert float((fe - fg).abs().max()) <= 1e-6 * float(fe.abs().max())
