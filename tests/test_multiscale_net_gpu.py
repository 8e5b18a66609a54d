"""GPU: the multi-scale DispResNet (scales=4), the fused depth pyramid inside the loss, and both through the trainer.  All at
B = 2, 64 x 128: the smallest size the decoder's reflection padding admits (scale 3's head sees 8 x 16, level 4 of the decoder 2 x 4)."""
import functools

import pytest
import torch

import multiscale_ref as MR
from arbiter import Verdicts, double_copy, perturb_, perturb_tensor
from seeding import reinit_by_name
from test_loss_gpu import grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, W = 2, 64, 128


def nets(seed=41, scales=4):
    from models.depth.resnet_dispnet import DispResNet
    from oracle import nets as on
    hip = reinit_by_name(DispResNet(scales=scales), seed)
    ref = on.DispResNet()
    ref.load_state_dict(hip.state_dict())
    return hip.to(DEV).train(), ref.train()


def test_scale0_is_bit_equal_to_the_single_scale_net():
    from models.depth.resnet_dispnet import DispResNet
    four, _ = nets()
    one = DispResNet().to(DEV).train()
    one.load_state_dict(four.state_dict())
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(43)).to(DEV)
    a, b = four(x), one(x)
    assert len(a) == 4 and len(b) == 1
    assert [tuple(t.shape) for t in a] == [(B, 1, H >> s, W >> s) for s in range(4)]
    assert torch.equal(a[0], b[0])
    pa, pb = four.forward_pair(x, x.flip(0)), one.forward_pair(x, x.flip(0))
    assert len(pa[0]) == 4 and len(pa[1]) == 4 and torch.equal(pa[0][0], pb[0][0]) and torch.equal(pa[1][0], pb[1][0])
    four.eval(), one.eval()
    with torch.no_grad():
        a, b = four(x), one(x)
        pa = four.forward_pair(x, x.flip(0))
    assert len(a) == 1 and len(pa[0]) == 1 and len(pa[1]) == 1 and torch.equal(a[0], b[0])


def test_all_scales_and_every_gradient_vs_fp64_arbiter():
    """All four outputs and EVERY parameter gradient -- the heads of scales 1 to 3 included -- against the oracle's encoder and decoder under the
    float64 arbiter, rule and constants of test_dispnets_gradients_vs_fp64_arbiter; a random coefficient map per scale as upstream."""
    hip, ref = nets()
    g = torch.Generator().manual_seed(53)
    x = torch.randn(B, 3, H, W, generator=g)
    want = MR.dispresnet_scales(ref, x)
    coefs = [torch.randn(o.shape, generator=g) for o in want]
    sum((o * c).sum() for o, c in zip(want, coefs)).backward()
    got = hip(x.to(DEV))
    assert len(got) == 4
    sum((o * c.to(DEV)).sum() for o, c in zip(got, coefs)).backward()

    def run64(net, xin):
        net.zero_grad()
        outs = MR.dispresnet_scales(net, xin)
        sum((o * c.double()).sum() for o, c in zip(outs, coefs)).backward()
        return outs, dict(net.named_parameters())
    out64, r64 = run64(double_copy(ref), x.double())
    envs = [run64(perturb_(double_copy(ref), 1e-6, 910 + e), perturb_tensor(x.double(), 1e-6, 960 + e))[1] for e in range(2)]
    v = Verdicts(floor=2.5e-4)
    for i, (a, b, c) in enumerate(zip(got, want, out64)):
        v.add("disp%d" % i, a, b, c)
    rp = dict(ref.named_parameters())
    judged = set()
    for n, q in hip.named_parameters():
        if rp[n].grad is not None:
            assert q.grad is not None, n
            v.add(n, q.grad, rp[n].grad, r64[n].grad, [env[n].grad for env in envs])
            judged.add(n)
    for s in range(4):                                       # decoder.decoder.10 .. 13 are the four heads
        assert {"decoder.decoder.%d.conv.weight" % (10 + s), "decoder.decoder.%d.conv.bias" % (10 + s)} <= judged
    v.check("test_all_scales_and_every_gradient_vs_fp64_arbiter", hip_abs=2e-3)


def test_forward_pair_equals_two_separate_calls():
    """forward_pair with 4 scales against two separate calls: comparison and tolerances of the existing pair test (test_step_gpu.py): the
    scalar within 1e-5 relative, the whole gradient within 1e-3 in L2."""
    hip, _ = nets(seed=141)
    state = {k: v.clone() for k, v in hip.state_dict().items()}
    g = torch.Generator().manual_seed(57)
    xa, xb = torch.randn(B, 3, H, W, generator=g).to(DEV), torch.randn(B, 3, H, W, generator=g).to(DEV)
    coefs = [[torch.randn(B, 1, H >> s, W >> s, generator=g).to(DEV) for s in range(4)] for _ in range(2)]

    def run(pair):
        hip.load_state_dict(state)
        hip.zero_grad()
        outs = hip.forward_pair(xa, xb) if pair else (hip(xa), hip(xb))
        assert len(outs[0]) == 4 and len(outs[1]) == 4
        loss = sum((o * c).sum() for per, cs in zip(outs, coefs) for o, c in zip(per, cs))
        loss.backward()
        return float(loss.detach()), torch.cat([p.grad.reshape(-1) for p in hip.parameters() if p.grad is not None]).clone()
    l1, g1 = run(True)
    l2, g2 = run(False)
    assert abs(l1 - l2) <= 1e-5 * abs(l2), (l1, l2)
    assert g1.numel() == g2.numel() and float((g1 - g2).norm() / g2.norm()) < 1e-3


# ------------------------------------------------------------------------------------------------ the loss
@functools.lru_cache(maxsize=None)
def loss_inputs():
    """The inputs of test_multiscale_losses_vs_oracle (seeds 31 / 32)."""
    from oracle.step import synthetic_batch
    s = synthetic_batch(B, H, W, seed=31)
    gen = torch.Generator().manual_seed(32)
    shapes = [(H, W), (H // 2, W // 2), (H // 4, W // 4), (H // 8, W // 8)]
    dt = [torch.rand(B, 1, h, w, generator=gen) for h, w in shapes]
    dr = [torch.rand(B, 1, h, w, generator=gen) for h, w in shapes]
    poses = 0.01 * torch.randn(B, 2, 6, generator=gen)
    return s["tgt"], s["ref_imgs"], s["intrinsics"], dt, dr, poses


@functools.lru_cache(maxsize=None)
def loss_reference(order, ssim, masked):
    """tests/multiscale_ref.py in float32, in float64, and in float64 on inputs perturbed by 1e-6 (the arbiter's envelope): computed once."""
    tgt, refs, K, dt, dr, poses = loss_inputs()
    modes = dict(order=order, ssim=ssim, min_reprojection=masked, automask=masked)
    r32 = MR.run(tgt, refs, dt, dr, poses, K, torch.float32, **modes)
    r64 = MR.run(tgt, refs, dt, dr, poses, K, torch.float64, **modes)
    env = []
    for e in range(2):
        pt = lambda t, k: perturb_tensor(t.double(), 1e-6, 1000 * (e + 1) + k)
        env.append(MR.run(pt(tgt, 3), [pt(r, 4 + i) for i, r in enumerate(refs)], [pt(d, 10 + i) for i, d in enumerate(dt)],
                          [pt(d, 20 + i) for i, d in enumerate(dr)], pt(poses, 2), K, torch.float64, **modes))
    return r32, r64, env


def hip_losses(fused, order, ssim, masked):
    from losses import Losses
    tgt, refs, K, dt, dr, poses = loss_inputs()
    x = [t.to(DEV).requires_grad_() for t in dt]
    y = [t.to(DEV).requires_grad_() for t in dr]
    z = poses.to(DEV).requires_grad_()
    crit = Losses(ssim=ssim, min_reprojection=masked, automask=masked, multiscale_upsample=order, fused_pyramid=fused)
    got = crit.forward(tgt.to(DEV), [r.to(DEV) for r in refs], [x, y], z, K.to(DEV), None)
    sum(got).backward()
    return [float(v.detach()) for v in got], [t.grad for t in x], [t.grad for t in y], z.grad


@pytest.mark.parametrize("order,ssim,masked", [("depth", False, False), ("depth", True, False), ("disparity", False, False),
                                               ("disparity", True, False), ("disparity", False, True)])
def test_fused_pyramid_vs_composition_and_definition(order, ssim, masked):
    """Losses(fused_pyramid=True) against fused_pyramid=False, and both against tests/multiscale_ref.py: loss values within 2e-5 relative,
    disparity gradients under test_multiscale_losses_vs_oracle's caps, the pose gradient under the float64 arbiter (as
    test_losses_vs_oracle_at_size judges it: the float32 CPU oracle is itself 4e-3 from float64 on these inputs in one mode)."""
    r32, r64, env = loss_reference(order, ssim, masked)
    fused = hip_losses(True, order, ssim, masked)
    plain = hip_losses(False, order, ssim, masked)
    close = lambda a, b: abs(a - b) <= 2e-5 * abs(b)
    for k in range(2):
        print("loss %d: fused %.8f composition %.8f definition %.8f" % (k, fused[0][k], plain[0][k], r32[0][k]))
        assert close(fused[0][k], plain[0][k]) and close(fused[0][k], r32[0][k]) and close(plain[0][k], r32[0][k])
    for i in range(4):
        numel = fused[1][i].numel()
        frac = max(5e-3, 8.0 / numel)
        l2 = 5e-3 if numel >= 4096 else 2e-2
        for t in (1, 2):
            grad_close(fused[t][i], r32[t][i], frac=frac, l2=l2)
            grad_close(plain[t][i], r32[t][i], frac=frac, l2=l2)
            grad_close(fused[t][i], plain[t][i].cpu(), frac=frac, l2=l2)
    v = Verdicts()
    v.add("d poses, fused", fused[3], r32[3], r64[3], [e[3] for e in env])
    v.add("d poses, composition", plain[3], r32[3], r64[3], [e[3] for e in env])
    v.check("test_fused_pyramid_vs_composition_and_definition[%s, ssim=%s, masked=%s]" % (order, ssim, masked))


def test_fused_pyramid_reads_forward_pair_outputs_in_place():
    """The two maps of a scale as forward_pair returns them are one stacked buffer: the pyramid takes it without a copy; separately allocated
    maps are concatenated.  Same result either way."""
    from mcav.multiscale import _stacked_pair, depth_pyramid
    g = torch.Generator().manual_seed(61)
    both = torch.rand(2 * B, 1, 16, 32, generator=g).to(DEV)
    buf, view = _stacked_pair(both[:B], both[B:])
    assert view and buf.data_ptr() == both.data_ptr() and tuple(buf.shape) == (2 * B, 1, 16, 32)
    buf2, view2 = _stacked_pair(both[:B].clone(), both[B:].clone())
    assert not view2 and torch.equal(buf2, both)
    a = depth_pyramid([both[:B]], [both[B:]], H, W)
    b = depth_pyramid([both[:B].clone()], [both[B:].clone()], H, W)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0])


# ------------------------------------------------------------------------------------------------ the trainer
def ms_trainer(graph):
    import dp_worker as WK
    from trainer import Trainer
    cfg = WK.build_config(H, W, B, graph)
    cfg["datasets"]["synthetic_length"] = 20          # (validation split 20 %: two batches for validate())
    cfg["model"]["depth"]["scales"] = 4
    cfg["loss"] = dict(fused_pyramid=True, multiscale_upsample="disparity")
    t = Trainer(cfg)
    assert t.depth_model.scales == 4 and t.criterion.fused_pyramid and t.criterion.multiscale_upsample == "disparity"
    WK.seed_models(t)
    t.set_train()
    return t


def test_trainer_multiscale_eager_hipgraph_epoch_and_validate():
    """model.depth.scales: 4 with loss: {fused_pyramid: true, multiscale_upsample: disparity}: one eager step and one hipGraph-replayed step
    from the same state give equal losses (as test_trainer_stereo_eager_and_hipgraph compares them); after the step every dispconv head has a
    non-zero gradient; a short synthetic epoch runs; validate() still runs (eval mode: scale 0 only)."""
    import numpy as np
    t0 = ms_trainer(0)
    batch = next(iter(t0.train_loader))
    results = []
    for t in (t0, ms_trainer(1)):
        outputs, loss = t.train_step(batch)
        torch.cuda.synchronize()
        results.append([float(x.detach()) for x in loss])
        for s in range(4):
            w = t.depth_model.decoder.conv("dispconv", s).conv.weight
            assert w.grad is not None and float(w.grad.abs().max()) > 0, s
    le, lg = results
    assert all(np.isfinite(x) for x in le)
    assert all(abs(x - y) <= 1e-6 * abs(y) for x, y in zip(le, lg)), (le, lg)
    before = t0.step
    t0.run_epoch()
    assert t0.step > before and torch.isfinite(sum(t0.loss)).item()
    acc = t0.validate()
    assert acc is not None
    assert t0.depth_model.training
