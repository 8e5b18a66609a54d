"""GPU: the networks in EVAL mode -- what validation, inference and everything behind them run -- against the float64 oracle.

Eval mode takes its own path (conv_bn(..., train=False) in mcav/depthnet.py, tape.batchnorm(..., train=False) for DispNetS): convolutions without
the statistics epilogue, mcav_bn_eval_coeffs on the running statistics, bn_apply / stem_bn_relu_pool_fwd on one-group coefficients even when two
passes are stacked.  Every other eval-mode assertion of the suite compares HIP with HIP; here every one compares with the oracle.

Cases: tests/eval_mode_cases.py (calibrated BatchNorm buffers that equal no batch's statistics; tests/test_eval_mode_cpu.py shows that batch
statistics, default buffers, a squared variance or ONE layer with default buffers move the float64 oracle by 7.6 .. 980 in depth max-relative,
0.26 .. 0.75 on DispNetS's outputs -- against the 1e-3 applied here).

Rules.
  * Features, disparity, DispNetS's outputs: the float64 arbiter (tests/arbiter.py), L2-relative per tensor,
        |HIP - fp64| <= 2 x max(|CPU fp32 oracle - fp64|, envelope, 2.5e-4),
    envelope = two float64 runs on weights and input perturbed by 1e-6.
  * Depth 1 / (10 d + 0.01) against the float64 oracle's: max-relative < 1e-3, AbsRel < 1e-4 (tests/test_step_gpu.py's full-size numbers);
    DispNetS's four outputs rel_err < 1e-3 (tests/test_nets_gpu.py's).
  * bf16: the train-mode statement's bounds (tests/test_bf16_gpu.py): max-relative 0.25, AbsRel 0.03, and the same net switched to fp32 at
    least 20 x closer in AbsRel.
  * Eval semantics are bit properties: torch.equal.

Measured on MI355X, worst over the input shapes and over single / stacked passes.  L2-relative |HIP - fp64|: the worst encoder feature and the
scale-0 disparity; then depth max-relative and AbsRel against float64 (the CPU fp32 oracle's own: 1.6e-5 .. 9.5e-5 and 2.7e-6 .. 1.0e-5):
                                 worst feature   disparity   depth max-rel   depth AbsRel
    DispResNet    default           2.2e-6        2.2e-6        2.8e-5          3.2e-6
    DispResNet    fp32-mfma         3.3e-6        3.3e-6        4.2e-5          4.6e-6
    DispResNet50  default           1.7e-5        7.7e-6        9.0e-5          1.0e-5
    DispResNet50  fp32-mfma         1.8e-5        8.6e-6        1.0e-4          1.2e-5
    DispResNetMS  default           2.4e-6        2.4e-6        2.7e-5          3.5e-6
    DispResNetMS  fp32-mfma         3.7e-6        3.6e-6        3.9e-5          5.1e-6
    DispNetS      default           four outputs: L2-relative 6.2e-7, rel_err 1.7e-6 (CPU fp32 oracle 1.4e-6)
    DispNetS      fp32-mfma         four outputs: L2-relative 6.2e-7, rel_err 1.4e-6
    every envelope and every CPU fp32 column is below 1.2e-4, so the floor of 2.5e-4 decides: the bound is 5e-4 L2-relative on every tensor.
    bf16 (DispResNet)               2x3x64x128: max-rel 0.180, AbsRel 0.0290;  3x3x96x160: max-rel 0.231, AbsRel 0.0262 -- inside 0.25 / 0.03, by
                                    3 % and 8 %: eval mode has no batch-statistics noise, but no batch statistics that re-centre every layer either;
                                    the same module switched to fp32: AbsRel 3.1e-6 / 3.2e-6 (9000 x closer)
    hand-off                        running statistics rel_err 6.0e-7 (CPU fp32 oracle 5.1e-7); then eval: 2.7e-6 L2, depth 2.4e-5 / 3.0e-6
    checkpoint                      features 2.3e-6 L2; depth 1.7e-7 / 3.7e-8: after the 8 steps of the synthetic epoch the disparity is nearly flat
                                    (all of it inside (0.02, 0.98)), so the five feature maps carry this comparison
"""
import functools

import pytest
import torch

import eval_mode_cases as E
from arbiter import Verdicts, perturb_, perturb_tensor
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("default", "fp32-mfma")
# ResNet-50 at the small shape only (the float64 oracle of the larger one is seconds of host time)
NET_SHAPES = [(n, s) for n in E.NETS for s in E.SHAPES if not (n == "DispResNet50" and s != E.SHAPES[0])]


# ------------------------------------------------------------------------------------------------ the oracle's side, computed once
def oracle_run(net, x):
    """-> (encoder features or None, outputs) of an oracle net in the mode it is in, no grad"""
    with torch.no_grad():
        if hasattr(net, "encoder"):
            feats = net.encoder(x)
            return [f.detach() for f in feats], [net.decoder(feats)[("disp", 0)].detach()]
        return None, [o.detach() for o in net(x)]


@functools.lru_cache(maxsize=None)
def reference(name, shape, seed=7):
    """x and what the oracle makes of it in eval mode: fp32 (the yardstick), float64 (the reference), and float64 on 1e-6-perturbed weights and
    input, twice (the envelope).  Shared by every test of the case; nothing here is modified afterwards."""
    x = E.image(shape, seed)
    r32 = E.loaded_oracle(name)
    r64 = E.loaded_oracle(name, torch.float64)
    out = dict(x=x, cpu32=oracle_run(r32, x), ref64=oracle_run(r64, x.double()), env=[])
    for e in range(2):
        out["env"].append(oracle_run(perturb_(E.loaded_oracle(name, torch.float64), 1e-6, 900 + e), perturb_tensor(x.double(), 1e-6, 950 + e)))
    return out


def loaded_hip(name, mode="default", **kw):
    from mcav import nn as N
    hip = E.hip_net(name, **kw)
    hip.load_state_dict(E.calibrated(name), strict=True)
    if mode != "default":
        N.set_compute_dtype(hip, mode)
    return hip.to(DEV).eval()


def hip_features(hip, xs):
    """the five encoder maps (NCHW) of depthnet.encoder_forward(..., train=False) on the images of xs stacked along the batch, as forward_pair
    stacks them (groups = len(xs): in eval mode the coefficients stay one group)"""
    from mcav import depthnet as D
    from mcav import nn as N
    from models.depth.resnet_dispnet import _to_nhwc4
    with torch.no_grad():
        feats, _ = D.encoder_forward(hip.encoder.encoder, _to_nhwc4(torch.cat(xs).contiguous()), False, groups=len(xs))
        return [N.nhwc_to_nchw(f) for f in feats]


def judge(v, tag, got_feats, got_outs, ref, part=None):
    """rows for the arbiter; part = (lo, hi): the rows of the stacked batch that belong to this reference"""
    cut = (lambda t: t) if part is None else (lambda t: t[part[0]:part[1]])
    if got_feats is not None:
        for i, f in enumerate(got_feats):
            v.add("%s f%d" % (tag, i), cut(f), ref["cpu32"][0][i], ref["ref64"][0][i], [env[0][i] for env in ref["env"]])
    for i, o in enumerate(got_outs):
        v.add("%s out%d" % (tag, i), o, ref["cpu32"][1][i], ref["ref64"][1][i], [env[1][i] for env in ref["env"]])


def check_depth(tag, got, ref):
    """depth of the scale-0 disparity against the float64 oracle's; prints, then asserts the full-size numbers"""
    mx, ab = E.depth_errors(got, ref["ref64"][1][0])
    mx32, ab32 = E.depth_errors(ref["cpu32"][1][0], ref["ref64"][1][0])
    print("  %-34s depth vs fp64: HIP max-rel %.3e AbsRel %.3e | CPU fp32 oracle max-rel %.3e AbsRel %.3e" % (tag, mx, ab, mx32, ab32))
    assert mx < E.DEPTH_MAX_REL and ab < E.DEPTH_ABS_REL, (tag, mx, ab)
    return mx, ab


def check_dispnets(tag, got, ref):
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, ref["ref64"][1])):
        e, e32 = rel_err(a, b), rel_err(ref["cpu32"][1][i], b)
        print("  %-34s disp%d vs fp64: HIP rel_err %.3e | CPU fp32 oracle %.3e" % (tag, i + 1, e, e32))
        worst = max(worst, e)
    assert worst < E.DISPNETS_REL, (tag, worst)


# ------------------------------------------------------------------------------------------------ 3. the networks against the oracle
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,shape", NET_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_eval_network_vs_oracle(name, shape, mode):
    ref = reference(name, shape)
    hip = loaded_hip(name, mode)
    x = ref["x"].to(DEV)
    v = Verdicts(factor=2.0, floor=2.5e-4)
    tag = "%s %s" % (name, mode)
    with torch.no_grad():
        out = list(hip(x))
    if name == "DispNetS":
        assert len(out) == 4
        judge(v, tag, None, out, ref)
        v.check("test_eval_network_vs_oracle[%s %s]" % (tag, shape))
        check_dispnets(tag, out, ref)
        return
    assert len(out) == 1 and out[0].shape == (shape[0], 1, shape[2], shape[3])      # eval: scale 0 only, DispResNetMS too
    judge(v, tag, hip_features(hip, [x]), out, ref)
    # the stacked form: two passes in one launch set, one-group eval coefficients; the oracle sees two calls
    ref_b = reference(name, shape, 9)
    xb = ref_b["x"].to(DEV)
    with torch.no_grad():
        pa, pb = hip.forward_pair(x, xb)
    assert len(pa) == 1 and len(pb) == 1
    pf = hip_features(hip, [x, xb])
    B = shape[0]
    judge(v, tag + " pair.a", pf, pa, ref, part=(0, B))
    judge(v, tag + " pair.b", pf, pb, ref_b, part=(B, 2 * B))
    v.check("test_eval_network_vs_oracle[%s %s]" % (tag, shape))
    check_depth(tag, out[0], ref)
    check_depth(tag + " pair.a", pa[0], ref)
    check_depth(tag + " pair.b", pb[0], ref_b)


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_eval_bf16_statement(shape):
    """bf16 conv tiles in eval mode inside the train-mode statement's own bounds (no batch-statistics noise here), and it is the bf16 path that
    ran: the same module switched to fp32 is at least 20 x closer in AbsRel and inside the fp32 bounds."""
    from mcav import nn as N
    name = "DispResNet"
    ref = reference(name, shape)
    hip = loaded_hip(name, dtype=torch.bfloat16)
    x = ref["x"].to(DEV)
    with torch.no_grad():
        got = hip(x)[0]
    mx, ab = E.depth_errors(got, ref["ref64"][1][0])
    print("  bf16 eval %s: depth vs fp64 max-rel %.3e AbsRel %.3e, disparity max-abs %.3e" %
          (shape, mx, ab, float((got.cpu().double() - ref["ref64"][1][0]).abs().max())))
    assert mx < 0.25 and ab < 0.03
    N.set_compute_dtype(hip, torch.float32)
    with torch.no_grad():
        mx32, ab32 = check_depth("the same module in fp32", hip(x)[0], ref)
    assert ab32 * 20 < ab, (ab32, ab)


# ------------------------------------------------------------------------------------------------ eval semantics, bit for bit
@pytest.mark.parametrize("name", E.NETS)
def test_eval_is_deterministic_and_per_image(name):
    """two eval forwards are equal; image 0's output does not change when the other images of the batch are replaced (same batch size: the same
    kernels and tiles, and nothing of the batch enters an eval-mode BatchNorm)"""
    shape = E.SHAPES[1]
    hip = loaded_hip(name)
    x = E.image(shape, 7).to(DEV)
    y = x.clone()
    y[1:] = E.image(shape, 8).to(DEV)[1:]
    with torch.no_grad():
        a, b, c = list(hip(x)), list(hip(x)), list(hip(y))
    for p, q, r in zip(a, b, c):
        assert torch.equal(p, q)
        assert torch.equal(p[0], r[0]) and not torch.equal(p[1:], r[1:])
    if name in E.RESNETS:
        with torch.no_grad():
            (pa, pb), (qa, qb) = hip.forward_pair(x, y), hip.forward_pair(y, x)
        assert torch.equal(pa[0][0], qa[0][0]) and torch.equal(pb[0][0], qb[0][0])      # image 0 of either pass, whatever else is stacked with it
        assert not torch.equal(pa[0][1:], qa[0][1:])


@pytest.mark.parametrize("which", ("PoseNet", "PoseFc"))
def test_pose_nets_have_no_mode(which):
    """no BatchNorm, no dropout: eval output == train output, bit for bit"""
    from seeding import reinit_by_name
    if which == "PoseNet":
        from models.pose.pose_net import PoseNet as Net
        shape = (3, 3, 96, 160)
    else:
        from models.pose.pose_fc import PoseFc as Net
        shape = (1, 3, 384, 1280)                       # the only size its head admits
    m = reinit_by_name(Net(), 21).to(DEV)
    tgt, r0, r1 = (E.image(shape, 60 + i).to(DEV) for i in range(3))
    with torch.no_grad():
        a = m.train()(tgt, [r0, r1])
        b = m.eval()(tgt, [r0, r1])
        c = m.train()(tgt, [r0, r1])
    assert torch.equal(a, b) and torch.equal(a, c) and float(a.abs().max()) > 0


@pytest.mark.parametrize("name", E.NETS)
def test_eval_leaves_state_alone(name):
    """forward (and forward_pair) in eval, with grad enabled: every running statistic and counter bit-identical afterwards, no counter update
    pending, no parameter has gained a .grad"""
    from mcav import nn as N
    hip = loaded_hip(name)
    N.flush_bn_counters()
    before = {k: v.clone() for k, v in hip.state_dict().items()}
    x = E.image(E.SHAPES[0], 7).to(DEV)
    out = list(hip(x))
    assert all(o.requires_grad for o in out)               # (an autograd node was recorded: this is the path a stray backward would take)
    if name in E.RESNETS:
        hip.forward_pair(x, x.flip(0).contiguous())
    torch.cuda.synchronize()
    assert not N._NBT_PENDING
    N.flush_bn_counters()
    after = hip.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert any(k.endswith("num_batches_tracked") and int(v) == E.CALIBRATION_STEPS for k, v in after.items())
    assert all(p.grad is None for p in hip.parameters())


# ------------------------------------------------------------------------------------------------ 4. train -> eval hand-off, checkpoint path
def test_train_to_eval_handoff():
    """Three train-mode forwards without an optimiser -- two single batches and one forward_pair, which the oracle sees as two calls, tgt then
    ref -- from the calibrated state: every running statistic within 1e-5 rel_err of the float64 oracle's (the bar of
    test_batchnorm_train_and_backward; the CPU fp32 oracle sits at 5.8e-7), every counter equal.  Then both go to eval and meet the bounds above:
    the momentum update order of the stacked passes, and that eval reads what training left."""
    name, shape = "DispResNet", E.SHAPES[0]
    hip = loaded_hip(name).train()
    r32 = E.loaded_oracle(name).train()
    r64 = E.loaded_oracle(name, torch.float64).train()
    xs = [E.image(shape, 30 + i) for i in range(4)]
    with torch.no_grad():
        hip(xs[0].to(DEV)); hip(xs[1].to(DEV)); hip.forward_pair(xs[2].to(DEV), xs[3].to(DEV))
        for x in xs:
            r32(x); r64(x.double())
    torch.cuda.synchronize()
    hs, s32, s64 = hip.state_dict(), r32.state_dict(), r64.state_dict()
    worst = (0.0, None)
    for k in hs:
        if k.endswith("num_batches_tracked"):
            assert int(hs[k]) == int(s64[k]) == E.CALIBRATION_STEPS + 4, k
        elif "running_" in k:
            e = rel_err(hs[k], s64[k])
            worst = max(worst, (e, k))
            assert e < 1e-5, (k, e, rel_err(s32[k], s64[k]))
            assert not torch.equal(hs[k].cpu(), E.calibrated(name)[k])
    print("  hand-off: worst running statistic %s rel_err %.3e (CPU fp32 oracle %.3e)" % (worst[1], worst[0], rel_err(s32[worst[1]], s64[worst[1]])))
    hip.eval(); r32.eval(); r64.eval()
    x = E.image(shape, 7)
    ref = dict(cpu32=oracle_run(r32, x), ref64=oracle_run(r64, x.double()), env=[])
    for e in range(2):
        pert = E.oracle_net(name).double()
        pert.load_state_dict(s64)
        ref["env"].append(oracle_run(perturb_(pert.eval(), 1e-6, 900 + e), perturb_tensor(x.double(), 1e-6, 950 + e)))
    v = Verdicts(factor=2.0, floor=2.5e-4)
    with torch.no_grad():
        out = hip(x.to(DEV))
    judge(v, "hand-off", hip_features(hip, [x.to(DEV)]), out, ref)
    v.check("test_train_to_eval_handoff")
    check_depth("hand-off", out[0], ref)


def test_checkpoint_to_inference_vs_oracle(tmp_path, monkeypatch):
    """Trainer (synthetic config, one short epoch) -> save_chkpnt -> inference.Inference(cfg, checkpoint=...): the BatchNorm buffers read back from
    the file are the trainer's, bit for bit, and Inference.disparity equals the oracle DispResNet loaded from the same file (strict) in eval."""
    import os
    import yaml
    from conftest import PKG
    from inference import Inference
    from oracle import nets as on
    from trainer import Trainer
    monkeypatch.chdir(tmp_path)
    cfg = yaml.full_load(open(os.path.join(PKG, "configs", "basic_config.yaml")))
    cfg["datasets"]["augmentation"].update(image_width=128, image_height=64)
    cfg["datasets"]["synthetic_length"] = 20
    cfg["action"].update(batch_size=2, verbose=False, save_checkpoints=False)
    t = Trainer(cfg)
    t.train()
    t.save_chkpnt()
    torch.cuda.synchronize()
    path = os.path.join(str(tmp_path), t.save_path)
    inf = Inference(cfg, checkpoint=path)
    state = torch.load(path, map_location="cpu")["dpth_mdl_state_dict"]
    trained = t.depth_model.state_dict()
    moved = 0
    for k, v in inf.depth_model.state_dict().items():
        assert torch.equal(v.cpu(), state[k]) and torch.equal(v, trained[k]), k
        if k.endswith("running_var"):
            moved += int(not bool((v == 1).all()))
        if k.endswith("num_batches_tracked"):
            assert int(v) > 0 and t.step > 0, k
    assert moved > 0
    r32 = on.DispResNet()
    r32.load_state_dict(state, strict=True)
    r32.eval()
    r64 = on.DispResNet()
    r64.load_state_dict(state, strict=True)
    r64.double().eval()
    x = E.image(E.SHAPES[0], 7)
    ref = dict(cpu32=oracle_run(r32, x), ref64=oracle_run(r64, x.double()), env=[])
    for e in range(2):
        pert = on.DispResNet()
        pert.load_state_dict(state, strict=True)
        ref["env"].append(oracle_run(perturb_(pert.double().eval(), 1e-6, 900 + e), perturb_tensor(x.double(), 1e-6, 950 + e)))
    got = inf.disparity(x)
    assert got.shape == (2, 1, 64, 128) and not inf.depth_model.training
    inside = float(((ref["ref64"][1][0] > 0.02) & (ref["ref64"][1][0] < 0.98)).double().mean())
    print("  checkpoint after %d steps: %.3f of the oracle's disparity inside (0.02, 0.98)" % (t.step, inside))
    assert inside >= 0.8 and all(float(f.std()) > 0 for f in ref["ref64"][0])
    v = Verdicts(factor=2.0, floor=2.5e-4)
    judge(v, "checkpoint", hip_features(inf.depth_model, [x.to(DEV)]), [got], ref)
    v.check("test_checkpoint_to_inference_vs_oracle")
    check_depth("checkpoint", got, ref)


# ------------------------------------------------------------------------------------------------ 5. backward through an eval-mode network
@pytest.mark.parametrize("name", ("DispResNet", "DispNetS"))
def test_backward_through_eval_is_refused_before_anything_runs(name):
    """The BatchNorm backward needs the batch statistics an eval-mode forward never saved.  The refusal is a host-side check at the FRONT of the
    backward: MCAVError, no parameter's .grad touched (not even those of the layers behind the first BatchNorm), nothing pending on the
    weight-gradient stream -- and the next train-mode backward in this process gives, bit for bit, what a module that never saw the refused
    one gives."""
    from mcav import nn as N
    from mcav.lib import MCAVError
    hip, fresh = loaded_hip(name), loaded_hip(name)
    x = E.image(E.SHAPES[0], 7).to(DEV)
    coef = [E.image(tuple(o.shape), 70 + i).to(DEV) for i, o in enumerate(reference(name, E.SHAPES[0])["ref64"][1])]
    marks = {}
    for n, p in hip.named_parameters():
        p.grad = torch.full_like(p, 0.5)
        marks[n] = p.grad
    calls = [lambda: hip(x)]
    if name in E.RESNETS:
        calls.append(lambda: hip.forward_pair(x, x.flip(0).contiguous())[0])
    for call in calls:
        out = list(call())
        with pytest.raises(MCAVError):
            sum((o * c).sum() for o, c in zip(out, coef)).backward()
        torch.cuda.synchronize()
        for n, p in hip.named_parameters():
            assert p.grad is marks[n] and bool((p.grad == 0.5).all()), n
        assert not N.WGRAD_SIDE.in_backward and not N.WGRAD_SIDE.forked and not N.WGRAD_BATCH.items and not N.WGRAD_SIDE.mains
    grads = []
    for m in (hip, fresh):
        m.train()
        for p in m.parameters():
            p.grad = None
        out = list(m(x))[:len(coef)]
        sum((o * c).sum() for o, c in zip(out, coef)).backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad for n, p in m.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n
