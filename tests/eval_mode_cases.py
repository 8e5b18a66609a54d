"""Eval-mode network cases shared by tests/test_eval_mode_cpu.py and tests/test_eval_mode_gpu.py (test infrastructure).

A freshly seeded net is useless in eval mode: reinit_by_name's weights under unit running variances let the activations grow from block to
block, the oracle's ResNet-50 disparity saturates at exactly 1.0 and ResNet-18's spans 2e-10 .. 1, so every comparison would pass on a constant.
calibrated() therefore gives the BatchNorm buffers the statistics of the net's own activations -- 20 train-mode forwards of the float64 oracle --
and then moves every buffer off them (running_mean += 0.1 sqrt(running_var) N(0,1), running_var *= exp(0.2 N(0,1))): what eval mode must read is
the BUFFERS, which after this equal no batch's statistics, so "batch statistics in eval mode" cannot pass by coincidence either.

The state is float32 (what a checkpoint holds); the HIP module and the oracle load the same tensors, the float64 oracle is the oracle .double().
MUTATIONS are the wiring errors the eval-mode tests exist to catch, applied to the float64 oracle: tests/test_eval_mode_cpu.py asserts that each
moves the output by at least 10 x the bound the GPU tests hold the HIP networks to.
"""
import copy
import functools

import torch

from seeding import reinit_by_name

SEED = 141
NETS = ("DispResNet", "DispResNet50", "DispResNetMS", "DispNetS")
RESNETS = NETS[:3]
SEEDS = {"DispResNet": SEED, "DispResNet50": SEED, "DispResNetMS": SEED + 2, "DispNetS": SEED}      # (the two ResNet-18 nets: two states)
SHAPES = ((2, 3, 64, 128), (3, 3, 96, 160))         # an odd batch, and a second tile geometry
CALIBRATION_SHAPE, CALIBRATION_STEPS = (4, 3, 64, 128), 20
# what the GPU tests hold the HIP networks to (tests/test_step_gpu.py's full-size numbers; tests/test_nets_gpu.py's for DispNetS's outputs) ...
DEPTH_MAX_REL, DEPTH_ABS_REL, DISPNETS_REL = 1e-3, 1e-4, 1e-3
SEPARATION = 10.0                                    # ... and how many times that every wrong definition must move the float64 oracle
# the one BatchNorm mutation (d) resets: the middle of the encoder
SINGLE_BN = {"DispResNet": "encoder.encoder.layer2.0.bn1", "DispResNet50": "encoder.encoder.layer2.0.bn1", "DispResNetMS": "encoder.encoder.layer2.0.bn1",
             "DispNetS": "conv3.2"}


def oracle_net(name):
    from oracle import nets as on
    return {"DispResNet": lambda: on.DispResNet(18), "DispResNet50": lambda: on.DispResNet(50), "DispResNetMS": lambda: on.DispResNet(18),
            "DispNetS": on.DispNetS}[name]()


def hip_net(name, **kw):
    """the HIP module of the same name (imports, and builds, without a GPU)"""
    if name == "DispNetS":
        from models.depth.disp_net import DispNetS
        return DispNetS(**kw)
    from models.depth import resnet_dispnet as m
    if kw:
        return m.DispResNet({"DispResNet": 18, "DispResNet50": 50, "DispResNetMS": 18}[name], scales=4 if name == "DispResNetMS" else 1, **kw)
    return getattr(m, name)()


def image(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def batchnorms(net):
    return [(n, m) for n, m in net.named_modules() if hasattr(m, "running_var") and m.running_var is not None]


@functools.lru_cache(maxsize=None)
def calibrated(name, seed=None):
    """-> the calibrated float32 state_dict of net `name` (module docstring).  Cached: treat the tensors as read-only."""
    seed = SEEDS[name] if seed is None else seed
    net = reinit_by_name(oracle_net(name), seed).double().train()
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for _ in range(CALIBRATION_STEPS):
            net(torch.randn(CALIBRATION_SHAPE, generator=g, dtype=torch.float64))
        for _, bn in batchnorms(net):
            bn.running_mean += 0.1 * torch.sqrt(bn.running_var) * torch.randn(bn.running_mean.shape, generator=g, dtype=torch.float64)
            bn.running_var *= torch.exp(0.2 * torch.randn(bn.running_var.shape, generator=g, dtype=torch.float64))
    return {k: (v.float() if v.dtype.is_floating_point else v.clone()) for k, v in net.state_dict().items()}


def loaded_oracle(name, dtype=torch.float32):
    """a new oracle net holding the calibrated state (strict), in eval mode"""
    net = oracle_net(name)
    net.load_state_dict(calibrated(name), strict=True)
    return net.to(dtype).eval()


def outputs(net, x):
    """-> the list of output maps: [scale-0 disparity] for the ResNets, the four maps for DispNetS"""
    with torch.no_grad():
        return [o.detach() for o in net(x)]


def depth(disp):
    return 1.0 / (10.0 * disp.detach().cpu().double() + 0.01)


def depth_errors(got, want):
    """-> (max-relative, AbsRel) of the depth of disparity `got` against that of `want`"""
    dg, dw = depth(got), depth(want)
    rel = (dg - dw).abs() / dw
    return float(rel.max()), float(rel.mean())


# ------------------------------------------------------------------------------------------------ the wrong definitions
def _batch_statistics(net, name):
    return net.train()


def _default_buffers(net, name):
    for _, bn in batchnorms(net):
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
    return net


def _var_squared(net, name):
    for _, bn in batchnorms(net):
        bn.running_var.pow_(2)
    return net


def _one_default_layer(net, name):
    bn = dict(batchnorms(net))[SINGLE_BN[name]]
    bn.running_mean.zero_(); bn.running_var.fill_(1.0)
    return net


MUTATIONS = {"batch statistics": _batch_statistics, "default buffers": _default_buffers, "var squared": _var_squared,
             "one layer's buffers default": _one_default_layer}


def mutated(net, name, mutation):
    """a deep copy of the (eval-mode) oracle `net` with the named wrong definition applied"""
    with torch.no_grad():
        return MUTATIONS[mutation](copy.deepcopy(net), name)
