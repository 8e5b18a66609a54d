"""CPU: the eval-mode cases of tests/eval_mode_cases.py are worth comparing against.

tests/test_eval_mode_gpu.py holds the HIP networks in eval mode to the float64 oracle on these cases.  That says something only if (1) both
sides load the same state, (2) the oracle's eval output is not saturated or constant, (3) the wiring errors the GPU tests exist to catch move
that output by far more than the bound they apply, and (4) eval mode in the oracle has the batch independence the GPU tests assert bit for bit.
All four are checked here, on the float64 oracle alone, so they are known without a GPU.

Measured (float64 oracle, the smaller of the two input shapes' values; depth max-relative for the ResNets, rel_err of the worst output for
DispNetS; asserted >= 10 x the GPU tests' bound, i.e. 1e-2; last column: scale 0 inside (0.02, 0.98), asserted >= 0.8):
                     batch statistics   default buffers   var squared   one layer's buffers default     usable fraction
    DispResNet             141                765             219                 51.8                       0.89
    DispResNet50           166                  1.0 *         448                  7.6                       0.93
    DispResNetMS           148                857              24.5              435                         0.83
    DispNetS                 0.26               0.62            0.55               0.26                      (outputs span 0.4 .. 10)
    * the mutant's disparity saturates at 1.0: depth 1 / (10 d + 0.01) then sits at its floor wherever the right one is larger
"""
import functools

import pytest
import torch

import eval_mode_cases as E
from conftest import rel_err


@functools.lru_cache(maxsize=None)
def oracle64(name):
    return E.loaded_oracle(name, torch.float64)


@functools.lru_cache(maxsize=None)
def right(name, shape):
    return E.outputs(oracle64(name), E.image(shape, 7).double())


@pytest.mark.parametrize("name", E.NETS)
def test_state_dicts_are_interchangeable(name):
    """keys (and their order), shapes and dtypes of the HIP module's state_dict equal the oracle's; the calibrated state loads strictly into both
    and comes back bit for bit"""
    hip, ref = E.hip_net(name), E.oracle_net(name)
    hs, rs = hip.state_dict(), ref.state_dict()
    assert list(hs) == list(rs)
    for k in hs:
        assert hs[k].shape == rs[k].shape and hs[k].dtype == rs[k].dtype, k
    state = E.calibrated(name)
    assert list(state) == list(rs)
    hip.load_state_dict(state, strict=True)
    ref.load_state_dict(state, strict=True)
    for k, v in hip.state_dict().items():
        assert torch.equal(v, state[k]) and torch.equal(ref.state_dict()[k], state[k]), k
    assert not hip.eval().training and all(not m.training for m in hip.modules())


@pytest.mark.parametrize("name", E.NETS)
def test_calibrated_buffers_are_no_batch_statistics(name):
    """every running statistic moved away from the defaults, variances positive, and the two ResNet-18 cases are two different states"""
    state = E.calibrated(name)
    for k, v in state.items():
        if k.endswith("running_var"):
            assert bool((v > 0).all()) and not bool((v == 1).all()), k
        if k.endswith("running_mean"):
            assert bool((v != 0).any()), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == E.CALIBRATION_STEPS
    assert E.calibrated(name) is state                        # cached
    if name == "DispResNetMS":
        assert not torch.equal(state["encoder.encoder.bn1.running_mean"], E.calibrated("DispResNet")["encoder.encoder.bn1.running_mean"])


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
@pytest.mark.parametrize("name", E.NETS)
def test_oracle_eval_output_is_usable(name, shape):
    outs = right(name, shape)
    if name in E.RESNETS:
        assert len(outs) == 1 and outs[0].shape == (shape[0], 1, shape[2], shape[3])
        inside = float(((outs[0] > 0.02) & (outs[0] < 0.98)).double().mean())
        print("%s %s: %.3f of scale 0 inside (0.02, 0.98), range %.3g .. %.3g" % (name, shape, inside, float(outs[0].min()), float(outs[0].max())))
        assert inside >= 0.8
    else:
        assert len(outs) == 4
        for o in outs:
            spread = float(o.max() - o.min())
            print("%s %s: output %s spans %.3g .. %.3g" % (name, shape, tuple(o.shape), float(o.min()), float(o.max())))
            assert spread > 1e-3 * float(o.abs().max())       # not constant


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
@pytest.mark.parametrize("name", E.NETS)
def test_wrong_definitions_are_far_outside_the_bound(name, shape):
    """each mutation of eval_mode_cases.MUTATIONS, applied to the float64 oracle, differs from the right one by >= 10 x the bound the GPU tests
    use: depth max-relative 1e-3 for the ResNets, rel_err 1e-3 on the outputs for DispNetS"""
    x = E.image(shape, 7).double()
    want = right(name, shape)
    for mutation in E.MUTATIONS:
        got = E.outputs(E.mutated(oracle64(name), name, mutation), x)
        if name in E.RESNETS:
            moved, bound = E.depth_errors(got[0], want[0])[0], E.DEPTH_MAX_REL
        else:
            moved, bound = max(rel_err(a, b) for a, b in zip(got, want)), E.DISPNETS_REL
        print("%-14s %-16s %-28s moves the output by %.3g (bound %g)" % (name, shape, mutation, moved, bound))
        assert moved >= E.SEPARATION * bound, (mutation, moved)
    assert not oracle64(name).training                       # the mutations worked on copies
    assert all(torch.equal(a, b) for a, b in zip(E.outputs(oracle64(name), x), want))


@pytest.mark.parametrize("name", E.NETS)
def test_oracle_eval_is_per_image(name):
    """image 0's eval output does not change when the other images of the batch are replaced (the batch size stays)"""
    shape = E.SHAPES[1]
    x = E.image(shape, 7).double()
    y = x.clone()
    y[1:] = E.image(shape, 8).double()[1:]
    for a, b in zip(right(name, shape), E.outputs(oracle64(name), y)):
        assert float((a[0] - b[0]).abs().max()) == 0.0
        assert float((a[1:] - b[1:]).abs().max()) > 0.0
