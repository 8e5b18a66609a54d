"""CPU: the multi-scale DispResNet's construction, checkpoints and config keys, the loss switches, and tests/multiscale_ref.py against the
oracle it is built from (no GPU call)."""
import json
import os
import types

import pytest
import torch

from conftest import GOLDEN


def test_dispresnet_scales_construct_with_the_same_state_dict():
    from models.depth.resnet_dispnet import DispResNet, DispResNet50MS, DispResNetMS
    want = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["DispResNet"]
    one, four = DispResNet(), DispResNet(scales=4)
    assert one.scales == 1 and four.scales == 4
    for m in (one, four, DispResNet(18, None, 2), DispResNetMS()):
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == want
    assert DispResNetMS().scales == 4 and DispResNet50MS().scales == 4
    assert list(DispResNet50MS().state_dict()) == list(DispResNet(50).state_dict())
    # training returns every scale, evaluation scale 0 only
    assert four.train().active_scales() == (0, 1, 2, 3) and four.eval().active_scales() == (0,)
    assert one.train().active_scales() == (0,)


def test_checkpoints_move_between_scale_counts():
    from models.depth.resnet_dispnet import DispResNet
    torch.manual_seed(5)
    one, four = DispResNet(), DispResNet(scales=4)
    four.load_state_dict(one.state_dict())                  # strict: every key present, none unexpected
    back = DispResNet()
    back.load_state_dict(four.state_dict())
    for (k, a), (_, b) in zip(one.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("bad", [0, 5, -1, 2.0, "4", True, None])
def test_bad_scales_raise(bad):
    from models.depth.resnet_dispnet import DispResNet
    with pytest.raises(ValueError, match="scales"):
        DispResNet(scales=bad)


def test_config_key_model_depth_scales():
    from trainer import Trainer
    stub = types.SimpleNamespace(train_from_scratch=True, device=torch.device("cpu"))
    cfg = lambda name, **kw: {"model": {"depth": dict(file="resnet_dispnet", name=name, **kw)}}
    assert Trainer.load_from_config(stub, cfg("DispResNet", scales=4), "depth").scales == 4
    assert Trainer.load_from_config(stub, cfg("DispResNet"), "depth").scales == 1
    assert Trainer.load_from_config(stub, cfg("DispResNetMS"), "depth").scales == 4
    for name in ("DispResNet50", "DispResNetMS"):           # no-argument classes: the key cannot apply
        with pytest.raises(ValueError, match="scales"):
            Trainer.load_from_config(stub, cfg(name, scales=4), "depth")
    with pytest.raises(ValueError, match="scales"):
        Trainer.load_from_config(stub, cfg("DispResNet", scales=7), "depth")


def test_loss_switches_are_plain_attributes():
    from losses import Losses
    c = Losses()
    assert c.multiscale_upsample == "depth" and c.fused_pyramid is False
    c = Losses(multiscale_upsample="disparity", fused_pyramid=True)
    assert c.multiscale_upsample == "disparity" and c.fused_pyramid is True
    with pytest.raises(ValueError, match="multiscale_upsample"):
        Losses(multiscale_upsample="nearest")


def test_multiscale_ref_equals_the_oracle_in_depth_order_and_differs_in_disparity_order():
    import multiscale_ref as mr
    from oracle import losses as ol
    from oracle.step import synthetic_batch
    B, H, W = 2, 32, 64
    s = synthetic_batch(B, H, W, seed=31)
    g = torch.Generator().manual_seed(32)
    dt = [torch.rand(B, 1, H >> k, W >> k, generator=g, dtype=torch.float64) for k in range(4)]
    dr = [torch.rand(B, 1, H >> k, W >> k, generator=g, dtype=torch.float64) for k in range(4)]
    poses = 0.01 * torch.randn(B, 2, 6, generator=g, dtype=torch.float64)
    tgt, refs, K = s["tgt"].double(), [r.double() for r in s["ref_imgs"]], s["intrinsics"].double()
    for ssim in (False, True):
        want = ol.losses_forward(tgt, refs, [dt, dr], poses, K, 0.85 if ssim else 0.0)
        got = mr.multiscale_losses(tgt, refs, [dt, dr], poses, K, "depth", ssim=ssim)
        assert abs(float(got[0]) - float(want[0])) < 1e-12 and float(got[1]) == float(want[1])
        other = mr.multiscale_losses(tgt, refs, [dt, dr], poses, K, "disparity", ssim=ssim)
        assert abs(float(other[0]) - float(want[0])) > 1e-6 and float(other[1]) == float(want[1])
    # scale 0 needs no resize: with one scale the two orders are one definition
    a = mr.multiscale_losses(tgt, refs, [dt[:1], dr[:1]], poses, K, "depth")
    b = mr.multiscale_losses(tgt, refs, [dt[:1], dr[:1]], poses, K, "disparity")
    assert float(a[0]) == float(b[0])
