"""TEST INFRASTRUCTURE (CPU, float32 or float64): the definition of the multi-scale loss in both upsampling orders, and the multi-scale
depth network, built from the oracle's pieces.

  depth order (the reference, losses.py:212-216):  D_s = interpolate(1 / (10 d_s + 0.01))
  disparity order (monodepth2):                    D_s = 1 / (10 interpolate(d_s) + 0.01)
  photometric term of scale s: the single-scale term on the full-resolution D_s, every term / (2 n) (oracle.losses.reprojection_loss; the
  masked modes through tests/minreproj_ref.py); smoothness on the native-resolution depths of tgt (oracle.losses.smooth_loss).
"""
import torch
import torch.nn.functional as F

from oracle import losses as ol
from oracle.geometry import disp_to_depth


def full_resolution_depths(disparity, H, W, order="depth"):
    """[time][scale] disparities -> [time][scale] depths at H x W."""
    if order not in ("depth", "disparity"):
        raise ValueError(order)
    up = lambda t: t if t.shape[-2:] == (H, W) else F.interpolate(t, [H, W], mode="bilinear", align_corners=False)
    to_depth = lambda d: 1 / (10 * d + 0.01)
    if order == "depth":
        return [[up(to_depth(d)) for d in per_time] for per_time in disparity]
    return [[to_depth(up(d)) for d in per_time] for per_time in disparity]


def multiscale_losses(tgt, refs, disparity, poses, K, order="depth", ssim=False, min_reprojection=False, automask=False):
    """-> [loss_mam, loss_smooth]; disparity = [disps(tgt), disps(ref0)], each a list over scales."""
    H, W = tgt.shape[-2:]
    full = full_resolution_depths(disparity, H, W, order)
    if min_reprojection or automask:
        from minreproj_ref import masked_losses
        mam = masked_losses(tgt, refs, full, poses, K, ssim=ssim, min_reprojection=min_reprojection, automask=automask,
                            inputs_are_depth=True)[0][0]
    else:
        mam = ol.reprojection_loss(tgt, refs, full, poses, K, 0.85 if ssim else 0.0)
    return [mam, ol.smooth_loss(disp_to_depth(disparity)[0])]


def run(tgt, refs, disp_t, disp_r, poses, K, dtype=torch.float32, **modes):
    """One evaluation in `dtype` with autograd -> (losses (2 floats), d disp_t (list), d disp_r (list), d poses)."""
    dts = [d.detach().to(dtype).clone().requires_grad_() for d in disp_t]
    drs = [d.detach().to(dtype).clone().requires_grad_() for d in disp_r]
    p = poses.detach().to(dtype).clone().requires_grad_()
    out = multiscale_losses(tgt.to(dtype), [r.to(dtype) for r in refs], [dts, drs], p, K, **modes)      # (K stays float64, as the kernels take it)
    sum(out).backward()
    return [float(o.detach()) for o in out], [d.grad for d in dts], [d.grad for d in drs], p.grad


def dispresnet_scales(net, x, scales=4):
    """oracle.nets.DispResNet's encoder and decoder called directly: the disparities of scales 0 .. scales-1 (the oracle's forward
    returns scale 0 only, as the reference does; its decoder computes all four)."""
    out = net.decoder(net.encoder(x))
    return [out[("disp", s)] for s in range(scales)]
