"""Test reference (CPU, float64 or float32) of the edge-aware smoothness on mean-normalised disparity (include/mcav_depth.h:
mcav_edge_smooth_fwd; monodepth2's get_smooth_loss(disp / (mean_disp + 1e-7), color)).  A restatement of the definition in torch ops:

  I_s   = the f x f box average of the image (f = H / h = W / w; f = 1: the image)
  m_b   = mean of d_b,  n = d_b / (m_b + 1e-7)
  wx    = exp(-mean_c |I_s(x) - I_s(x+1)|),  wy likewise
  E     = mean over the x-pairs of |n(x) - n(x+1)| wx  +  mean over the y-pairs of |n(y) - n(y+1)| wy   (a direction without pairs: 0)
  multi-scale:  weight / n_scales * sum_s 2^-s E_s(d_s, image)

Gradients come from autograd (torch's |.|' at 0 is 0).  full_losses puts it next to the photometric part of tests/minreproj_ref.py, which is
built on the oracle's warp, so a Losses(edge_aware_smoothness=True) call has one float64 counterpart.
"""
import torch
import torch.nn.functional as F

import minreproj_ref as MR

EPS = 1e-7


def box(img, h, w):
    H, W = img.shape[-2:]
    if H % h or W % w or H // h != W // w:
        raise ValueError("image %dx%d is not an integer multiple f x f of %dx%d" % (H, W, h, w))
    f = H // h
    return img if f == 1 else F.avg_pool2d(img, f)


def edge_smooth(disp, img):
    """One scale: disp [B,1,h,w], img [B,3,H,W] -> E (0-dim tensor)."""
    B, _, h, w = disp.shape
    I = box(img, h, w)
    n = disp / (disp.mean((1, 2, 3), keepdim=True) + EPS)
    E = (disp * 0).sum()                     # 0, with a gradient of 0 where no direction has pairs
    if w > 1:
        wx = torch.exp(-(I[..., :, :-1] - I[..., :, 1:]).abs().mean(1, keepdim=True))
        E = E + ((n[..., :, :-1] - n[..., :, 1:]).abs() * wx).mean()
    if h > 1:
        wy = torch.exp(-(I[..., :-1, :] - I[..., 1:, :]).abs().mean(1, keepdim=True))
        E = E + ((n[..., :-1, :] - n[..., 1:, :]).abs() * wy).mean()
    return E


def edge_smooth_scales(disps, img, weight=1e-3):
    """The Losses term: weight / n * sum_s 2^-s E_s."""
    if torch.is_tensor(disps):
        disps = [disps]
    n = len(disps)
    return sum(weight / n * 2.0 ** -s * edge_smooth(d, img) for s, d in enumerate(disps))


def run(disps, img, dtype=torch.float64, weight=1e-3, upstream=1.0):
    """-> (loss float, [d loss / d disp_s]) evaluated in dtype with autograd; disps: one tensor or a list."""
    multi = isinstance(disps, (list, tuple))
    ds = [d.detach().to(dtype).clone().requires_grad_() for d in (disps if multi else [disps])]
    E = edge_smooth_scales(ds, img.detach().to(dtype), weight)
    (upstream * E).backward()
    g = [d.grad for d in ds]
    return float(E.detach()), (g if multi else g[0])


def closed_form_grad(disp, img):
    """dE/dd from the closed form of include/mcav_depth.h: dR/dd / (m + eps) - R / ((m + eps)^2 h w), per sample, with the stencil written
    out pair by pair (not by autograd)."""
    B, _, h, w = disp.shape
    I = box(img, h, w)
    d = disp.detach()
    g = torch.zeros_like(d)
    R = torch.zeros(B, dtype=d.dtype)
    if w > 1:
        wx = torch.exp(-(I[..., :, :-1] - I[..., :, 1:]).abs().mean(1, keepdim=True)) / (B * h * (w - 1))
        dx = d[..., :, :-1] - d[..., :, 1:]
        R += (dx.abs() * wx).sum((1, 2, 3))
        g[..., :, :-1] += dx.sign() * wx
        g[..., :, 1:] -= dx.sign() * wx
    if h > 1:
        wy = torch.exp(-(I[..., :-1, :] - I[..., 1:, :]).abs().mean(1, keepdim=True)) / (B * (h - 1) * w)
        dy = d[..., :-1, :] - d[..., 1:, :]
        R += (dy.abs() * wy).sum((1, 2, 3))
        g[..., :-1, :] += dy.sign() * wy
        g[..., 1:, :] -= dy.sign() * wy
    me = (d.mean((1, 2, 3)) + EPS).reshape(B, 1, 1, 1)
    return g / me - R.reshape(B, 1, 1, 1) / (me * me * h * w), float((R / me.reshape(B)).sum())


def full_losses(tgt, refs, disp_t, disp_r, poses, K, dtype=torch.float64, weight=1e-3, upstream=(1.0, 1.0), **modes):
    """Losses(edge_aware_smoothness=True, **modes).forward in dtype: loss_mam from tests/minreproj_ref.py (the oracle's warp), loss_smooth
    the edge-aware term of tgt's disparities.  -> (losses (2 floats), (d disp_t, d disp_r, d poses))."""
    multi = isinstance(disp_t, (list, tuple))
    dts = [d.detach().to(dtype).clone().requires_grad_() for d in (disp_t if multi else [disp_t])]
    drs = [d.detach().to(dtype).clone().requires_grad_() for d in (disp_r if multi else [disp_r])]
    p = poses.detach().to(dtype).clone().requires_grad_()
    (mam, _), _, _ = MR.masked_losses(tgt.to(dtype), [r.to(dtype) for r in refs], [dts, drs], p, K, **modes)
    sm = edge_smooth_scales(dts, tgt.to(dtype), weight)
    (upstream[0] * mam + upstream[1] * sm).backward()
    gt = [d.grad for d in dts]
    gr = [d.grad for d in drs]
    return [float(mam.detach()), float(sm.detach())], (gt if multi else gt[0], gr if multi else gr[0], p.grad)
