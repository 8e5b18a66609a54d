"""Test reference (CPU, float32 or float64) of the masked loss modes: per-pixel minimum reprojection and auto-masking
(include/mcav_depth.h: MCAV_WL_MIN_REPROJ / MCAV_WL_AUTOMASK).  A restatement of the definition, built on the oracle's pieces:

  err(X, T)(p)  = channel mean of |T - X|, or of 0.85 ssim_distance(X, T) + 0.15 |T - X| (ssim)
  e_w = err(warped source of warp w, T_w),  i_w = err(unwarped source S_w, T_w)   (warps of oracle.losses.warp_plan)
  min_reprojection:  warps 0 and 1 -> one term mean_p min(e_0, e_1) of weight tw[0] + tw[1]; warp 2 alone
  automask:          every term also takes the minimum with the identity errors of the warps it covers
  ties:              candidates are taken in the order identities (warp 0 first), then reprojections (warp 0 first); a later
                     candidate replaces the current choice only if it is strictly smaller

Gradients come from autograd: torch.where sends a pixel's gradient to the chosen candidate only (an identity error has none).
"""
import torch
import torch.nn.functional as F

from oracle.geometry import disp_to_depth, inverse_warp
from oracle.losses import smooth_loss, ssim_distance, warp_plan

IDENTITY = 2


def pixel_error(x, t, ssim):
    """[B,3,H,W] x2 -> [B,H,W]: the channel mean of the photometric error."""
    e = (t - x).abs()
    if ssim:
        e = 0.85 * ssim_distance(x, t) + 0.15 * e
    return e.mean(1)


def select(cands, codes):
    """Running minimum in tie order -> (value [B,H,W], code [B,H,W] int64, gap [B,H,W]): gap = the distance between the two smallest
    candidates relative to the larger of them (a near tie when small)."""
    m, code = cands[0], torch.full(cands[0].shape, codes[0], dtype=torch.int64)
    for c, k in zip(cands[1:], codes[1:]):
        take = c < m
        m = torch.where(take, c, m)
        code = torch.where(take, torch.full_like(code, k), code)
    if len(cands) > 1:
        v = torch.stack([c.detach() for c in cands]).sort(0).values
        gap = (v[1] - v[0]) / v[1].abs().clamp_min(1e-30)
    else:
        gap = torch.full(m.shape, float("inf"), dtype=m.dtype)
    return m, code, gap


def masked_losses(tgt, refs, disparity, poses, K, ssim=False, min_reprojection=False, automask=False, inputs_are_depth=False):
    """-> ([loss_mam, loss_smooth], [selection [B,2,H,W] int64 per scale], [near-tie gap [B,2,H,W] per scale]).
    disparity = [disps(tgt), disps(ref0)], each a list over scales (coarser scales are resized to the image size as the oracle does);
    term weights as the fused kernel's callers use them: (0.25, 0.25, 0.5) for one scale, every term / (2 n) for n scales."""
    depths = disparity if inputs_are_depth else disp_to_depth(disparity)
    plan = warp_plan(tgt, refs, depths, poses)
    n = len(depths[0])
    B, _, H, W = tgt.shape
    tw = (0.5 / (2 * n), 0.5 / (2 * n), 1.0 / (2 * n))
    total, sels, gaps = 0, [], []
    for s in range(n):
        e, i = [], []
        for w in plan:
            D = w["depth"][s]
            if D.shape[-1] != W:
                D = F.interpolate(D, [H, W], mode="bilinear", align_corners=False)
            e.append(pixel_error(inverse_warp(w["src"], D[:, 0], w["pose"], K, w["inv"]), w["target"], ssim))
            i.append(pixel_error(w["src"], w["target"], ssim))
        sel = torch.zeros(B, 2, H, W, dtype=torch.int64)
        gap = torch.full((B, 2, H, W), float("inf"), dtype=tgt.dtype)
        groups = [((0, 1), 0), ((2,), 1)] if min_reprojection else [((0,), 0), ((1,), None), ((2,), 1)]
        for ws, plane in groups:
            cands = ([i[w] for w in ws] if automask else []) + [e[w] for w in ws]
            codes = ([IDENTITY] * len(ws) if automask else []) + (list(range(len(ws))) if len(ws) > 1 else [0])
            m, code, g = select(cands, codes)
            total = total + sum(tw[w] for w in ws) * m.mean()
            if plane is not None:
                sel[:, plane], gap[:, plane] = code, g
        sels.append(sel)
        gaps.append(gap)
    return [total, smooth_loss(depths[0])], sels, gaps


def run(tgt, refs, disp_t, disp_r, poses, K, dtype=torch.float64, upstream=(1.0, 1.0), **modes):
    """One evaluation in `dtype` with autograd -> (losses (2 floats), (d disp_t, d disp_r, d poses), selections, gaps).
    disp_t / disp_r: tensors (one scale) or lists of tensors (several scales)."""
    multi = isinstance(disp_t, (list, tuple))
    dts = [d.detach().to(dtype).clone().requires_grad_() for d in (disp_t if multi else [disp_t])]
    drs = [d.detach().to(dtype).clone().requires_grad_() for d in (disp_r if multi else [disp_r])]
    p = poses.detach().to(dtype).clone().requires_grad_()
    out, sels, gaps = masked_losses(tgt.to(dtype), [r.to(dtype) for r in refs], [dts, drs], p, K, **modes)
    (upstream[0] * out[0] + upstream[1] * out[1]).backward()
    gt = [d.grad for d in dts]
    gr = [d.grad for d in drs]
    return ([float(out[0].detach()), float(out[1].detach())], (gt if multi else gt[0], gr if multi else gr[0], p.grad), sels, gaps)
