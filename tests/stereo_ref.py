"""Test reference (CPU, float32 or float64) of the mono + stereo loss (include/mcav_depth.h: mcav_warp_loss_stereo_fwd_bwd), a restatement
of its definition built on the oracle's pieces and on minreproj_ref:

  warp s         the stereo frame warped into tgt with depth(tgt), the same K and the fixed pose (0, 0, 0, -b, 0, 0): rotation exactly I,
                 translation (-b, 0, 0); b = x of the stereo camera's centre in the target camera's frame (metres).  No pose gradient.
  e_s, i_s       err(warped stereo, tgt), err(stereo, tgt)
  plain          tw0 mean e_0 + tw1 mean e_1 + tws mean e_s + tw2 mean e_2
  min_reprojection   (tw0 + tw1 + tws) mean_p min(e_0, e_1, e_s); warp 2 alone
  automask       every term also takes the minimum with the identity errors of the warps it covers
  ties           identities (i_0, i_1, i_s), then reprojections (e_0, e_1, e_s); a later candidate wins only if strictly smaller
  selection      plane 0 code 3 = the stereo warp

Term weights (1/6, 1/6, 1/2, 1/6) for one scale, every weight / n for n scales.
"""
import torch
import torch.nn.functional as F

import minreproj_ref as M
from oracle.geometry import disp_to_depth, inverse_warp
from oracle.losses import smooth_loss, warp_plan

STEREO = 3
IDENTITY = M.IDENTITY
TERM_WEIGHTS = (1 / 6, 1 / 6, 0.5, 1 / 6)


def stereo_pose(baseline):
    """[B] -> the [B,6] pose (axis-angle, translation) of the fixed stereo transform [I | (-b, 0, 0)]."""
    b = torch.as_tensor(baseline)
    p = torch.zeros(b.shape[0], 6, dtype=b.dtype)
    p[:, 3] = -b
    return p


def stereo_losses(tgt, refs, stereo, baseline, disparity, poses, K, ssim=False, min_reprojection=False, automask=False,
                  inputs_are_depth=False, term_weights=None):
    """-> ([loss_mam, loss_smooth], [selection [B,2,H,W] int64 per scale], [near-tie gap [B,2,H,W] per scale])."""
    depths = disparity if inputs_are_depth else disp_to_depth(disparity)
    plan = warp_plan(tgt, refs, depths, poses)
    plan.append(dict(group=0, src=stereo, target=tgt, depth=depths[0], pose=stereo_pose(baseline).to(tgt.dtype), inv=False))
    n = len(depths[0])
    B, _, H, W = tgt.shape
    tw = [w / n for w in (term_weights or TERM_WEIGHTS)]
    tw = [tw[0], tw[1], tw[2], tw[3]]                     # indexed by plan position: 0, 1, 2, 3 = stereo
    total, sels, gaps = 0, [], []
    for s in range(n):
        e, i = [], []
        for w in plan:
            D = w["depth"][s]
            if D.shape[-1] != W:
                D = F.interpolate(D, [H, W], mode="bilinear", align_corners=False)
            e.append(M.pixel_error(inverse_warp(w["src"], D[:, 0], w["pose"], K, w["inv"]), w["target"], ssim))
            i.append(M.pixel_error(w["src"], w["target"], ssim))
        sel = torch.zeros(B, 2, H, W, dtype=torch.int64)
        gap = torch.full((B, 2, H, W), float("inf"), dtype=tgt.dtype)
        if min_reprojection:
            groups = [((0, 1, 3), 0), ((2,), 1)]
        else:
            groups = [((0,), 0), ((1,), None), ((3,), None), ((2,), 1)]
        for ws, plane in groups:
            cands = ([i[w] for w in ws] if automask else []) + [e[w] for w in ws]
            codes = ([IDENTITY] * len(ws) if automask else []) + ([(STEREO if w == 3 else w) for w in ws] if len(ws) > 1 else [0])
            m, code, g = M.select(cands, codes)
            total = total + sum(tw[w] for w in ws) * m.mean()
            if plane is not None:
                sel[:, plane], gap[:, plane] = code, g
        sels.append(sel)
        gaps.append(gap)
    return [total, smooth_loss(depths[0])], sels, gaps


def run(tgt, refs, stereo, baseline, disp_t, disp_r, poses, K, dtype=torch.float64, upstream=(1.0, 1.0), **modes):
    """One evaluation in `dtype` with autograd -> (losses (2 floats), (d disp_t, d disp_r, d poses), selections, gaps)."""
    multi = isinstance(disp_t, (list, tuple))
    dts = [d.detach().to(dtype).clone().requires_grad_() for d in (disp_t if multi else [disp_t])]
    drs = [d.detach().to(dtype).clone().requires_grad_() for d in (disp_r if multi else [disp_r])]
    p = poses.detach().to(dtype).clone().requires_grad_()
    out, sels, gaps = stereo_losses(tgt.to(dtype), [r.to(dtype) for r in refs], stereo.to(dtype), torch.as_tensor(baseline).to(dtype),
                                    [dts, drs], p, K, **modes)
    (upstream[0] * out[0] + upstream[1] * out[1]).backward()
    gt = [d.grad for d in dts]
    gr = [d.grad for d in drs]
    return ([float(out[0].detach()), float(out[1].detach())], (gt if multi else gt[0], gr if multi else gr[0], p.grad), sels, gaps)
