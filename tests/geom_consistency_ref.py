"""Test reference (CPU, float64, stock torch ops, differentiable by autograd) of the depth geometry-consistency term -- the FROZEN
definition of include/mcav_depth.h: mcav_geom_consistency_fwd / _bwd (SC-SfMLearner, Bian et al., NeurIPS 2019: compute_pairwise_loss and
mean_on_mask).

Two directions, the geometries of the fused loss kernel's warps 0 and 2:
  d = 0:  a = tgt,  b = ref0,  [R|t] = pose_to_Rt(pose[:,0], invert=false)
  d = 1:  a = ref0, b = tgt,   [R|t] = its rigid inverse
For each pixel p = (x, y) of a with depth D_a(p):
  c        = P [K^-1 [x y 1]^T D_a ; 1],  P = K [R|t]
  (ix, iy) = csrc/warp_math.h's sampling position: pix = c[:2] / (c2 + 1e-5); g = (pix / (size-1) - 0.5) * 2; i = ((g + 1) / 2) * (size-1)
  D_proj   = c2,  D_samp = the bilinear sample of D_b at (ix, iy), zero padding, align_corners=True
  valid    = 0 <= ix <= W-1 and 0 <= iy <= H-1 and D_proj >= 1e-3     (NaN: not valid)
  diff     = |D_proj - D_samp| / (D_proj + D_samp)                      (torch's |.|' at 0 is 0)
  n_d      = number of valid pixels over batch and image;  E_d = sum(valid * diff) / n_d if n_d > min_valid, else 0 with zero gradients
  loss_gc  = 0.5 * (E_0 + E_1)
Differences from SC-SfMLearner: it clamps D_proj at 1e-3 where this definition drops the pixel (a clamped pixel has no gradient through
D_proj either); its mean_on_mask is min_valid = 100.  The count carries no gradient.  Depths are D = 1 / (10 disp + 0.01) unless given.

The term is only piecewise smooth: `flagged` names the pixels within TIE of a validity border, a bilinear cell edge or D_proj = D_samp,
where a float32 evaluation may legitimately land on the other side, and `touched` the texels of D_b such a pixel's taps can reach.
"""
import torch
import torch.nn.functional as F

from oracle import geometry as G

MIN_DEPTH = 1e-3
TIE = 1e-3


def direction(Da, Db, pose, K, invert, min_valid, ties=True):
    """Da, Db: [B,1,H,W] depths; pose: [B,6]; K: [B,3,3].  -> dict(E, n, S, diff [B,H,W] (-1 invalid), valid, flagged, touched).
    ties=False: E only, without the tie bookkeeping (tensor ops on the inputs' device, no host synchronisation)."""
    B, _, H, W = Da.shape
    T = G.pose_to_matrix(pose, invert=invert)
    P = K @ T[:, :3, :]
    X = G.reconstruct(Da[:, 0], K).reshape(B, 3, -1)
    c = P[:, :, :3] @ X + P[:, :, 3:]
    z = c[:, 2] + 1e-5
    gx = (c[:, 0] / z / (W - 1) - 0.5) * 2
    gy = (c[:, 1] / z / (H - 1) - 0.5) * 2
    ix = ((gx + 1) / 2) * (W - 1)
    iy = ((gy + 1) / 2) * (H - 1)
    Dp = c[:, 2].reshape(B, H, W)
    grid = torch.stack([gx, gy], -1).reshape(B, H, W, 2)
    Ds = F.grid_sample(Db, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
    ixd, iyd = ix.detach().reshape(B, H, W), iy.detach().reshape(B, H, W)
    valid = (ixd >= 0) & (ixd <= W - 1) & (iyd >= 0) & (iyd <= H - 1) & (Dp.detach() >= MIN_DEPTH)
    den = torch.where(valid, Dp + Ds, torch.ones_like(Dp))
    diff = torch.where(valid, (Dp - Ds).abs() / den, torch.zeros_like(Dp))
    n = valid.sum()
    S = diff.sum()
    E = torch.where(n > min_valid, S / n.clamp(min=1), S * 0.0)      # (the branch not taken gets no gradient: zero below min_valid)
    if not ties:
        return dict(E=E)
    n = int(n)
    # ---- the pixels a float32 evaluation may decide differently
    with torch.no_grad():
        loose = (ixd >= -TIE) & (ixd <= W - 1 + TIE) & (iyd >= -TIE) & (iyd <= H - 1 + TIE) & (Dp >= MIN_DEPTH - TIE)
        border = ((ixd.abs() < TIE) | ((ixd - (W - 1)).abs() < TIE) | (iyd.abs() < TIE) | ((iyd - (H - 1)).abs() < TIE) |
                  ((Dp - MIN_DEPTH).abs() < TIE))
        cell = ((ixd - ixd.round()).abs() < TIE) | ((iyd - iyd.round()).abs() < TIE)
        equal = (Dp - Ds).abs() < TIE
        flagged = loose & (border | cell | equal)
        border = loose & border                            # the ties that change the valid SET (the others move the loss continuously)
        touched = torch.zeros(B, H, W, dtype=torch.bool)
        bb, yy, xx = torch.nonzero(flagged, as_tuple=True)
        if len(bb):
            x0 = ixd[bb, yy, xx].floor().long()
            y0 = iyd[bb, yy, xx].floor().long()
            for dy in (-1, 0, 1, 2):
                for dx in (-1, 0, 1, 2):
                    ty, tx = y0 + dy, x0 + dx
                    ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
                    touched[bb[ok], ty[ok], tx[ok]] = True
    out = torch.where(valid, diff.detach(), -torch.ones_like(Dp))
    return dict(E=E, n=n, S=float(S.detach()), diff=out, valid=valid, flagged=flagged, border=border, touched=touched)


def geom_consistency(disp_t, disp_r, poses, K, min_valid=100, inputs_are_depth=False, ties=True):
    """-> (loss_gc (0-dim tensor, differentiable), [direction 0, direction 1])"""
    Dt = disp_t if inputs_are_depth else 1 / (10 * disp_t + 0.01)
    Dr = disp_r if inputs_are_depth else 1 / (10 * disp_r + 0.01)
    K = K.to(Dt.dtype)
    d0 = direction(Dt, Dr, poses[:, 0], K, False, min_valid, ties)
    d1 = direction(Dr, Dt, poses[:, 0], K, True, min_valid, ties)
    return 0.5 * (d0["E"] + d1["E"]), [d0, d1]


def run(disp_t, disp_r, poses, K, min_valid=100, weight=1.0, upstream=1.0, inputs_are_depth=False, dtype=torch.float64):
    """Evaluate in dtype with autograd.  -> dict: loss (weight * loss_gc), d_disp_t, d_disp_r, d_poses (of upstream * weight * loss_gc),
    n [2], diff [B,2,H,W], flagged [B,2,H,W] (plane d: pixels of direction d's frame a), touched [B,2,H,W] (plane 0: texels of tgt that a
    flagged pixel of direction 1 reaches, plane 1: texels of ref0 reached from direction 0), flagged_share, border [2] (the number of
    pixels per direction within TIE of a validity border: only these can change n_d)."""
    dt = disp_t.detach().to(dtype).clone().requires_grad_()
    dr = disp_r.detach().to(dtype).clone().requires_grad_()
    p = poses.detach().to(dtype).clone().requires_grad_()
    loss, (d0, d1) = geom_consistency(dt, dr, p, K.detach().to(dtype), min_valid, inputs_are_depth)
    (upstream * weight * loss).backward()
    flagged = torch.stack([d0["flagged"], d1["flagged"]], 1)
    return dict(loss=weight * float(loss.detach()), d_disp_t=dt.grad, d_disp_r=dr.grad, d_poses=p.grad, n=[d0["n"], d1["n"]],
                diff=torch.stack([d0["diff"], d1["diff"]], 1), flagged=flagged,
                border=[int(d0["border"].sum()), int(d1["border"].sum())],
                touched=torch.stack([d1["touched"], d0["touched"]], 1),
                flagged_share=float(flagged.double().mean()), valid_share=float(torch.stack([d0["valid"], d1["valid"]]).double().mean()))


def composition(disp_t, disp_r, poses, K, min_valid=100):
    """The same definition on whatever device and dtype the inputs have (tools/geom_bench.py's stock-torch baseline)."""
    return geom_consistency(disp_t, disp_r, poses, K, min_valid, ties=False)[0]


# ---------------------------------------------------------------------------------------------- the inputs the CPU and GPU tests share
def intrinsics(B, H, W):
    """K = [[0.58 W, 0, (W-1)/2], [0, 1.92 H, (H-1)/2], [0, 0, 1]], rounded to float32 (what the kernel reads), as float64."""
    K = torch.tensor([[0.58 * W, 0.0, (W - 1) / 2], [0.0, 1.92 * H, (H - 1) / 2], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return K.float().double().repeat(B, 1, 1)


def smooth_disparity(B, H, W, g):
    """Smooth random disparities in [0.05, 0.6]: a coarse uniform field, bilinearly enlarged."""
    u = torch.rand(B, 1, max(H // 6, 2), max(W // 6, 2), generator=g, dtype=torch.float64)
    u = F.interpolate(u, size=(H, W), mode="bilinear", align_corners=True).clamp(0, 1)
    return (0.05 + 0.55 * u).float().double()


def inputs(B, H, W, seed, rot=0.02, trans=0.15, forward=0.0):
    """-> disp_t, disp_r [B,1,H,W], poses [B,2,6], K [B,3,3]: float64 tensors holding float32 values.  Rotations up to `rot` rad per axis,
    translations up to `trans`; forward: added to t_z of pose[:,0] (the many-to-one case)."""
    g = torch.Generator().manual_seed(seed)
    dt, dr = smooth_disparity(B, H, W, g), smooth_disparity(B, H, W, g)
    poses = torch.rand(B, 2, 6, generator=g, dtype=torch.float64) * 2 - 1
    poses[..., :3] *= rot
    poses[..., 3:] *= trans
    poses[:, 0, 5] += forward
    return dt, dr, poses.float().double(), intrinsics(B, H, W)
