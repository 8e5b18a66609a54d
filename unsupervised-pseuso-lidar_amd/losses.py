"""losses.py -- drop-in for the reference's losses.py on MI355X.

Same call surface (reference losses.py:12-54, 56-271): ``Losses().forward(tgt, ref_imgs, disparity, poses,
intrinsics, gt) -> [loss_mam, loss_smooth]`` with ``sum(loss).backward()`` working, and ``SSIM().standard_loss``.
The arithmetic runs in ONE fused HIP kernel (csrc/warp_loss.hip, mcav_warp_loss_fwd_bwd): disp->depth, the
three inverse warps per triplet (incl. the tgt->refs[1] warp with depth(ref0) and the inverted pose[0],
reference losses.py:203-207), bilinear sampling, L1 means, second-order smoothness, and the analytic backward
to both disparity maps and to the poses.  The kernel evaluates forward and backward together assuming unit
upstream gradients (what ``sum(loss).backward()`` supplies); a different upstream re-runs it with the real
weights, decided on the device without a host sync.
"""
import ctypes

import torch

from mcav import lib as L


class _WarpLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp_t, disp_r, poses, tgt, ref0, ref1, K, flags, term_weights, selection=None, stereo=None, baseline=None,
                grad_out=None):
        """grad_out: optional pair of preallocated tensors (shaped like disp_t, disp_r) that receive the gradients w.r.t. the two maps -- the
        depth pyramid's gradient buffer (mcav/multiscale.py), whose backward then reads them where they lie."""
        B, _, H, W = tgt.shape
        for n, t in (("tgt", tgt), ("ref0", ref0), ("ref1", ref1), ("disp_t", disp_t), ("disp_r", disp_r), ("poses", poses)):
            L.dev(t, n)
        if stereo is not None:              # mono + stereo: the fixed-baseline fourth warp (include/mcav_depth.h: mcav_warp_loss_stereo_fwd_bwd)
            L.dev(stereo, "stereo")
            L.dev(baseline, "stereo_baseline")
            if stereo.shape != tgt.shape or baseline.numel() != B or len(term_weights) != 4:
                raise L.MCAVError("stereo: the frame must be [B,3,H,W] like tgt, stereo_baseline [B], and there are 4 term weights")
        if K.dtype == torch.float64:
            flags |= L.WL_K_F64
        L.dev(K, "intrinsics", K.dtype)
        h = L.lib()
        ws = L.workspace(h.mcav_warp_loss_workspace_bytes(B, H, W), tgt.device, "warp_loss", zero=True)
        losses = torch.empty(2, dtype=torch.float32, device=tgt.device)
        if grad_out is not None:
            g_dt, g_dr = (L.dev(g, "grad_out") for g in grad_out)
            if g_dt.shape != disp_t.shape or g_dr.shape != disp_r.shape:
                raise L.MCAVError("grad_out: one tensor shaped like each depth map")
        else:
            g_dt = torch.empty_like(disp_t)
            g_dr = torch.empty_like(disp_r)
        g_p = torch.empty_like(poses)
        tw = (ctypes.c_float * len(term_weights))(*term_weights)
        args = [L.ptr(tgt), L.ptr(ref0), L.ptr(ref1), L.ptr(disp_t), L.ptr(disp_r), L.ptr(poses), L.ptr(K), B, H, W]
        tail = [tw, L.ptr(losses), L.ptr(g_dt), L.ptr(g_dr), L.ptr(g_p), L.ptr(ws), ws.numel(), L.stream()]
        from mcav import nn as N
        i0 = h.mcav_kernel_timer_count() if N.PROFILE_LOSS is not None else 0
        masked = (flags & (L.WL_MIN_REPROJ | L.WL_AUTOMASK)) != 0
        if stereo is not None:
            sel = [L.ptr(selection), selection.numel() if selection is not None else 0]
            L.check(h.mcav_warp_loss_stereo_fwd_bwd(*args, flags, None, *tail, *sel, L.ptr(stereo), L.ptr(baseline)),
                    "mcav_warp_loss_stereo_fwd_bwd")
        elif masked:        # min-reprojection / auto-masking: the same kernels' masked instantiations (include/mcav_depth.h)
            sel = [L.ptr(selection), selection.numel() if selection is not None else 0]
            L.check(h.mcav_warp_loss_masked_fwd_bwd(*args, flags, None, *tail, *sel), "mcav_warp_loss_masked_fwd_bwd")
        else:
            L.check(h.mcav_warp_loss_fwd_bwd(*args, flags, None, *tail), "mcav_warp_loss_fwd_bwd")
        if N.PROFILE_LOSS is not None:
            N.PROFILE_LOSS.append(("warp_loss", i0, h.mcav_kernel_timer_count()))       # ONE launch since round 3 (prepare / finalize folded in)
        st = None if stereo is None else [L.ptr(stereo), L.ptr(baseline)]
        ctx.rerun = (args, tail, flags, st, (tgt, ref0, ref1, disp_t, disp_r, poses, K, ws, losses, stereo, baseline))
        ctx.grads = (g_dt, g_dr, g_p)
        l0, l1 = losses.unbind(0)
        return l0, l1

    @staticmethod
    def backward(ctx, g0, g1):
        args, tail, flags, st, keep = ctx.rerun
        g_dt, g_dr, g_p = ctx.grads
        dev = g_dt.device
        if g0 is not None and g1 is not None:          # the usual case (sum(loss).backward()): ONE launch instead of a fill and two copies
            up = torch.stack([g0.reshape(()), g1.reshape(())]).to(dtype=torch.float32, device=dev)
        else:
            up = torch.zeros(2, dtype=torch.float32, device=dev)
            if g0 is not None:
                up[0:1].copy_(g0.reshape(1))
            if g1 is not None:
                up[1:2].copy_(g1.reshape(1))
        scratch = torch.empty(2, dtype=torch.float32, device=dev)
        tail = list(tail)
        tail[1] = L.ptr(scratch)        # loss values are not needed again
        # no-op on the device when upstream == (1, 1); otherwise recomputes the gradients with the real weights
        if st is not None:                                 # (as the masked entry: the re-run selects exactly as the first run did)
            L.check(L.lib().mcav_warp_loss_stereo_fwd_bwd(*args, flags | L.WL_SKIP_IF_UNIT, L.ptr(up), *tail, L.ptr(None), 0, *st),
                    "mcav_warp_loss_stereo_fwd_bwd(bwd)")
        elif flags & (L.WL_MIN_REPROJ | L.WL_AUTOMASK):      # (the re-run selects exactly as the first run did: same inputs, same code)
            L.check(L.lib().mcav_warp_loss_masked_fwd_bwd(*args, flags | L.WL_SKIP_IF_UNIT, L.ptr(up), *tail, L.ptr(None), 0),
                    "mcav_warp_loss_masked_fwd_bwd(bwd)")
        else:
            L.check(L.lib().mcav_warp_loss_fwd_bwd(*args, flags | L.WL_SKIP_IF_UNIT, L.ptr(up), *tail), "mcav_warp_loss_fwd_bwd(bwd)")
        return g_dt, g_dr, g_p, None, None, None, None, None, None, None, None, None, None


L.register({
    "mcav_geom_consistency_workspace_bytes": (L.c_sz, [L.c_i, L.c_i, L.c_i]),
    "mcav_geom_consistency_fwd": (L.c_i, [L.c_p] * 4 + [L.c_i, L.c_i, L.c_i, L.c_u, L.c_i, L.c_f, L.c_p, L.c_p, L.c_p, L.c_p, L.c_sz, L.c_p]),
    "mcav_geom_consistency_bwd": (L.c_i, [L.c_p] * 4 + [L.c_i, L.c_i, L.c_i, L.c_u, L.c_i, L.c_f, L.c_p, L.c_p, L.c_p, L.c_p, L.c_p, L.c_i,
                                          L.c_p, L.c_sz, L.c_p]),
})


class _GeomConsistencyFn(torch.autograd.Function):
    """SC-SfMLearner's depth geometry consistency between the two depth maps of a step (include/mcav_depth.h: mcav_geom_consistency_fwd /
    _bwd) -> weight * loss_gc.  The forward leaves its counts and sums on the device (`saved`); the backward reads them and autograd's
    upstream from there: no host sync, both capturable.  diff_out: optional [B,2,H,W] float tensor that receives the per-pixel diff."""

    @staticmethod
    def forward(ctx, disp_t, disp_r, poses, K, flags, min_valid, weight, diff_out=None):
        for n, t in (("disp_t", disp_t), ("disp_r", disp_r), ("poses", poses)):
            L.dev(t, n)
        L.dev(K, "intrinsics", K.dtype)
        if K.dtype == torch.float64:
            flags |= L.WL_K_F64
        B, C, H, W = disp_t.shape
        if C != 1 or disp_r.shape != disp_t.shape or tuple(poses.shape) != (B, 2, 6) or tuple(K.shape) != (B, 3, 3):
            raise L.MCAVError("geometry consistency expects two [B,1,H,W] maps, poses [B,2,6] and intrinsics [B,3,3]")
        if diff_out is not None:
            L.dev(diff_out, "consistency")
            if tuple(diff_out.shape) != (B, 2, H, W):
                raise L.MCAVError("geometry consistency: the diff planes are [B,2,H,W]")
        h = L.lib()
        dev = disp_t.device
        ws = L.workspace(max(h.mcav_geom_consistency_workspace_bytes(B, H, W), 1), dev, "geom_consistency")
        saved = torch.empty(4 + 24 * B, dtype=torch.float64, device=dev)
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        args = [L.ptr(disp_t), L.ptr(disp_r), L.ptr(poses), L.ptr(K), B, H, W, flags, int(min_valid), float(weight), L.ptr(saved)]
        L.check(h.mcav_geom_consistency_fwd(*args, L.ptr(loss), L.ptr(diff_out), L.ptr(ws), ws.numel(), L.stream()),
                "mcav_geom_consistency_fwd")
        ctx.keep = (args, (disp_t, disp_r, poses, K, saved))
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        args, (disp_t, disp_r, poses, K, saved) = ctx.keep
        h = L.lib()
        B, _, H, W = disp_t.shape
        up = g.reshape(1).to(torch.float32).contiguous()
        ws = L.workspace(max(h.mcav_geom_consistency_workspace_bytes(B, H, W), 1), disp_t.device, "geom_consistency")
        g_dt, g_dr, g_p = torch.empty_like(disp_t), torch.empty_like(disp_r), torch.empty_like(poses)
        L.check(h.mcav_geom_consistency_bwd(*args, L.ptr(up), L.ptr(g_dt), L.ptr(g_dr), L.ptr(g_p), 0, L.ptr(ws), ws.numel(), L.stream()),
                "mcav_geom_consistency_bwd")
        return g_dt, g_dr, g_p, None, None, None, None, None


STEREO_TERM_WEIGHTS = (1 / 6, 1 / 6, 0.5, 1 / 6)      # (tw0, tw1, tw2, tws): the target-view group is the mean of its three warps


class SSIM:
    """SSIM.standard_loss (reference losses.py:12-54) as a HIP kernel (3x3 box over reflection padding)."""

    def standard_loss(self, x, y, C1=1e-4, C2=9e-4, kernel_size=3, stride=1):
        if kernel_size != 3 or stride != 1:
            raise L.MCAVError("SSIM: only kernel_size=3, stride=1 (the reference's defaults) are implemented")
        x = L.dev(x.contiguous(), "x")
        y = L.dev(y.contiguous(), "y")
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        L.check(L.lib().mcav_ssim_fwd(L.ptr(x), L.ptr(y), B * C, H, W, C1, C2, L.ptr(out), L.stream()), "mcav_ssim_fwd")
        return out


class Losses:
    """`Losses()` is the reference's live loss (L1 photometric, losses.py:183-240).  `Losses(ssim=True)` -- or setting `.ssim` on an
    instance, which is what `loss: {ssim: true}` in a trainer config does -- switches the photometric term of every warp to
    0.85 * SSIM.standard_loss(warped, target) + 0.15 * |target - warped| (the mix of the reference's dormant
    compute_photometric_loss, losses.py:66-77, without its mean + 0.5 std clip), evaluated by the same fused kernel (MCAV_WL_SSIM).

    `min_reprojection` / `automask` (attributes as well; trainer config `loss: {min_reprojection: true, automask: true}`) combine the
    pixels of the photometric term as monodepth2 does, in the same fused kernel (MCAV_WL_MIN_REPROJ / MCAV_WL_AUTOMASK,
    include/mcav_depth.h): the two warps into the target view become one term, the per-pixel minimum of their errors; auto-masking takes
    the minimum with the identity (unwarped) errors as well, and a pixel an identity error wins sends no gradient.  Ties are deterministic
    (identity first, then warp 0).  With `keep_selection` the last forward's selection maps stay in `.selection`, one uint8 [B,2,H,W]
    tensor per scale (plane 0: warps 0 / 1 -> 0 / 1, identity 2; plane 1: warp 2 kept 0, identity 2).

    `edge_aware_smoothness` (attribute as well; trainer config `loss: {edge_aware_smoothness: true, edge_smoothness_weight: 1e-3}`) replaces
    the reference's second-order depth smoothness with monodepth2's term, `edge_aware_smooth_loss(disparities of tgt, tgt)`: first order, on
    disparity divided by its per-image mean, weighted down at image edges, `edge_smoothness_weight` (1e-3) / n_scales * 2^-s per scale
    (include/mcav_depth.h: mcav_edge_smooth_fwd).  loss_mam is what the same call gives without it.

    `stereo` (attribute as well; trainer config `loss: {stereo: true}`) is monodepth2's mono + stereo training: `forward(...,
    stereo=<[B,3,H,W] stereo frame of the target>, stereo_baseline=<[B] float32, metres>)` adds that frame as one more source view of the
    target, warped with depth(tgt) and the FIXED transform [I | (-b, 0, 0)] (include/mcav_depth.h: mcav_warp_loss_stereo_fwd_bwd).  It
    joins warps 0 and 1 -- in their per-pixel minimum under `min_reprojection`, with its own identity error under `automask` -- and its known
    metric baseline makes the learnt depth metric: what pseudo-LiDAR needs.  Term weights (1/6, 1/6, 1/6 and 1/2 for warp 2) / n_scales;
    selection code 3 = the stereo warp.  b is the x of the stereo camera's centre in the target camera's frame (KITTI left target: +0.54),
    negated for a mirrored sample.

    `multiscale_upsample` / `fused_pyramid` (attributes as well; trainer config `loss: {multiscale_upsample: depth|disparity, fused_pyramid:
    true}`) act when the depth net returns several scales (DispNetS, DispResNet(scales=n)): every coarse scale is evaluated at full
    resolution, as D_s = resize(1 / (10 d_s + 0.01)) ("depth", the reference's order, losses.py:212-216; the default) or as
    D_s = 1 / (10 resize(d_s) + 0.01) ("disparity", monodepth2's).  With `fused_pyramid` the coarse scales of both depth passes go through
    one forward and one backward launch (include/mcav_depth.h: mcav_depth_pyramid_fwd / _bwd) instead of a launch per scale, pass, operation
    and direction; the loss is the same."""

    def __init__(self, ssim=False, min_reprojection=False, automask=False, keep_selection=False, edge_aware_smoothness=False,
                 edge_smoothness_weight=1e-3, stereo=False, multiscale_upsample="depth", fused_pyramid=False,
                 geometry_consistency=False, geometry_consistency_weight=0.5, geometry_min_valid=100, keep_consistency=False):
        self.clip_loss = 0.5
        self.geometry_consistency = bool(geometry_consistency)
        self.geometry_consistency_weight = float(geometry_consistency_weight)
        self.geometry_min_valid = int(geometry_min_valid)
        self.keep_consistency = bool(keep_consistency)
        self.consistency = None
        self.stereo = bool(stereo)
        self.ssim = bool(ssim)
        self.min_reprojection = bool(min_reprojection)
        self.automask = bool(automask)
        self.keep_selection = bool(keep_selection)
        self.selection = None
        self.edge_aware_smoothness = bool(edge_aware_smoothness)
        self.edge_smoothness_weight = float(edge_smoothness_weight)
        if multiscale_upsample not in ("depth", "disparity"):
            raise ValueError("multiscale_upsample must be 'depth' or 'disparity', got %r" % (multiscale_upsample,))
        self.multiscale_upsample = multiscale_upsample
        self.fused_pyramid = bool(fused_pyramid)

    def _flags(self, n_scales):
        return L.WL_SSIM if self.ssim else 0

    def _mask_flags(self):
        return (L.WL_MIN_REPROJ if self.min_reprojection else 0) | (L.WL_AUTOMASK if self.automask else 0)

    def _selection(self, tgt):
        if not self.keep_selection:
            return None
        B, _, H, W = tgt.shape
        alloc = torch.empty if self._mask_flags() else torch.zeros      # (the plain loss keeps every warp: all zeros)
        return alloc((B, 2, H, W), dtype=torch.uint8, device=tgt.device)

    def _stereo_inputs(self, tgt_img, stereo, stereo_baseline):
        if not self.stereo:
            if stereo is not None or stereo_baseline is not None:
                raise L.MCAVError("stereo / stereo_baseline given to a Losses without .stereo: set Losses(stereo=True) (trainer config "
                                  "`loss: {stereo: true}`) for mono + stereo training, or pass neither")
            return None, None
        if stereo is None or stereo_baseline is None:
            raise L.MCAVError("Losses(stereo=True) needs the stereo frame and stereo_baseline (forward(..., stereo=, stereo_baseline=))")
        b = stereo_baseline
        if not torch.is_tensor(b):
            b = torch.as_tensor(b, dtype=torch.float32)
        b = b.to(device=tgt_img.device, dtype=torch.float32).reshape(-1).contiguous()
        return stereo.contiguous(), b

    def forward(self, tgt_img, ref_imgs, disparity, poses, intrinsics, gt=None, stereo=None, stereo_baseline=None):
        """-> [loss_mam, loss_smooth] (and the weighted geometry-consistency term when `.geometry_consistency` is set).  disparity =
        [disps(tgt), disps(ref0)], each a list over scales.  stereo / stereo_baseline: the stereo frame [B,3,H,W] and its baseline [B]
        (metres), used (and required) when `.stereo` is set."""
        out = self._forward(tgt_img, ref_imgs, disparity, poses, intrinsics, stereo, stereo_baseline)
        if self.geometry_consistency:
            if disparity[0][0].shape[-2:] != tgt_img.shape[-2:] or disparity[1][0].shape[-2:] != tgt_img.shape[-2:]:
                raise L.MCAVError("geometry consistency acts on scale 0 of both depth passes at the image's resolution (the intrinsics' own)")
            out = list(out) + [self.geometry_consistency_loss(disparity[0][0], disparity[1][0], poses, intrinsics)]
        return out

    def geometry_consistency_loss(self, disp_t, disp_r, poses, intrinsics, inputs_are_depth=False, lds_tile=False):
        """geometry_consistency_weight * loss_gc of two full-resolution [B,1,H,W] maps (sigmoid disparities, or depths with
        inputs_are_depth) under poses[:,0] and the intrinsics of that resolution.  lds_tile: the backward's scatter goes through an
        LDS tile (MCAV_GC_LDS_TILE) instead of four global adds per pixel: the same bits, another schedule (tools/geom_bench.py)."""
        diff = None
        if self.keep_consistency:
            B, _, H, W = disp_t.shape
            diff = torch.empty((B, 2, H, W), dtype=torch.float32, device=disp_t.device)
        loss = _GeomConsistencyFn.apply(disp_t.contiguous(), disp_r.contiguous(), poses.contiguous(), intrinsics.contiguous(),
                                        (L.WL_INPUT_DEPTH if inputs_are_depth else 0) | (L.GC_LDS_TILE if lds_tile else 0), self.geometry_min_valid,
                                        self.geometry_consistency_weight, diff)
        if diff is not None:
            self.consistency = diff
        return loss

    def _forward(self, tgt_img, ref_imgs, disparity, poses, intrinsics, stereo=None, stereo_baseline=None):
        st, sb = self._stereo_inputs(tgt_img, stereo, stereo_baseline)
        disp_t, disp_r = disparity[0], disparity[1]
        n = len(disp_t)
        ssim_flag = self._flags(max(n, len(disp_r)))
        mask_flags = self._mask_flags()
        if n != 1 or len(disp_r) != 1:
            from mcav.multiscale import multiscale_losses
            sel = [] if self.keep_selection else None
            out = multiscale_losses(tgt_img, ref_imgs, disparity, poses, intrinsics, ssim=self.ssim, min_reprojection=self.min_reprojection,
                                    automask=self.automask, selections=sel, edge_aware_smoothness=self.edge_aware_smoothness,
                                    edge_smoothness_weight=self.edge_smoothness_weight, stereo=st, stereo_baseline=sb,
                                    multiscale_upsample=self.multiscale_upsample, fused_pyramid=self.fused_pyramid)
            if sel is not None:
                self.selection = sel
            return out
        tw = (0.25, 0.25, 0.5)     # mean of the two tgt-view L1 terms and the third term, averaged (losses.py:227-240)
        if st is not None:
            tw = STEREO_TERM_WEIGHTS
        sel = self._selection(tgt_img)
        smooth_flag = L.WL_NO_SMOOTH if self.edge_aware_smoothness else 0
        l0, l1 = _WarpLossFn.apply(disp_t[0].contiguous(), disp_r[0].contiguous(), poses.contiguous(), tgt_img.contiguous(),
                                   ref_imgs[0].contiguous(), ref_imgs[1].contiguous(), intrinsics.contiguous(),
                                   ssim_flag | mask_flags | smooth_flag, tw, sel, st, sb)
        if sel is not None:
            self.selection = [sel]
        if self.edge_aware_smoothness:
            # l1 is exactly 0 under MCAV_WL_NO_SMOOTH; keeping it in the sum hands the fused kernel the usual upstream (1, 1) under
            # sum(loss).backward(), so its backward stays a no-op instead of a re-run with (1, 0)
            return [l0, l1 + self.edge_aware_smooth_loss(disp_t[0], tgt_img)]
        return [l0, l1]

    def edge_aware_smooth_loss(self, disp, img):
        """monodepth2's edge-aware smoothness of tgt's disparity (one [B,1,h,w] map or a list over scales) against the target image img
        [B,3,H,W] (H / h = W / w an integer; coarser scales see img box-averaged to their size): edge_smoothness_weight / n * sum_s 2^-s E_s."""
        from mcav.multiscale import edge_smooth_loss
        return edge_smooth_loss(disp, img, self.edge_smoothness_weight)

    def reprojection_loss(self, tgt, refs, depths, poses, intrinsics, mode='min'):
        """Reference signature (losses.py:183): takes DEPTHS (nested [time][scale])."""
        if mode != 'min':
            raise L.MCAVError("reprojection_loss: only mode='min' (the reference's live path) is implemented")
        ssim_flag = self._flags(len(depths[0]))
        if len(depths[0]) != 1:
            from mcav.multiscale import multiscale_losses
            return multiscale_losses(tgt, refs, depths, poses, intrinsics, inputs_are_depth=True, ssim=self.ssim)[0]
        tw = (0.25, 0.25, 0.5)
        l0, _ = _WarpLossFn.apply(depths[0][0].contiguous(), depths[1][0].contiguous(), poses.contiguous(), tgt.contiguous(),
                                  refs[0].contiguous(), refs[1].contiguous(), intrinsics.contiguous(),
                                  L.WL_INPUT_DEPTH | L.WL_NO_SMOOTH | ssim_flag, tw)
        return l0

    def smooth_loss(self, pred_map):
        from mcav.multiscale import smooth_loss
        return smooth_loss(pred_map)
