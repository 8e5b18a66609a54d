"""Loss-stage pieces that are not the fused single-scale kernel: standalone smoothness, multi-scale nets.

smooth_loss: Losses.smooth_loss (reference losses.py:242-260) for a list of depth scales, weight /2.3 per scale.
edge_smooth_loss: monodepth2's edge-aware smoothness on mean-normalised disparity (Losses(edge_aware_smoothness=True)).
multiscale_losses: Losses.forward for depth nets that return several scales (DispNetS): every coarser depth is
bilinearly resized to full resolution before warping (losses.py:212-216); smoothness stays at native resolution.
"""
import torch

from . import lib as L


class _SmoothFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *maps):
        h = L.lib()
        dev = maps[0].device
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        weight = 1.0
        ctx.maps = maps
        for D in maps:
            L.dev(D, "depth")
            B, C, H, W = D.shape
            if C != 1:
                raise L.MCAVError("smooth_loss expects [B,1,H,W] maps")
            ws = L.workspace(h.mcav_smooth_workspace_bytes(B, H, W), dev, "smooth")
            scratch = torch.empty_like(D)
            L.check(h.mcav_smooth_loss_fwd_bwd(L.ptr(D), B, H, W, weight, None, L.ptr(loss), L.ptr(scratch), 0, L.ptr(ws), ws.numel(),
                                               L.stream()), "mcav_smooth_loss_fwd_bwd")
            weight /= 2.3
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        h = L.lib()
        dev = g.device
        up = g.reshape(1).to(torch.float32).contiguous()
        dummy = torch.zeros(1, dtype=torch.float32, device=dev)
        grads = []
        weight = 1.0
        for D in ctx.maps:
            B, _, H, W = D.shape
            ws = L.workspace(h.mcav_smooth_workspace_bytes(B, H, W), dev, "smooth")
            gD = torch.empty_like(D)
            L.check(h.mcav_smooth_loss_fwd_bwd(L.ptr(D), B, H, W, weight, L.ptr(up), L.ptr(dummy), L.ptr(gD), 0, L.ptr(ws), ws.numel(),
                                               L.stream()), "mcav_smooth_loss_fwd_bwd")
            grads.append(gD)
            weight /= 2.3
        return tuple(grads)


def smooth_loss(pred_map):
    if not isinstance(pred_map, (tuple, list)):
        pred_map = [pred_map]
    return _SmoothFn.apply(*[m.contiguous() for m in pred_map])


class _EdgeSmoothFn(torch.autograd.Function):
    """monodepth2's edge-aware smoothness on mean-normalised disparity (include/mcav_depth.h: mcav_edge_smooth_fwd / _bwd), summed over
    scales with the given weights.  Forward: one launch per scale into one accumulator; the per-sample sums each launch saves feed its
    backward, which reads autograd's upstream from the device (no host sync: capturable)."""

    @staticmethod
    def forward(ctx, img, weights, *maps):
        h = L.lib()
        L.dev(img, "image")
        B, C, H, W = img.shape
        if C != 3:
            raise L.MCAVError("edge-aware smoothness expects a [B,3,H,W] image")
        dev = img.device
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        saved = []
        for D, wt in zip(maps, weights):
            L.dev(D, "disparity")
            if D.dim() != 4 or D.shape[0] != B or D.shape[1] != 1:
                raise L.MCAVError("edge-aware smoothness expects [B,1,h,w] disparities of the image's batch")
            hh, ww = D.shape[-2:]
            ws = L.workspace(max(h.mcav_edge_smooth_workspace_bytes(B, hh, ww), 1), dev, "edge_smooth", zero=True)
            sv = torch.empty(2 * B, dtype=torch.float64, device=dev)
            L.check(h.mcav_edge_smooth_fwd(L.ptr(D), L.ptr(img), B, H, W, hh, ww, wt, L.ptr(sv), L.ptr(loss), L.ptr(ws), ws.numel(),
                                           L.stream()), "mcav_edge_smooth_fwd")
            saved.append(sv)
        ctx.keep = (img, maps, weights, saved)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        h = L.lib()
        img, maps, weights, saved = ctx.keep
        B, _, H, W = img.shape
        up = g.reshape(1).to(torch.float32).contiguous()
        grads = []
        for D, wt, sv in zip(maps, weights, saved):
            hh, ww = D.shape[-2:]
            gD = torch.empty_like(D)
            L.check(h.mcav_edge_smooth_bwd(L.ptr(D), L.ptr(img), B, H, W, hh, ww, wt, L.ptr(sv), L.ptr(up), L.ptr(gD), 0, L.stream()),
                    "mcav_edge_smooth_bwd")
            grads.append(gD)
        return (None, None, *grads)


def edge_smooth_loss(disp, img, weight=1e-3):
    """Edge-aware smoothness of one disparity map or a list over scales (monodepth2): weight / n * sum_s 2^-s E_s(disp_s, img box-averaged
    to scale s's size).  disp: sigmoid disparities [B,1,h,w] (not depths); img: the target image [B,3,H,W], H / h = W / w an integer."""
    if not isinstance(disp, (tuple, list)):
        disp = [disp]
    n = len(disp)
    weights = tuple(float(weight) / n * 2.0 ** -s for s in range(n))
    return _EdgeSmoothFn.apply(img.contiguous(), weights, *[d.contiguous() for d in disp])


class _ResizeFn(torch.autograd.Function):
    """F.interpolate(D, [H, W], mode='bilinear', align_corners=False) on [B,1,h,w] maps (losses.py:214-215)."""

    @staticmethod
    def forward(ctx, D, H, W):
        D = L.dev(D.contiguous(), "depth")
        B, C, h, w = D.shape
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=D.device)
        L.check(L.lib().mcav_resize_bilinear_fwd(L.ptr(D), B, h, w, L.ptr(out), H, W, 0.0, 0.0, L.stream()), "mcav_resize_bilinear_fwd")
        ctx.dims = (B, h, w, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        B, h, w, H, W = ctx.dims
        g = L.dev(g.contiguous(), "grad")
        out = torch.empty((B, 1, h, w), dtype=torch.float32, device=g.device)
        L.check(L.lib().mcav_resize_bilinear_bwd(L.ptr(g), B, h, w, L.ptr(out), H, W, 0.0, 0.0, 0, L.stream()), "mcav_resize_bilinear_bwd")
        return out, None, None


def _stacked_pair(dt, dr):
    """The target and reference maps of one scale as ONE [2B,1,h,w] buffer: a view when they already lie back to back in one allocation
    (DispResNet.forward_pair's outputs), a concatenation otherwise.  -> (buffer, was a view)"""
    if dt.shape != dr.shape:
        raise L.MCAVError("depth pyramid: the two passes' maps of a scale must have one shape")
    B, _, h, w = dt.shape
    if (dt.is_contiguous() and dr.is_contiguous() and dt.untyped_storage().data_ptr() == dr.untyped_storage().data_ptr()
            and dr.data_ptr() == dt.data_ptr() + 4 * dt.numel()):
        return torch.as_strided(dt, (2 * B, 1, h, w), (h * w, h * w, w, 1)), True
    return torch.cat([dt, dr], 0), False


class _DepthPyramidFn(torch.autograd.Function):
    """Coarse disparities of both depth passes -> their full-resolution depths (include/mcav_depth.h: mcav_depth_pyramid_fwd / _bwd): one
    launch forward, one backward, for up to PYR_MAX_LEVELS scales.  Inputs (tgt_1, ref_1, tgt_2, ref_2, ...), each [B,1,h,w]; outputs the
    depths in that order, each [B,1,H,W], then the gradient buffer [levels,2B,1,H,W]: a consumer that writes the gradient of output k
    straight into that buffer's slice k (losses._WarpLossFn's grad_out) saves the backward its gather copy."""

    @staticmethod
    def forward(ctx, H, W, flags, *disps):
        n = len(disps) // 2
        if n < 1 or n > L.PYR_MAX_LEVELS or len(disps) != 2 * n:
            raise L.MCAVError("depth pyramid: 1 to %d scales, a target and a reference map each" % L.PYR_MAX_LEVELS)
        bufs = [_stacked_pair(L.dev(disps[2 * l].contiguous(), "disparity"), L.dev(disps[2 * l + 1].contiguous(), "disparity"))[0] for l in range(n)]
        B2 = bufs[0].shape[0]
        if any(b.shape[0] != B2 for b in bufs):
            raise L.MCAVError("depth pyramid: every scale must have the same batch")
        out = torch.empty((n, B2, 1, H, W), dtype=torch.float32, device=bufs[0].device)
        d_out = torch.empty_like(out)
        levels = (L.PyrLevel * n)(*[L.PyrLevel(b.data_ptr(), 0, b.shape[2], b.shape[3]) for b in bufs])
        L.check(L.lib().mcav_depth_pyramid_fwd(levels, n, B2, H, W, flags, L.ptr(out), L.stream()), "mcav_depth_pyramid_fwd")
        ctx.keep = (bufs, out, d_out, flags)
        ctx.mark_non_differentiable(d_out)
        B = B2 // 2
        return tuple(out[l, p * B:(p + 1) * B] for l in range(n) for p in range(2)) + (d_out,)

    @staticmethod
    def backward(ctx, *grads):
        bufs, out, d_out, flags = ctx.keep
        n, B2, _, H, W = out.shape
        B = B2 // 2
        for k, g in enumerate(grads[:2 * n]):
            slot = d_out[k // 2, (k % 2) * B:(k % 2 + 1) * B]
            if g is None:
                slot.zero_()
            elif not (g.data_ptr() == slot.data_ptr() and g.is_contiguous() and g.shape == slot.shape):
                slot.copy_(g)           # (a gradient that did not come straight from the consumer's write into the buffer)
        dd = [torch.empty_like(b) for b in bufs]
        levels = (L.PyrLevel * n)(*[L.PyrLevel(b.data_ptr(), g.data_ptr(), b.shape[2], b.shape[3]) for b, g in zip(bufs, dd)])
        L.check(L.lib().mcav_depth_pyramid_bwd(levels, n, B2, H, W, flags, L.ptr(out), L.ptr(d_out), L.stream()), "mcav_depth_pyramid_bwd")
        return (None, None, None) + tuple(g[p * B:(p + 1) * B] for g in dd for p in range(2))


def depth_pyramid(disp_t, disp_r, H, W, resize_then_depth=False):
    """Full-resolution depths of the coarse scales of both passes through the fused pyramid kernels.  disp_t, disp_r: lists of [B,1,h,w]
    sigmoid disparities (any number: groups of PYR_MAX_LEVELS, one launch pair each).  -> (depths of tgt, depths of ref, gradient slots):
    slot s is the pair of [B,1,H,W] views a consumer may write d loss / d depth into (see _DepthPyramidFn)."""
    flags = L.PYR_RESIZE_THEN_DEPTH if resize_then_depth else 0
    Dt, Dr, slots = [], [], []
    for g0 in range(0, len(disp_t), L.PYR_MAX_LEVELS):
        pairs = [d for s in range(g0, min(g0 + L.PYR_MAX_LEVELS, len(disp_t))) for d in (disp_t[s], disp_r[s])]
        res = _DepthPyramidFn.apply(H, W, flags, *pairs)
        d_out, B = res[-1], pairs[0].shape[0]
        for l in range(len(pairs) // 2):
            Dt.append(res[2 * l])
            Dr.append(res[2 * l + 1])
            slots.append((d_out[l, :B], d_out[l, B:]))
    return Dt, Dr, slots


def multiscale_losses(tgt, refs, disparity, poses, K, inputs_are_depth=False, ssim=False, min_reprojection=False, automask=False,
                      selections=None, edge_aware_smoothness=False, edge_smoothness_weight=1e-3, stereo=None, stereo_baseline=None,
                      multiscale_upsample="depth", fused_pyramid=False):
    """Losses.forward for depth nets that return several scales (DispNetS, DispResNet(scales=n)).  Per scale: depth (from disparity),
    bilinear resize to the image size, the fused 3-warp kernel (L1, or the 0.85 SSIM + 0.15 L1 mix when ssim: the reference composes its
    photometric term per scale, losses.py:209-221) on the resized depths; smoothness on the native-resolution depths of tgt.
    min_reprojection / automask: the masked modes of losses.Losses, applied per scale; selections: a list that receives each scale's
    selection map (uint8 [B,2,H,W]).  edge_aware_smoothness: the smoothness term is edge_smooth_loss(disparities of tgt, tgt,
    edge_smoothness_weight) instead (disparity inputs only).  stereo / stereo_baseline: the mono + stereo loss at every scale (the stereo
    frame [B,3,H,W], its baseline [B] float32 on the device; term weights (1/6, 1/6, 1/2, 1/6) / n).
    multiscale_upsample: "depth" = the reference's order, D_s = resize(1 / (10 d_s + 0.01)); "disparity" = monodepth2's,
    D_s = 1 / (10 resize(d_s) + 0.01) (disparity inputs only).  fused_pyramid: the coarse scales of both passes go through ONE forward and
    ONE backward launch (depth_pyramid) instead of a disp_to_depth and a resize launch per scale, pass and direction."""
    import losses as LS                      # the fused kernel's autograd node
    from geometry.pose_geometry import _DispToDepthFn, disp_to_depth
    from mcav import tape  # noqa: F401  (registers the resize entry points)
    if multiscale_upsample not in ("depth", "disparity"):
        raise L.MCAVError("multiscale_upsample must be 'depth' or 'disparity', got %r" % (multiscale_upsample,))
    H, W = tgt.shape[-2:]
    rtd = multiscale_upsample == "disparity"
    slots = None
    if fused_pyramid or rtd:
        if inputs_are_depth:
            raise L.MCAVError("multiscale_upsample='disparity' and fused_pyramid act on disparities, not depths")
        nsc = len(disparity[0])
        coarse = [s for s in range(nsc) if disparity[0][s].shape[-1] != W]
        # the reference's smoothness reads the native-resolution depths of tgt; the edge-aware term reads the disparities themselves
        depths = [None if edge_aware_smoothness else [_DispToDepthFn.apply(d) for d in disparity[0]]]
        full = [[None] * nsc, [None] * nsc]
        for s in range(nsc):
            if s not in coarse:                            # already at the image's size: the depth, nothing to resize
                full[0][s] = depths[0][s] if depths[0] is not None else _DispToDepthFn.apply(disparity[0][s])
                full[1][s] = _DispToDepthFn.apply(disparity[1][s])
            elif not fused_pyramid:
                full[0][s], full[1][s] = (_DispToDepthFn.apply(_ResizeFn.apply(disparity[t][s], H, W)) for t in (0, 1))
        if fused_pyramid and coarse:
            Dt, Dr, sl = depth_pyramid([disparity[0][s] for s in coarse], [disparity[1][s] for s in coarse], H, W, rtd)
            slots = {}
            for k, s in enumerate(coarse):
                full[0][s], full[1][s], slots[s] = Dt[k], Dr[k], sl[k]
    else:
        depths = disparity if inputs_are_depth else disp_to_depth(disparity)
        full = None
    n = len(disparity[0])
    tw = (0.5 / (2 * n), 0.5 / (2 * n), 1.0 / (2 * n))      # mean of the two tgt-view terms; every term / (2 n)  (losses.py:227-240)
    if stereo is not None:
        tw = tuple(w / n for w in LS.STEREO_TERM_WEIGHTS)
        stereo, stereo_baseline = stereo.contiguous(), stereo_baseline.contiguous()
    flags = L.WL_INPUT_DEPTH | L.WL_NO_SMOOTH | (L.WL_SSIM if ssim else 0)
    flags |= (L.WL_MIN_REPROJ if min_reprojection else 0) | (L.WL_AUTOMASK if automask else 0)
    masked = min_reprojection or automask
    total = None
    for s in range(n):
        if full is not None:
            Dt, Dr = full[0][s], full[1][s]
        else:
            Dt, Dr = depths[0][s], depths[1][s]
            if Dt.shape[-1] != W:
                Dt, Dr = _ResizeFn.apply(Dt, H, W), _ResizeFn.apply(Dr, H, W)
        sel = None
        if selections is not None:
            sel = (torch.empty if masked else torch.zeros)((tgt.shape[0], 2, H, W), dtype=torch.uint8, device=tgt.device)
            selections.append(sel)
        l0, _ = LS._WarpLossFn.apply(Dt.contiguous(), Dr.contiguous(), poses.contiguous(), tgt.contiguous(), refs[0].contiguous(),
                                     refs[1].contiguous(), K.contiguous(), flags, tw, sel, stereo, stereo_baseline,
                                     slots.get(s) if slots else None)      # (pyramid scales: the gradients land in its buffer)
        total = l0 if total is None else total + l0
    if edge_aware_smoothness:
        if inputs_are_depth:
            raise L.MCAVError("edge-aware smoothness acts on disparities, not depths")
        return [total, edge_smooth_loss(disparity[0], tgt, edge_smoothness_weight)]
    return [total, smooth_loss(depths[0])]
