"""Pillars -> bird's-eye-view pseudo-image on the GPU: the first layers of a LiDAR 3-D detector (PointPillars / SECOND / OpenPCDet).

`PillarFeatureNet(weight, bias)` is PillarVFE's single layer in evaluation mode -- Linear, BatchNorm1d folded into it, ReLU, the maximum
over a pillar's points -- and `pseudo_image(pillars)` is that layer followed by PointPillarScatter: a `PillarBatch` in, the dense
[B, C_out, ny, nx] canvas a convolutional backbone reads out, in one launch that writes every element of the canvas once
(mcav_pillar_pseudo_image; the definition is tests/pfn_ref.py).  `from_state_dict` reads a detector checkpoint's `vfe.pfn_layers.0.*`.
Nothing is read back.

Both calls are differentiable: when grad mode is on and the weight, the bias, bias_pad or the pillars' voxels require a gradient they run
through one torch.autograd.Function whose backward is `gradients` (mcav_pillar_pseudo_image_bwd; the definition is tests/pfn_bwd_ref.py),
which recomputes the layer and keeps nothing of the forward.  `PillarFeatureLayer` is the torch.nn.Module with a PFNLayer's state dict
that fine-tunes the layer on pseudo-LiDAR clouds, and with batch_stats=True trains it with BatchNorm's batch statistics: `pillar_moments`
(mcav_pillar_moments; the definition is tests/pfn_stats_ref.py) sums the used voxel slots and their products once, `fold_batch` turns the
moments into the folded layer, and `pillar_moments_backward` (mcav_pillar_moments_bwd) carries the statistics' gradient to the voxels.
"""
import ctypes

import numpy as np
import torch

from mcav import lib as L

from .clouds import PillarBatch, PillarGrid

L.register({
    "mcav_pillar_pseudo_image": (L.c_i, [L.c_p] * 4 + [L.c_i, ctypes.c_longlong] + [L.c_i] * 4 + [L.c_p] * 3 + [L.c_i, L.c_i] + [L.c_p] * 3),
    "mcav_pillar_pseudo_image_bwd_workspace_bytes": (L.c_sz, [ctypes.c_longlong, L.c_i, L.c_i]),
    "mcav_pillar_pseudo_image_bwd": (L.c_i, [L.c_p] * 4 + [L.c_i, ctypes.c_longlong] + [L.c_i] * 4 + [L.c_p] * 3 + [L.c_i, L.c_i] + [L.c_p] * 6 +
                                     [L.c_p, L.c_sz, L.c_p]),
    "mcav_pillar_moments_workspace_bytes": (L.c_sz, [ctypes.c_longlong, L.c_i, L.c_i]),
    "mcav_pillar_moments": (L.c_i, [L.c_p] * 3 + [L.c_i, ctypes.c_longlong, L.c_i, L.c_i] + [L.c_p] * 2 + [L.c_sz, L.c_p]),
    "mcav_pillar_moments_bwd": (L.c_i, [L.c_p] * 3 + [L.c_i, ctypes.c_longlong, L.c_i, L.c_i] + [L.c_p] * 4),
})

PFN_NHWC = 1                                   # include/mcav_depth.h MCAV_PFN_NHWC
COLUMNS, OUT_CHANNELS = (4, 9), (32, 64, 96, 128)


def _f64(sd, key, shape=None, optional=False):
    if key not in sd:
        if optional:
            return None
        raise L.MCAVError("PillarFeatureNet: the state dict has no %r" % key)
    v = sd[key]
    v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    v = v.astype(np.float64)
    if shape is not None and v.shape != shape:
        raise L.MCAVError("PillarFeatureNet: %r is %s, expected %s" % (key, list(v.shape), list(shape)))
    return v


def _checked_pillars(pillars, what, columns=None, device=None, need_grid=False):
    """-> capacity, B.  Shapes, columns and the grid first, devices and dtypes last: what can be refused without a GPU is.  columns: what a
    layer takes (None: 4 or 9); device: the layer's (None: the voxels')"""
    if not isinstance(pillars, PillarBatch):
        raise L.MCAVError("%s: pillars must be a PillarBatch, got %r" % (what, type(pillars).__name__))
    vox = pillars.voxels
    if not torch.is_tensor(vox) or vox.dim() != 3 or not 1 <= vox.shape[1] <= 64:
        raise L.MCAVError("%s: voxels must be [capacity, N <= 64, C]" % what)
    if columns is None and vox.shape[2] not in COLUMNS:
        raise L.MCAVError("%s: the pillars have %d columns, not 4 or 9" % (what, vox.shape[2]))
    if columns is not None and vox.shape[2] != columns:
        raise L.MCAVError("%s: the pillars have %d columns, the layer takes %d" % (what, vox.shape[2], columns))
    cap, B = vox.shape[0], len(pillars)
    if B < 1 or cap < 1:
        raise L.MCAVError("%s: an empty PillarBatch" % what)
    buffers = ((pillars.coords, "coords", (cap, 4), torch.int32), (pillars.num_points, "num_points", (cap,), torch.int32),
               (pillars.offsets, "offsets", (B + 1,), torch.int32), (vox, "voxels", tuple(vox.shape), torch.float32))
    for t, name, shape, _ in buffers:
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            raise L.MCAVError("%s: %s must be %s" % (what, name, list(shape)))
    if need_grid and not isinstance(pillars.grid, PillarGrid):
        raise L.MCAVError("%s: the PillarBatch has no grid (pillarize sets it)" % what)
    device = vox.device if device is None else device
    for t, name, _, dt in buffers:
        if L.dev(t, name, dt).device != device:
            raise L.MCAVError("%s: %s is on %s, the layer on %s" % (what, name, t.device, device))
    return cap, B


# ---------------------------------------------------------------------------------------------- the voxels' moments
def moments_size(columns):
    return 2 + columns + columns * columns


def _moments_vector(t, columns, dev, what, name):
    if not torch.is_tensor(t) or tuple(t.shape) != (moments_size(columns),) or L.dev(t, name, torch.float64).device != dev:
        raise L.MCAVError("%s: %s must be float64 [%d] on %s" % (what, name, moments_size(columns), dev))
    return t


def pillar_moments(pillars, out=None):
    """-> float64 [2 + C + C C] on the pillars' device (mcav_pillar_moments, two launches, nothing read back; the definition is
    tests/pfn_stats_ref.py): rows = P N, used = the number of used slots, s[c] = the sum of the used slots' column c, M[c][c'] = the sum of
    the products of their columns c and c'.  The statistics of y = W x over all P N rows of the zero-padded tensor follow from them
    (fold_batch).  out: a tensor to fill (needed under graph capture).
    Differentiable: with grad mode on and pillars.voxels requiring a gradient the call is a node of the autograd graph (out= is refused
    then) whose backward is pillar_moments_backward; rows and used have no gradient."""
    wants_grad = torch.is_grad_enabled() and isinstance(pillars, PillarBatch) and torch.is_tensor(pillars.voxels) and pillars.voxels.requires_grad
    if wants_grad and out is not None:
        raise L.MCAVError("pillar_moments: out= cannot be given when a gradient is required")
    cap, B = _checked_pillars(pillars, "pillar_moments")
    if wants_grad:
        return _MomentsFunction.apply(pillars, pillars.voxels)
    vox = pillars.voxels
    N, columns, dev = vox.shape[1], vox.shape[2], vox.device
    out = torch.empty(moments_size(columns), dtype=torch.float64, device=dev) if out is None else _moments_vector(out, columns, dev, "pillar_moments", "out")
    hl = L.lib()
    nbytes = hl.mcav_pillar_moments_workspace_bytes(cap, N, columns)
    if nbytes == 0:
        raise L.MCAVError("pillar_moments: %d rows of %d slots and %d columns are refused" % (cap, N, columns))
    with torch.cuda.device(dev):
        ws = L.workspace(nbytes, dev, "pfn_stats")
        L.check(hl.mcav_pillar_moments(L.ptr(vox), L.ptr(pillars.num_points), L.ptr(pillars.offsets), B, cap, N, columns, L.ptr(out), L.ptr(ws),
                                       nbytes, L.stream()), "mcav_pillar_moments")
    return out


def pillar_moments_backward(pillars, grad_moments, out=None):
    """The backward of pillar_moments as a plain call (mcav_pillar_moments_bwd, one launch, no host synchronisation): grad_moments float64
    [2 + C + C C], laid out as the moments are (its first two entries are not read; the part of M may be any matrix H) -> d_voxels
    [capacity, N, C] float32, every element written: float32(g_s[c] + sum_c' (H[c][c'] + H[c'][c]) x[c']) in the used slots, +0.0 in the
    others.  out: the tensor to fill (needed under graph capture)."""
    cap, B = _checked_pillars(pillars, "pillar_moments_backward")
    vox = pillars.voxels
    N, columns, dev = vox.shape[1], vox.shape[2], vox.device
    grad = _moments_vector(grad_moments, columns, dev, "pillar_moments_backward", "grad_moments")
    if out is None:
        out = torch.empty(tuple(vox.shape), dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or tuple(out.shape) != tuple(vox.shape) or L.dev(out, "out").device != dev:
        raise L.MCAVError("pillar_moments_backward: out must be float32 %s on %s" % (list(vox.shape), dev))
    with torch.cuda.device(dev):
        L.check(L.lib().mcav_pillar_moments_bwd(L.ptr(vox), L.ptr(pillars.num_points), L.ptr(pillars.offsets), B, cap, N, columns,
                                                L.c_p(grad.data_ptr() + 16), L.c_p(grad.data_ptr() + 8 * (2 + columns)), L.ptr(out), L.stream()),
                "mcav_pillar_moments_bwd")
    return out


class _MomentsFunction(torch.autograd.Function):
    """pillar_moments as one node: the backward is pillar_moments_backward on the saved voxels"""

    @staticmethod
    def forward(ctx, pillars, voxels):
        ctx.pillars = pillars
        ctx.save_for_backward(voxels)
        return pillar_moments(pillars)                                                      # grad mode is off in here

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        voxels, = ctx.saved_tensors
        if voxels.data_ptr() != ctx.pillars.voxels.data_ptr():
            raise L.MCAVError("backward: the PillarBatch's voxels were replaced after the forward")
        return None, pillar_moments_backward(ctx.pillars, grad.to(torch.float64).contiguous())


def fold_batch(weight, gamma, beta, moments, eps, running_mean, running_var, grid=None, dtype=torch.float32):
    """A bias-free Linear and the training-mode BatchNorm1d behind it folded into one layer, the batch statistics taken from the voxels'
    moments: a pure function of differentiable float64 torch ops on any device, rounded once to float32 at the end.
    weight [C_out, C or 10], gamma, beta, running_mean, running_var [C_out], moments float64 [2 + C + C C] (pillar_moments)
    -> weight' [C_out, C], bias, bias_pad (None: the bias itself) float32; mean, var (biased) float64 [C_out] as folded; rows.
        mean = W s / rows,  var = max(diag(W (M / rows) W^T) - mean^2, 0),  scale = gamma / sqrt(var + eps),
        weight' = W scale,  bias = beta - mean scale
    A 10-column weight (OpenPCDet's z - zc column, zc from `grid`) extends the 9-column moments by that column first and is collapsed to
    nine columns as PillarFeatureNet.fold_state_dict does.  With rows < 2 there are no batch statistics (stock BatchNorm raises): the
    running ones are folded, chosen by a torch.where on the device, and come back as mean and var.  dtype: what the folded layer is
    rounded to (the kernels take float32; float64 leaves the fold unrounded)."""
    w = weight.double()
    columns = 9 if w.shape[1] == 10 else w.shape[1]
    rows, used = moments[0], moments[1]
    s, M = moments[2:2 + columns], moments[2 + columns:].view(columns, columns)
    if w.shape[1] == 10:
        if not isinstance(grid, PillarGrid):
            raise L.MCAVError("fold_batch: a 10-column weight (z - zc) needs the PillarGrid whose z range gives zc")
        zc = (grid.z[0] + grid.z[1]) / 2.0
        cross = M[2] - zc * s                                                               # sum of (z - zc) x_j
        last = M[2, 2] - 2.0 * zc * s[2] + zc * zc * used
        s = torch.cat([s, (s[2] - zc * used)[None]])
        M = torch.cat([torch.cat([M, cross[:, None]], dim=1), torch.cat([cross, last[None]])[None, :]], dim=0)
    ok = rows >= 2
    count = torch.where(ok, rows, torch.ones_like(rows))
    batch_mean = (w @ s) / count
    batch_var = torch.clamp(((w @ (M / count)) * w).sum(dim=1) - batch_mean * batch_mean, min=0.0)
    mean = torch.where(ok, batch_mean, running_mean.double())
    var = torch.where(ok, batch_var, running_var.double())
    scale = gamma.double() / torch.sqrt(var + eps)
    wf = w * scale[:, None]
    bf = beta.double() + (0.0 - mean) * scale
    if w.shape[1] != 10:
        return wf.to(dtype).contiguous(), bf.to(dtype), None, mean, var, rows
    bias = bf - wf[:, 9] * zc
    wf = torch.cat([wf[:, :2], (wf[:, 2] + wf[:, 9])[:, None], wf[:, 3:9]], dim=1)
    return wf.to(dtype).contiguous(), bias.to(dtype), bf.to(dtype), mean, var, rows


def update_running_stats(norm, mean, var, rows):
    """BatchNorm1d's training-mode update of `norm`'s buffers from fold_batch's mean, var (biased) and rows, in float64 device ops under
    no_grad, nothing read back: running_mean = (1 - m) running_mean + m mean, running_var likewise with var rows / (rows - 1),
    num_batches_tracked += 1; m = norm.momentum, or 1 / num_batches_tracked (the cumulative average) for None.  rows < 2 updates nothing."""
    with torch.no_grad():
        ok = rows >= 2
        tracked = norm.num_batches_tracked + ok.to(norm.num_batches_tracked.dtype)
        m = 1.0 / tracked.double().clamp(min=1.0) if norm.momentum is None else norm.momentum
        unbiased = var * (rows / torch.where(ok, rows - 1.0, torch.ones_like(rows)))
        for buf, new in ((norm.running_mean, mean), (norm.running_var, unbiased)):
            buf.copy_(torch.where(ok, (1.0 - m) * buf.double() + m * new, buf.double()))
        norm.num_batches_tracked.copy_(tracked)


class PillarFeatureNet:
    """weight [C_out, C], bias [C_out], bias_pad [C_out]: float32 on the GPU, C = 4 or 9 (a PillarBatch's columns), C_out a multiple of 32
    in 32..128.  feat[p, o] = max over the pillar's points of relu(weight[o] . point + bias[o]); a pillar with unused slots also takes
    relu(bias_pad[o]) into the maximum.  bias_pad=None means bias_pad = bias: what second.pytorch and OpenPCDet compute, whose zero-padded
    rows go through the layer; zeros ignore the padding."""

    def __init__(self, weight, bias, bias_pad=None):
        bias_pad = bias if bias_pad is None else bias_pad
        for t, name in ((weight, "weight"), (bias, "bias"), (bias_pad, "bias_pad")):
            if not torch.is_tensor(t):
                raise L.MCAVError("PillarFeatureNet: %s must be a tensor on the GPU" % name)
        if weight.dim() != 2 or weight.shape[1] not in COLUMNS or weight.shape[0] not in OUT_CHANNELS:
            raise L.MCAVError("PillarFeatureNet: weight must be [C_out, C] with C in %s and C_out in %s, got %s"
                              % (COLUMNS, OUT_CHANNELS, list(weight.shape)))
        self.c_out, self.columns = int(weight.shape[0]), int(weight.shape[1])
        for t, name in ((bias, "bias"), (bias_pad, "bias_pad")):
            if tuple(t.shape) != (self.c_out,):
                raise L.MCAVError("PillarFeatureNet: %s must be [%d], got %s" % (name, self.c_out, list(t.shape)))
        self.weight, self.bias, self.bias_pad = L.dev(weight, "weight"), L.dev(bias, "bias"), L.dev(bias_pad, "bias_pad")
        if not (self.bias.device == self.bias_pad.device == self.weight.device):
            raise L.MCAVError("PillarFeatureNet: weight, bias and bias_pad must be on one device")

    @staticmethod
    def fold_state_dict(sd, prefix="vfe.pfn_layers.0.", eps=1e-3, grid=None):
        """-> weight [C_out, C], bias [C_out], bias_pad [C_out] as float32 numpy arrays: `linear.weight` (and an optional `linear.bias`) with
        the evaluation-mode `norm.{weight, bias, running_mean, running_var}` folded in, in float64, rounded once:
        scale = gamma / sqrt(var + eps), w' = w scale, b' = beta + (linear.bias - mean) scale.  An OpenPCDet weight of 10 columns
        (x y z i, 3 offsets from the mean, 3 from the pillar's centre) is taken when `grid` is given: its 10th column is z - zc with one
        zc = (z0 + z1) / 2 per grid, so w'[:, 2] += w'[:, 9], bias = b' - w'[:, 9] zc, and the zero-padded rows see bias_pad = b'."""
        w = _f64(sd, prefix + "linear.weight")
        if w.ndim != 2 or w.shape[0] not in OUT_CHANNELS or w.shape[1] not in COLUMNS + (10,):
            raise L.MCAVError("PillarFeatureNet: %slinear.weight must be [C_out, 4, 9 or 10] with C_out in %s, got %s"
                              % (prefix, OUT_CHANNELS, list(w.shape)))
        n = (w.shape[0],)
        gamma, beta = _f64(sd, prefix + "norm.weight", n), _f64(sd, prefix + "norm.bias", n)
        mean, var = _f64(sd, prefix + "norm.running_mean", n), _f64(sd, prefix + "norm.running_var", n)
        lb = _f64(sd, prefix + "linear.bias", n, optional=True)
        if not (var + eps > 0).all():
            raise L.MCAVError("PillarFeatureNet: %snorm.running_var + eps must be positive" % prefix)
        scale = gamma / np.sqrt(var + eps)
        wf = w * scale[:, None]
        bf = beta + ((0.0 if lb is None else lb) - mean) * scale
        bias = bf
        if w.shape[1] == 10:
            if not isinstance(grid, PillarGrid):
                raise L.MCAVError("PillarFeatureNet: a 10-column weight (z - zc) needs the PillarGrid whose z range gives zc")
            zc = (grid.z[0] + grid.z[1]) / 2.0
            bias = bf - wf[:, 9] * zc
            wf = np.concatenate([wf[:, :2], (wf[:, 2] + wf[:, 9])[:, None], wf[:, 3:9]], axis=1)
        f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)
        return f32(wf), f32(bias), f32(bf)

    @classmethod
    def from_state_dict(cls, sd, prefix="vfe.pfn_layers.0.", eps=1e-3, grid=None, device="cuda"):
        """The layer of a detector checkpoint (fold_state_dict) on `device`"""
        return cls(*[torch.from_numpy(v).to(device) for v in cls.fold_state_dict(sd, prefix, eps, grid)])

    def _pillars(self, pillars, what, need_grid=False):
        return _checked_pillars(pillars, what, self.columns, self.weight.device, need_grid)

    def _features_out(self, features, cap, what):
        if tuple(features.shape) != (cap, self.c_out) or L.dev(features, "features").device != self.weight.device:
            raise L.MCAVError("%s: features must be [%d, %d] on %s" % (what, cap, self.c_out, self.weight.device))
        return features

    def _call(self, pillars, B, cap, nx, ny, flags, canvas, features):
        with torch.cuda.device(self.weight.device):
            L.check(L.lib().mcav_pillar_pseudo_image(L.ptr(pillars.voxels), L.ptr(pillars.coords), L.ptr(pillars.num_points),
                                                     L.ptr(pillars.offsets), B, cap, pillars.voxels.shape[1], self.columns, nx, ny,
                                                     L.ptr(self.weight), L.ptr(self.bias), L.ptr(self.bias_pad), self.c_out, flags,
                                                     L.ptr(canvas), L.ptr(features), L.stream()), "mcav_pillar_pseudo_image")

    def features(self, pillars, out=None):
        """-> [capacity, C_out] float32: a feature row for every pillar of the batch (rows at and beyond the pillar count are not
        written).  out: a tensor to fill.  No canvas is made.  Differentiable (see pseudo_image)."""
        cap, B = self._pillars(pillars, "features")
        if self._wants_grad(pillars):
            if out is not None:
                raise L.MCAVError("features: out= cannot be given when a gradient is required")
            return _PillarFunction.apply(self, pillars, None, self.weight, self.bias, self.bias_pad, pillars.voxels)
        out = torch.empty((cap, self.c_out), dtype=torch.float32, device=self.weight.device) if out is None else self._features_out(out, cap, "features")
        self._call(pillars, B, cap, 1, 1, 0, None, out)
        return out

    def pseudo_image(self, pillars, layout="nchw", out=None, features=None):
        """-> [B, C_out, ny, nx] float32 on pillars.grid, every element written: the pillar's features in its cell, +0.0 elsewhere.
        layout: "nchw", or "nhwc": the same shape as a channels_last tensor (a torch backbone takes either).  out: a canvas of that
        shape and memory format to fill (needed under graph capture); features: a [capacity, C_out] tensor that also receives the
        feature rows.  No host synchronisation.
        Differentiable: with grad mode on and a weight, bias, bias_pad or pillars.voxels that requires a gradient the call is a node of the
        autograd graph (out= and features= are refused then) whose backward is `gradients`; the pillars' coords, num_points and offsets
        must still hold what they held when backward runs."""
        if layout not in ("nchw", "nhwc"):
            raise L.MCAVError("pseudo_image: layout must be 'nchw' or 'nhwc', got %r" % (layout,))
        cap, B = self._pillars(pillars, "pseudo_image", need_grid=True)
        if self._wants_grad(pillars):
            if out is not None or features is not None:
                raise L.MCAVError("pseudo_image: out= and features= cannot be given when a gradient is required")
            return _PillarFunction.apply(self, pillars, layout, self.weight, self.bias, self.bias_pad, pillars.voxels)
        grid = pillars.grid
        shape, dev = (B, self.c_out, grid.ny, grid.nx), self.weight.device
        if features is not None:
            features = self._features_out(features, cap, "pseudo_image")
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev, memory_format=torch.channels_last if layout == "nhwc" else torch.contiguous_format)
        else:
            if not torch.is_tensor(out) or tuple(out.shape) != shape or not out.is_cuda or out.device != dev or out.dtype != torch.float32:
                raise L.MCAVError("pseudo_image: out must be float32 %s on %s" % (list(shape), dev))
            if not (out.permute(0, 2, 3, 1) if layout == "nhwc" else out).is_contiguous():
                raise L.MCAVError("pseudo_image: out must be %s" % ("channels_last" if layout == "nhwc" else "contiguous"))
        self._call(pillars, B, cap, grid.nx, grid.ny, PFN_NHWC if layout == "nhwc" else 0, out, features)
        return out

    # ------------------------------------------------------------------------------------------ the backward
    def _wants_grad(self, pillars):
        return torch.is_grad_enabled() and any(t.requires_grad for t in (self.weight, self.bias, self.bias_pad, pillars.voxels))

    def gradients(self, pillars, grad_canvas=None, grad_features=None, layout="nchw", need_voxels=False, out=None):
        """The backward of pseudo_image / features as a plain call (mcav_pillar_pseudo_image_bwd, two launches, no host synchronisation):
        grad_canvas [B, C_out, ny, nx] float32 in `layout`'s memory format and / or grad_features [capacity, C_out] float32 ->
        (d_weight [C_out, C], d_bias [C_out], d_bias_pad [C_out], d_voxels [capacity, N, C] or None), all float32.  The layer is
        recomputed, so the slot that receives a channel's gradient is the one whose value the forward wrote.  d_voxels costs
        capacity N C 4 bytes and is made only with need_voxels; every row of it is written, zeros behind the last pillar.
        out: the three or four tensors to fill (needed under graph capture)."""
        if layout not in ("nchw", "nhwc"):
            raise L.MCAVError("gradients: layout must be 'nchw' or 'nhwc', got %r" % (layout,))
        if grad_canvas is None and grad_features is None:
            raise L.MCAVError("gradients: grad_canvas or grad_features must be given")
        cap, B = self._pillars(pillars, "gradients", need_grid=grad_canvas is not None)
        return _gradients(pillars, self.weight.detach(), self.bias.detach(), self.bias_pad.detach(), cap, B, grad_canvas, grad_features, layout,
                          need_voxels, out)


def _gradients(pillars, weight, bias, bias_pad, cap, B, grad_canvas, grad_features, layout, need_voxels, out):
    dev, (c_out, columns), N = weight.device, weight.shape, pillars.voxels.shape[1]
    nx = ny = 1
    if grad_canvas is not None:
        nx, ny = pillars.grid.nx, pillars.grid.ny
        shape = (B, c_out, ny, nx)
        if not torch.is_tensor(grad_canvas) or tuple(grad_canvas.shape) != shape or grad_canvas.device != dev or grad_canvas.dtype != torch.float32:
            raise L.MCAVError("gradients: grad_canvas must be float32 %s on %s" % (list(shape), dev))
        if not (grad_canvas.permute(0, 2, 3, 1) if layout == "nhwc" else grad_canvas).is_contiguous():
            raise L.MCAVError("gradients: grad_canvas must be %s" % ("channels_last" if layout == "nhwc" else "contiguous"))
    if grad_features is not None:
        if not torch.is_tensor(grad_features) or tuple(grad_features.shape) != (cap, c_out) or L.dev(grad_features, "grad_features").device != dev:
            raise L.MCAVError("gradients: grad_features must be [%d, %d] on %s" % (cap, c_out, dev))
    shapes = [(c_out, columns), (c_out,), (c_out,)] + ([(cap, N, columns)] if need_voxels else [])
    if out is None:
        out = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
    else:
        out = list(out)
        if len(out) == 4 and not need_voxels:
            out = out[:3]                                    # a d_voxels buffer that nobody asked to fill is left alone
        if len(out) != len(shapes):
            raise L.MCAVError("gradients: out must hold %d tensors (d_weight, d_bias, d_bias_pad%s)" % (len(shapes), ", d_voxels" if need_voxels else ""))
        for t, s, name in zip(out, shapes, ("d_weight", "d_bias", "d_bias_pad", "d_voxels")):
            if not torch.is_tensor(t) or tuple(t.shape) != s or L.dev(t, name).device != dev:
                raise L.MCAVError("gradients: out's %s must be float32 %s on %s" % (name, list(s), dev))
    hl = L.lib()
    nbytes = hl.mcav_pillar_pseudo_image_bwd_workspace_bytes(cap, columns, c_out)
    if nbytes == 0:
        raise L.MCAVError("gradients: %d rows of %d columns under %d channels are refused" % (cap, columns, c_out))
    with torch.cuda.device(dev):
        ws = L.workspace(nbytes, dev, "pfn_bwd")
        L.check(hl.mcav_pillar_pseudo_image_bwd(L.ptr(pillars.voxels), L.ptr(pillars.coords), L.ptr(pillars.num_points), L.ptr(pillars.offsets),
                                                B, cap, N, columns, nx, ny, L.ptr(weight), L.ptr(bias), L.ptr(bias_pad), c_out,
                                                PFN_NHWC if layout == "nhwc" else 0, L.ptr(grad_canvas), L.ptr(grad_features), L.ptr(out[0]),
                                                L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]) if need_voxels else L.c_p(0), L.ptr(ws), nbytes,
                                                L.stream()), "mcav_pillar_pseudo_image_bwd")
    return out[0], out[1], out[2], (out[3] if need_voxels else None)


class _PillarFunction(torch.autograd.Function):
    """features (layout None) or pseudo_image as one node: the forward is the call without a graph, the backward is `gradients` on the
    saved weight, bias, bias_pad and voxels.  bias_pad being the bias itself, autograd adds the two gradients."""

    @staticmethod
    def forward(ctx, net, pillars, layout, weight, bias, bias_pad, voxels):
        ctx.pillars, ctx.layout = pillars, layout
        ctx.sizes = net._pillars(pillars, "backward", need_grid=layout is not None)
        ctx.save_for_backward(weight, bias, bias_pad, voxels)
        return net.features(pillars) if layout is None else net.pseudo_image(pillars, layout=layout)        # grad mode is off in here

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        weight, bias, bias_pad, voxels = ctx.saved_tensors
        if voxels.data_ptr() != ctx.pillars.voxels.data_ptr():
            raise L.MCAVError("backward: the PillarBatch's voxels were replaced after the forward")
        cap, B = ctx.sizes
        grad = grad.to(torch.float32)
        if ctx.layout is None:
            canvas, feats, layout = None, grad.contiguous(), "nchw"
        else:
            layout = ctx.layout
            canvas, feats = grad.contiguous(memory_format=torch.channels_last if layout == "nhwc" else torch.contiguous_format), None
        dw, db, dp, dv = _gradients(ctx.pillars, weight, bias, bias_pad, cap, B, canvas, feats, layout, ctx.needs_input_grad[6], None)
        return None, None, None, dw, db, dp, dv


class PillarFeatureLayer(torch.nn.Module):
    """PointPillars' PFNLayer as a trainable module on the fused kernels: submodules `linear` (no bias) and `norm` (BatchNorm1d), so the
    state dict is a PFNLayer's -- linear.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.num_batches_tracked --
    and a detector checkpoint's `vfe.pfn_layers.0.*` loads and saves.  in_columns: 4 or 9 (a PillarBatch's columns), or OpenPCDet's 10
    with the PillarGrid whose z range gives the tenth column's zc (the pillars still hold 9 columns); out_channels in 32, 64, 96, 128.

    forward(pillars, layout) folds the BatchNorm with its RUNNING statistics into the layer in differentiable float64 torch ops
    (PillarFeatureNet.fold_state_dict's formulas, rounded once to float32) and calls PillarFeatureNet.pseudo_image, whose backward is the
    HIP kernel.  This is frozen-statistics fine-tuning: linear.weight, norm.weight and norm.bias learn; running_mean and running_var are
    never updated, in train() as in eval(), and batch statistics over the pillars' points are not computed.

    batch_stats=True makes train() what BatchNorm1d's is: forward, features and folded(pillars) take the statistics of the batch -- of
    y = W x over all P N rows of the zero-padded voxels, as second.pytorch's masked rows give them -- from the voxels' moments
    (pillar_moments: 2 + C + C C numbers, one pass over the used slots, no [P, N, C_out] tensor), fold them (fold_batch) and update
    running_mean, running_var (unbiased) and num_batches_tracked as BatchNorm1d does, on the device, without a read-back; momentum=None is
    the cumulative average.  A batch of fewer than two rows folds the running statistics and updates nothing.  The gradients of the
    parameters flow through the statistics, and so does a second gradient of the voxels (pillar_moments_backward), which autograd adds
    to the kernel's.  eval() is the frozen path.  The state dict does not change."""

    def __init__(self, in_columns=9, out_channels=64, eps=1e-3, grid=None, batch_stats=False):
        super().__init__()
        if in_columns not in COLUMNS + (10,) or out_channels not in OUT_CHANNELS:
            raise L.MCAVError("PillarFeatureLayer: in_columns must be 4, 9 or 10 and out_channels in %s, got %r and %r"
                              % (OUT_CHANNELS, in_columns, out_channels))
        if in_columns == 10 and not isinstance(grid, PillarGrid):
            raise L.MCAVError("PillarFeatureLayer: 10 columns (z - zc) need the PillarGrid whose z range gives zc")
        self.in_columns, self.out_channels, self.eps, self.grid = in_columns, out_channels, float(eps), grid
        self.batch_stats = bool(batch_stats)
        self.linear = torch.nn.Linear(in_columns, out_channels, bias=False)
        self.norm = torch.nn.BatchNorm1d(out_channels, eps=eps)

    def _folded_batch(self, pillars):
        """the fold under the batch's statistics, and BatchNorm1d's update of the buffers: device ops, nothing read back"""
        norm = self.norm
        if not self.linear.weight.is_cuda:
            raise L.MCAVError("PillarFeatureLayer: batch statistics need the layer on the GPU: the moments have no CPU fallback")
        moments = pillar_moments(pillars)
        wf, bias, bias_pad, mean, var, rows = fold_batch(self.linear.weight, norm.weight, norm.bias, moments, self.eps, norm.running_mean,
                                                         norm.running_var, self.grid)
        update_running_stats(norm, mean, var, rows)
        return wf, bias, bias_pad

    def folded(self, pillars=None):
        """-> weight [C_out, C], bias, bias_pad (None: the bias itself) as float32 tensors with the parameters' graph behind them.
        pillars: the batch whose statistics a batch_stats layer in train() folds (and updates its buffers with, once per call); without
        them, in eval() or without batch_stats the running statistics are folded."""
        if pillars is not None and self.batch_stats and self.training:
            return self._folded_batch(pillars)
        w = self.linear.weight.double()
        scale = self.norm.weight.double() / torch.sqrt(self.norm.running_var.double() + self.eps)
        wf = w * scale[:, None]
        bf = self.norm.bias.double() + (0.0 - self.norm.running_mean.double()) * scale
        if self.in_columns != 10:
            return wf.float().contiguous(), bf.float(), None
        zc = (self.grid.z[0] + self.grid.z[1]) / 2.0
        bias = bf - wf[:, 9] * zc
        wf = torch.cat([wf[:, :2], (wf[:, 2] + wf[:, 9])[:, None], wf[:, 3:9]], dim=1)
        return wf.float().contiguous(), bias.float(), bf.float()

    def forward(self, pillars, layout="nchw"):
        """-> the pseudo-image [B, C_out, ny, nx] of PillarFeatureNet.pseudo_image under the folded layer"""
        return PillarFeatureNet(*self.folded(pillars)).pseudo_image(pillars, layout=layout)

    def features(self, pillars):
        """-> the feature rows [capacity, C_out] of PillarFeatureNet.features under the folded layer: forward without the canvas"""
        return PillarFeatureNet(*self.folded(pillars)).features(pillars)

    def eval_net(self):
        """-> the PillarFeatureNet of the current parameters, without a graph"""
        with torch.no_grad():
            return PillarFeatureNet(*[None if t is None else t.detach() for t in self.folded()])
