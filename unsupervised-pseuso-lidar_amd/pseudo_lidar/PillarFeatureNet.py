"""Pillars -> bird's-eye-view pseudo-image on the GPU: the first layers of a LiDAR 3-D detector (PointPillars / SECOND / OpenPCDet).

`PillarFeatureNet(weight, bias)` is PillarVFE's single layer in evaluation mode -- Linear, BatchNorm1d folded into it, ReLU, the maximum
over a pillar's points -- and `pseudo_image(pillars)` is that layer followed by PointPillarScatter: a `PillarBatch` in, the dense
[B, C_out, ny, nx] canvas a convolutional backbone reads out, in one launch that writes every element of the canvas once
(mcav_pillar_pseudo_image; the definition is tests/pfn_ref.py).  `from_state_dict` reads a detector checkpoint's `vfe.pfn_layers.0.*`.
Nothing is read back.
"""
import ctypes

import numpy as np
import torch

from mcav import lib as L

from .PseudoLiDAR import PillarBatch, PillarGrid

L.register({
    "mcav_pillar_pseudo_image": (L.c_i, [L.c_p] * 4 + [L.c_i, ctypes.c_longlong] + [L.c_i] * 4 + [L.c_p] * 3 + [L.c_i, L.c_i] + [L.c_p] * 3),
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
        """shapes, columns and the grid first, devices and dtypes last: what can be refused without a GPU is"""
        if not isinstance(pillars, PillarBatch):
            raise L.MCAVError("%s: pillars must be a PillarBatch, got %r" % (what, type(pillars).__name__))
        vox = pillars.voxels
        if not torch.is_tensor(vox) or vox.dim() != 3 or not 1 <= vox.shape[1] <= 64:
            raise L.MCAVError("%s: voxels must be [capacity, N <= 64, C]" % what)
        if vox.shape[2] != self.columns:
            raise L.MCAVError("%s: the pillars have %d columns, the layer takes %d" % (what, vox.shape[2], self.columns))
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
        for t, name, _, dt in buffers:
            if L.dev(t, name, dt).device != self.weight.device:
                raise L.MCAVError("%s: %s is on %s, the layer on %s" % (what, name, t.device, self.weight.device))
        return cap, B

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
        written).  out: a tensor to fill.  No canvas is made."""
        cap, B = self._pillars(pillars, "features")
        out = torch.empty((cap, self.c_out), dtype=torch.float32, device=self.weight.device) if out is None else self._features_out(out, cap, "features")
        self._call(pillars, B, cap, 1, 1, 0, None, out)
        return out

    def pseudo_image(self, pillars, layout="nchw", out=None, features=None):
        """-> [B, C_out, ny, nx] float32 on pillars.grid, every element written: the pillar's features in its cell, +0.0 elsewhere.
        layout: "nchw", or "nhwc": the same shape as a channels_last tensor (a torch backbone takes either).  out: a canvas of that
        shape and memory format to fill (needed under graph capture); features: a [capacity, C_out] tensor that also receives the
        feature rows.  No host synchronisation."""
        if layout not in ("nchw", "nhwc"):
            raise L.MCAVError("pseudo_image: layout must be 'nchw' or 'nhwc', got %r" % (layout,))
        cap, B = self._pillars(pillars, "pseudo_image", need_grid=True)
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
