"""evaluate.py -- depth metrics as the reference defines them (evaluate.py:6-39), computed on the GPU.

`compute_errors(gt, pred)` keeps the reference's call shape: `gt` a depth tensor, `pred` the depth network's output (a list whose
first entry is the full-resolution sigmoid disparity, or that tensor itself).  One fused pass (mcav_depth_metrics) instead of ~25
numpy temporaries; only the ten result floats cross PCIe.  Differences from the reference, on purpose: it works (the reference's
`disp_to_depth(pred[0]).cpu()` raises on the nested list it gets, evaluate.py:11-12) and 'sq_rel' is the squared-relative error
(the reference stores rms under that key, evaluate.py:36).  `min_gt`: ground-truth values <= min_gt are skipped (sparse KITTI
ground truth); the default -1 takes every element, as the reference does.

`evaluate_depth(gt, pred, sizes, crop, ...)` is the KITTI protocol of monodepth2's evaluate_depth.py instead: per image, at the ground
truth's own resolution, crop, depth range, per-image median scaling, metrics averaged over images (mcav_eval_depth; the definition is
tests/eval_protocol_ref.py).  `reduce_rows` turns the per-image rows of several batches into that result with one read-back.
`scales=` takes one scale per image on the device (mcav_eval_depth_scaled), e.g. pseudo_lidar.ground_scale's, which needs no ground truth.
"""
import torch

from mcav import lib as L

L.register({
    "mcav_depth_metrics_workspace_bytes": (L.c_sz, []),
    "mcav_depth_metrics": (L.c_i, [L.c_p, L.c_p, L.c_sz, L.c_f, L.c_p, L.c_p, L.c_sz, L.c_p]),
    "mcav_eval_depth_workspace_bytes": (L.c_sz, [L.c_i, L.c_i, L.c_i]),
    "mcav_eval_depth": (L.c_i, [L.c_p, L.c_p] + [L.c_i] * 5 + [L.c_p, L.c_p, L.c_f, L.c_f, L.c_f, L.c_i, L.c_p, L.c_p, L.c_sz, L.c_p]),
    "mcav_eval_depth_scaled": (L.c_i, [L.c_p, L.c_p] + [L.c_i] * 5 + [L.c_p, L.c_p, L.c_f, L.c_f, L.c_f, L.c_p, L.c_i, L.c_p, L.c_p, L.c_sz,
                                       L.c_p]),
})

KEYS = ("silog", "abs_rel", "log10", "rms", "sq_rel", "log_rms", "d1", "d2", "d3")


def compute_errors(gt, pred, min_gt=-1.0):
    disp = pred[0] if isinstance(pred, (list, tuple)) else pred
    gt = L.dev(gt.detach().to(torch.float32).contiguous(), "gt")
    disp = L.dev(disp.detach().to(torch.float32).contiguous(), "pred")
    if gt.numel() != disp.numel():
        raise L.MCAVError("compute_errors: gt has %d elements, the prediction %d" % (gt.numel(), disp.numel()))
    h = L.lib()
    ws = L.workspace(h.mcav_depth_metrics_workspace_bytes(), gt.device, "metrics")
    out = torch.empty(10, dtype=torch.float32, device=gt.device)
    L.check(h.mcav_depth_metrics(L.ptr(gt), L.ptr(disp), gt.numel(), float(min_gt), L.ptr(out), L.ptr(ws), ws.numel(), L.stream()),
            "mcav_depth_metrics")
    vals = out.cpu().tolist()
    acc = dict(zip(KEYS, vals[:9]))
    acc["count"] = int(vals[9])
    return acc


EVAL_MEDIAN_SCALING = 1                        # include/mcav_depth.h MCAV_EVAL_MEDIAN_SCALING
ROW_KEYS = KEYS + ("count", "ratio")
# crop boxes as fractions of the true ground-truth size (monodepth evaluation_utils.py / monodepth2 evaluate_depth.py)
CROPS = {"garg": (0.40810811, 0.99189189, 0.03594771, 0.96405229),
         "eigen": (0.3324324, 0.91351351, 0.0359477, 0.96405229)}


def crop_box(Hb, Wb, crop):
    """-> (y0, y1, x0, x1), half-open.  crop: 'garg', 'eigen' (float64 products, truncated), None (the whole image) or an explicit box."""
    if crop is None:
        return (0, Hb, 0, Wb)
    if isinstance(crop, str):
        if crop not in CROPS:
            raise L.MCAVError("evaluate_depth: crop must be 'garg', 'eigen', None or (y0, y1, x0, x1), got %r" % crop)
        fy0, fy1, fx0, fx1 = CROPS[crop]
        return (int(fy0 * Hb), int(fy1 * Hb), int(fx0 * Wb), int(fx1 * Wb))
    box = tuple(int(v) for v in crop)
    if len(box) != 4:
        raise L.MCAVError("evaluate_depth: an explicit crop is (y0, y1, x0, x1), got %r" % (crop,))
    return box


def eval_depth_rows(gt, pred, sizes=None, crop="garg", min_depth=1e-3, max_depth=80.0, median_scaling=True, scale=1.0, scales=None):
    """The per-image rows [B, 11] (ROW_KEYS: the nine metrics, count, ratio) on the device; no read-back.  Arguments as evaluate_depth."""
    disp = pred[0] if isinstance(pred, (list, tuple)) else pred
    gt = L.dev(gt.detach().to(torch.float32).contiguous(), "gt")
    disp = L.dev(disp.detach().to(torch.float32).contiguous(), "pred")
    if gt.dim() == 4:
        if gt.shape[1] != 1:
            raise L.MCAVError("evaluate_depth: gt must be [B,1,Hg,Wg] or [B,Hg,Wg], got %s" % (tuple(gt.shape),))
        gt = gt[:, 0]
    if disp.dim() == 4:
        if disp.shape[1] != 1:
            raise L.MCAVError("evaluate_depth: the prediction must be [B,1,h,w] or [B,h,w], got %s" % (tuple(disp.shape),))
        disp = disp[:, 0]
    if gt.dim() != 3 or disp.dim() != 3 or gt.shape[0] != disp.shape[0]:
        raise L.MCAVError("evaluate_depth: gt %s and prediction %s do not describe one batch" % (tuple(gt.shape), tuple(disp.shape)))
    B, Hg, Wg = gt.shape
    h, w = disp.shape[1:]
    if sizes is None:
        sizes = [(Hg, Wg)] * B
    sizes = [tuple(int(v) for v in s) for s in (sizes.tolist() if hasattr(sizes, "tolist") else sizes)]
    if len(sizes) != B or any(len(s) != 2 or not (1 <= s[0] <= Hg and 1 <= s[1] <= Wg) for s in sizes):
        raise L.MCAVError("evaluate_depth: sizes must hold %d pairs (Hb, Wb) with 1 <= Hb <= %d, 1 <= Wb <= %d, got %r" % (B, Hg, Wg, sizes))
    per_image = isinstance(crop, (list, tuple)) and len(crop) == B and len(crop) > 0 and isinstance(crop[0], (list, tuple))
    boxes = [crop_box(Hb, Wb, crop[b] if per_image else crop) for b, (Hb, Wb) in enumerate(sizes)]
    if not (float(min_depth) > 0 and float(max_depth) > float(min_depth)):
        raise L.MCAVError("evaluate_depth: need 0 < min_depth < max_depth, got %r, %r" % (min_depth, max_depth))
    dev = gt.device
    meta = torch.tensor([v for s in sizes for v in s] + [v for bx in boxes for v in bx], dtype=torch.int32).to(dev)
    rows = torch.empty((B, 11), dtype=torch.float32, device=dev)
    h_ = L.lib()
    ws = L.workspace(h_.mcav_eval_depth_workspace_bytes(B, Hg, Wg), dev, "eval_depth")
    flags = EVAL_MEDIAN_SCALING if median_scaling else 0
    if scales is None:
        L.check(h_.mcav_eval_depth(L.ptr(gt), L.ptr(disp), B, Hg, Wg, h, w, L.ptr(meta), L.c_p(meta.data_ptr() + 4 * 2 * B),
                                   float(min_depth), float(max_depth), float(scale), flags, L.ptr(rows), L.ptr(ws), ws.numel(), L.stream()),
                "mcav_eval_depth")
        return rows
    if not torch.is_tensor(scales) or tuple(scales.shape) != (B,):
        raise L.MCAVError("evaluate_depth: scales must be a float32 tensor [%d] on the GPU" % B)
    scales = L.dev(scales.detach().contiguous() if scales.is_cuda else scales, "scales")     # (a column of ground_scale's rows: packed here)
    L.check(h_.mcav_eval_depth_scaled(L.ptr(gt), L.ptr(disp), B, Hg, Wg, h, w, L.ptr(meta), L.c_p(meta.data_ptr() + 4 * 2 * B),
                                      float(min_depth), float(max_depth), float(scale), L.ptr(scales), flags, L.ptr(rows), L.ptr(ws),
                                      ws.numel(), L.stream()), "mcav_eval_depth_scaled")
    return rows


def reduce_rows(rows, ground=None):
    """Per-image rows (one [B, 11] tensor or a list of them, e.g. one per batch) -> the protocol's result: the mean of every metric over
    the images with count > 0, 'images', the total pixel 'count', and monodepth2's scale statistics 'ratio_median' = median(ratios),
    'ratio_std' = std(ratios / ratio_median).  The rows are joined on the device and read back once.
    ground: the rows [B, 4] of pseudo_lidar.ground_scale for the same images (or a list of them), when its scales were used: adds
    'ground_scale_mean' and 'ground_scale_std' over the images the estimator accepted (status 1) and 'ground_fallbacks', the others."""
    import numpy as np
    if isinstance(rows, (list, tuple)):
        rows = torch.cat(list(rows)) if rows else torch.empty((0, 11))
    r = rows.detach().cpu().numpy().astype(np.float64).reshape(-1, 11)
    valid = r[:, 9] > 0
    out = {k: float(np.mean(r[valid, i])) if valid.any() else float("nan") for i, k in enumerate(KEYS)}
    out["images"] = int(valid.sum())
    out["count"] = int(r[valid, 9].sum())
    ratios = r[valid, 10]
    med = float(np.median(ratios)) if ratios.size else float("nan")
    out["ratio_median"] = med
    out["ratio_std"] = float(np.std(ratios / med)) if ratios.size else float("nan")
    if ground is not None:
        if isinstance(ground, (list, tuple)):
            ground = torch.cat(list(ground)) if ground else torch.empty((0, 4))
        g = ground.detach().cpu().numpy().astype(np.float64).reshape(-1, 4)
        ok = g[:, 3] > 0
        out["ground_scale_mean"] = float(np.mean(g[ok, 0])) if ok.any() else float("nan")
        out["ground_scale_std"] = float(np.std(g[ok, 0])) if ok.any() else float("nan")
        out["ground_fallbacks"] = int((~ok).sum())
    return out


def evaluate_depth(gt, pred, sizes=None, crop="garg", min_depth=1e-3, max_depth=80.0, median_scaling=True, scale=1.0, per_image=False,
                   scales=None):
    """The KITTI depth protocol (monodepth2 evaluate_depth.py) on the GPU.
    gt: [B,1,Hg,Wg] or [B,Hg,Wg] ground-truth depth in metres (0 = no return), zero-padded to the batch's largest image; pred: the
    network's sigmoid disparity as compute_errors takes it ([B,1,h,w] / [B,h,w], or a list whose first entry it is).  sizes: the true
    (Hb, Wb) of every image (host; default: (Hg, Wg)).  crop: 'garg', 'eigen', None, an explicit (y0, y1, x0, x1) or a list of B of
    them.  scale: monodepth2's pred_depth_scale_factor; scales: a float32 tensor [B] on the GPU, one more factor per image.  -> the dict of reduce_rows; with per_image=True also the [B, 11] device rows."""
    rows = eval_depth_rows(gt, pred, sizes, crop, min_depth, max_depth, median_scaling, scale, scales)
    out = reduce_rows(rows)
    return (out, rows) if per_image else out
