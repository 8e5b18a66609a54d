"""TEST INFRASTRUCTURE: the KITTI depth evaluation protocol restated in numpy / torch-CPU -- the yardstick of mcav_eval_depth and
evaluate.evaluate_depth.  It restates monodepth2's evaluate_depth.py (and monodepth's evaluation_utils.py, where the crops come from):

For image b with true ground-truth size (Hb, Wb), gt in metres (0 = no return) and the network's sigmoid disparity disp[b] (h x w):
  1. up   = disp[b] resized to (Hb, Wb): F.interpolate(mode="bilinear", align_corners=False)
  2. pred = 1 / (10 up + 0.01), float32 with each operation rounded (this repository's disp_to_depth); pred *= scale
  3. mask = (gt > min_depth) & (gt < max_depth) & box, box the half-open [y0, y1) x [x0, x1) of crop_box()
  4. median scaling: ratio = median(gt[mask]) / median(pred[mask]) (np.median on float32, ratio in float32); pred *= ratio
  5. pred = clip(pred, min_depth, max_depth)
  6. the metrics of evaluate.KEYS over the mask (sq_rel the squared-relative error, silog = 100 sqrt(mean(e^2) - mean(e)^2))
  7. the mean of every metric over the images with count > 0; images, total count, ratio_median = median(ratios),
     ratio_std = std(ratios / ratio_median)
An image without a valid pixel gets a NaN row (count 0) and is left out of the means.  min_depth / max_depth act as float32 values, as
numpy compares and clips a float32 array with them.  Metrics are float64 over the float32 gt and pred.
"""
import numpy as np
import torch

KEYS = ("silog", "abs_rel", "log10", "rms", "sq_rel", "log_rms", "d1", "d2", "d3")
ROW_KEYS = KEYS + ("count", "ratio")
CROPS = {"garg": (0.40810811, 0.99189189, 0.03594771, 0.96405229),
         "eigen": (0.3324324, 0.91351351, 0.0359477, 0.96405229)}


def crop_box(Hb, Wb, crop):
    """-> (y0, y1, x0, x1): 'garg' / 'eigen' fractions of the true size (float64 products, truncated), None = the whole image, or an
    explicit (y0, y1, x0, x1)."""
    if crop is None:
        return (0, Hb, 0, Wb)
    if isinstance(crop, str):
        fy0, fy1, fx0, fx1 = CROPS[crop]
        return (int(fy0 * Hb), int(fy1 * Hb), int(fx0 * Wb), int(fx1 * Wb))
    return tuple(int(v) for v in crop)


def upsample(disp, Hb, Wb):
    """step 1: float32 [h, w] -> [Hb, Wb]"""
    t = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float32))[None, None]
    return torch.nn.functional.interpolate(t, size=(Hb, Wb), mode="bilinear", align_corners=False)[0, 0].numpy()


def depth_of(up, scale=1.0):
    """step 2, numpy float32"""
    up = np.asarray(up, dtype=np.float32)
    return (np.float32(1) / (np.float32(10) * up + np.float32(0.01))) * np.float32(scale)


def metrics(g, p):
    """step 6: float32 arrays of the masked pixels -> the nine metrics (float64)"""
    g, p = np.asarray(g, np.float64), np.asarray(p, np.float64)
    thresh = np.maximum(g / p, p / g)
    e = np.log(p) - np.log(g)
    var = np.mean(e ** 2) - np.mean(e) ** 2
    return {"silog": 100.0 * np.sqrt(max(var, 0.0) if not np.isnan(var) else var),
            "abs_rel": np.mean(np.abs(g - p) / g),
            "log10": np.mean(np.abs(np.log10(p) - np.log10(g))),
            "rms": np.sqrt(np.mean((g - p) ** 2)),
            "sq_rel": np.mean((g - p) ** 2 / g),
            "log_rms": np.sqrt(np.mean((np.log(g) - np.log(p)) ** 2)),
            "d1": np.mean(thresh < 1.25), "d2": np.mean(thresh < 1.25 ** 2), "d3": np.mean(thresh < 1.25 ** 3)}


def image_row(gt, disp, box, min_depth=1e-3, max_depth=80.0, median_scaling=True, scale=1.0, with_medians=False):
    """One image: gt float32 [Hb, Wb] (its true size), disp float32 [h, w] -> row [11] float64 (KEYS, count, ratio)."""
    gt = np.asarray(gt, dtype=np.float32)
    Hb, Wb = gt.shape
    lo, hi = np.float32(min_depth), np.float32(max_depth)
    pred = depth_of(upsample(disp, Hb, Wb), scale)
    y0, y1, x0, x1 = box
    inbox = np.zeros((Hb, Wb), bool)
    inbox[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
    mask = (gt > lo) & (gt < hi) & inbox
    g, p = gt[mask], pred[mask]
    row = np.full(11, np.nan)
    row[9] = g.size
    med = (np.float32(np.nan), np.float32(np.nan))
    if g.size == 0:
        return (row, med) if with_medians else row
    ratio = np.float32(1)
    if median_scaling:
        med = (np.float32(np.median(g)), np.float32(np.median(p)))
        ratio = np.float32(med[0] / med[1])
        p = p * ratio
    p = np.clip(p, lo, hi)
    m = metrics(g, p)
    row[:9] = [m[k] for k in KEYS]
    row[10] = ratio
    return (row, med) if with_medians else row


def reduce_rows(rows):
    """step 7: rows [N, 11] -> the mean dict"""
    rows = np.asarray(rows, np.float64).reshape(-1, 11)
    valid = rows[:, 9] > 0
    out = {k: float(np.mean(rows[valid, i])) if valid.any() else float("nan") for i, k in enumerate(KEYS)}
    out["images"] = int(valid.sum())
    out["count"] = int(rows[valid, 9].sum())
    r = rows[valid, 10]
    med = float(np.median(r)) if r.size else float("nan")
    out["ratio_median"] = med
    out["ratio_std"] = float(np.std(r / med)) if r.size else float("nan")
    return out


def evaluate(gt, disp, sizes=None, crop="garg", min_depth=1e-3, max_depth=80.0, median_scaling=True, scale=1.0):
    """gt [B, Hg, Wg] (padded) float32, disp [B, h, w]; sizes [(Hb, Wb)] (default: the padded size); crop: see crop_box, or a list of B
    explicit boxes.  -> (mean dict, rows [B, 11])"""
    gt = np.asarray(gt, np.float32).reshape(-1, *np.shape(gt)[-2:])
    disp = np.asarray(disp, np.float32).reshape(gt.shape[0], *np.shape(disp)[-2:])
    B, Hg, Wg = gt.shape
    sizes = [(Hg, Wg)] * B if sizes is None else [tuple(int(v) for v in s) for s in sizes]
    rows = []
    for b in range(B):
        Hb, Wb = sizes[b]
        c = crop[b] if isinstance(crop, (list, tuple)) and len(crop) == B and isinstance(crop[0], (list, tuple)) else crop
        rows.append(image_row(gt[b, :Hb, :Wb], disp[b], crop_box(Hb, Wb, c), min_depth, max_depth, median_scaling, scale))
    rows = np.stack(rows)
    return reduce_rows(rows), rows
