"""Oriented 3-D boxes on the GPU: overlap and batched non-maximum suppression, what follows a detector's head on the pseudo-image
(include/mcav_depth.h: mcav_box_iou, mcav_box_nms; OpenPCDet / second.pytorch iou3d_nms: boxes_iou_bev, boxes_iou3d, nms_gpu).

A box is 7 float32 (x, y, z, dx, dy, dz, heading): the centre, dx along the heading, the heading a rotation about +z, counter-clockwise
(OpenPCDet's LiDAR frame).  An invalid box (a non-finite number, an extent outside [0.001, 1024] m, |heading| > 32) overlaps nothing and
is never kept.  `nms` runs score threshold -> top pre_max -> greedy suppression for a whole batch in three launches; nothing is read back
until DetectionBatch.counts() is asked."""
import ctypes

import numpy as np
import torch

from mcav import lib as L

from ._host import grown

c_ll = ctypes.c_longlong

L.register({
    "mcav_box_iou": (L.c_i, [L.c_p, c_ll, L.c_p, c_ll, L.c_i, L.c_p, L.c_p]),
    "mcav_box_nms_workspace_bytes": (L.c_sz, [L.c_i, c_ll, L.c_i]),
    "mcav_box_nms": (L.c_i, [L.c_p, L.c_p, L.c_p, L.c_i, c_ll, L.c_f, L.c_f, L.c_i, L.c_i, L.c_i, L.c_p, L.c_p, L.c_p, L.c_p, L.c_p, L.c_sz, L.c_p]),
})

IOU_MODES = {"bev": 0, "3d": 1}            # MCAV_BOX_IOU_BEV, MCAV_BOX_IOU_3D
NMS_MAX_CANDIDATES = 4096                  # MCAV_NMS_MAX_CANDIDATES


def _rows(t, name, what):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 7:
        raise L.MCAVError("%s: %s must be a tensor [n, 7] (x, y, z, dx, dy, dz, heading) on the GPU" % (what, name))
    return L.dev(t, name)


def _iou(a, b, mode, what):
    a, b = _rows(a, "a", what), _rows(b, "b", what)
    if a.device != b.device:
        raise L.MCAVError("%s: a is on %s, b on %s" % (what, a.device, b.device))
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    if out.numel() == 0:                                     # an empty tensor has no address to hand over
        return out
    with torch.cuda.device(a.device):
        L.check(L.lib().mcav_box_iou(L.ptr(a), a.shape[0], L.ptr(b), b.shape[0], mode, L.ptr(out), L.stream()), "mcav_box_iou")
    return out


def boxes_iou_bev(a, b):
    """a [Na, 7], b [Nb, 7] float32 on the GPU -> [Na, Nb] float32: the overlap of the boxes' bird's-eye-view rectangles, intersection over
    union, never above 1 (mcav_box_iou)."""
    return _iou(a, b, IOU_MODES["bev"], "boxes_iou_bev")


def boxes_iou3d(a, b):
    """a [Na, 7], b [Nb, 7] float32 on the GPU -> [Na, Nb] float32: the overlap of the boxes' volumes (the bird's-eye-view intersection
    times the shared height), intersection over union (mcav_box_iou)."""
    return _iou(a, b, IOU_MODES["3d"], "boxes_iou3d")


class DetectionBatch:
    """What nms fills and keeps, on the device: `keep` int32 [B, post_max] (the kept rows' anchor indices in the order kept, -1 behind the
    count), `num` int32 [B], `boxes` [B, post_max, 7] and `scores` [B, post_max] float32 (+0.0 behind the count), `labels` int64
    [B, post_max] when the scores came per class (the class of each kept row, -1 behind the count; else None), and the call's workspace."""

    def __init__(self, batch, post_max, device):
        B, post_max = int(batch), int(post_max)
        self.keep = torch.empty((B, post_max), dtype=torch.int32, device=device)
        self.num = torch.empty((B,), dtype=torch.int32, device=device)
        self.boxes = torch.empty((B, post_max, 7), dtype=torch.float32, device=device)
        self.scores = torch.empty((B, post_max), dtype=torch.float32, device=device)
        self.labels = None
        self._ws, self._host = None, None

    def __len__(self):
        return self.num.numel()

    def counts(self):
        """num on the host (numpy int64 [B]): the one read-back of the batch, kept until the next call into this object."""
        if self._host is None:
            self._host = self.num.cpu().numpy().astype(np.int64)
        return self._host

    def split(self):
        """-> per image a dict(keep, boxes, scores, labels) of the kept rows (views of the batch's buffers; labels None without classes)"""
        return [dict(keep=self.keep[b, :n], boxes=self.boxes[b, :n], scores=self.scores[b, :n],
                     labels=None if self.labels is None else self.labels[b, :n]) for b, n in enumerate(self.counts().tolist())]


def nms(boxes, scores, classes=None, score_thresh=0.1, iou_thresh=0.01, pre_max=4096, post_max=500, iou="bev", out=None):
    """Batched score threshold -> top pre_max -> greedy rotated suppression on the device (mcav_box_nms) -> DetectionBatch.  The defaults
    are OpenPCDet's PointPillars-KITTI post-processing.
    boxes [B, A, 7] and scores [B, A] float32 on the GPU.  scores [B, A, K] (per class) is reduced with max / argmax first; the argmax
    comes back as `labels` of the kept rows and does not separate the classes unless it is also passed as `classes`.
    classes: None, or int32 [B, A]: only kept rows of the same class suppress a row.
    A row is a candidate when its box is valid and score >= score_thresh; the first pre_max by (score descending, index ascending) are
    walked in that order and one is kept iff no earlier kept one (of its class) has iou > iou_thresh with it, until post_max are kept.
    iou: "bev" or "3d".  Nothing is read back.  out: a DetectionBatch to reuse with its workspace (needed under graph capture)."""
    if not torch.is_tensor(boxes) or not torch.is_tensor(scores):
        raise L.MCAVError("nms: boxes and scores must be tensors on the GPU")
    if boxes.dim() != 3 or boxes.shape[2] != 7 or boxes.shape[0] < 1 or boxes.shape[1] < 1:
        raise L.MCAVError("nms: boxes must be [B, A, 7], got %s" % (tuple(boxes.shape),))
    B, A = boxes.shape[:2]
    if scores.dim() not in (2, 3) or tuple(scores.shape[:2]) != (B, A) or (scores.dim() == 3 and scores.shape[2] < 1):
        raise L.MCAVError("nms: scores must be [%d, %d] or [%d, %d, K], got %s" % (B, A, B, A, tuple(scores.shape)))
    if iou not in IOU_MODES:
        raise L.MCAVError("nms: iou must be 'bev' or '3d', got %r" % (iou,))
    pre_max, post_max, score_thresh, iou_thresh = int(pre_max), int(post_max), float(score_thresh), float(iou_thresh)
    if not 1 <= post_max <= pre_max <= NMS_MAX_CANDIDATES:
        raise L.MCAVError("nms: 1 <= post_max <= pre_max <= %d is required, got post_max=%d pre_max=%d" % (NMS_MAX_CANDIDATES, post_max, pre_max))
    if np.isnan(score_thresh) or np.isnan(iou_thresh):
        raise L.MCAVError("nms: the thresholds must not be NaN")
    boxes = L.dev(boxes, "boxes")
    dev = boxes.device
    if classes is not None:
        if not torch.is_tensor(classes) or tuple(classes.shape) != (B, A):
            raise L.MCAVError("nms: classes must be int32 [%d, %d]" % (B, A))
        if L.dev(classes, "classes", torch.int32).device != dev:
            raise L.MCAVError("nms: classes is on %s, boxes on %s" % (classes.device, dev))
    if L.dev(scores, "scores").device != dev:
        raise L.MCAVError("nms: scores is on %s, boxes on %s" % (scores.device, dev))
    label_of = None
    if scores.dim() == 3:
        scores, label_of = scores.max(dim=2)
        scores = scores.contiguous()
    if out is None:
        out = DetectionBatch(B, post_max, dev)
    elif not isinstance(out, DetectionBatch) or tuple(out.keep.shape) != (B, post_max) or out.keep.device != dev:
        raise L.MCAVError("nms: out must be a DetectionBatch of %d images and post_max %d on %s" % (B, post_max, dev))
    hl = L.lib()
    nbytes = hl.mcav_box_nms_workspace_bytes(B, A, pre_max)
    if nbytes == 0:
        raise L.MCAVError("nms: %d images of %d anchors are refused (B <= 65535, B * A < 2^31)" % (B, A))
    ws = out._ws = grown(out._ws, nbytes, dev)
    out._host = None
    with torch.cuda.device(dev):
        L.check(hl.mcav_box_nms(L.ptr(boxes), L.ptr(scores), L.ptr(classes), B, A, score_thresh, iou_thresh, IOU_MODES[iou], pre_max, post_max,
                                L.ptr(out.keep), L.ptr(out.num), L.ptr(out.boxes), L.ptr(out.scores), L.ptr(ws), ws.numel(), L.stream()),
                "mcav_box_nms")
    if label_of is None:
        out.labels = None
    else:
        picked = torch.gather(label_of, 1, out.keep.clamp(min=0).to(torch.int64))
        labels = torch.where(out.keep >= 0, picked, torch.full_like(picked, -1))
        if out.labels is not None and out.labels.shape == labels.shape:
            out.labels.copy_(labels)                         # the same buffer again: a captured call replays into it
        else:
            out.labels = labels
    return out
