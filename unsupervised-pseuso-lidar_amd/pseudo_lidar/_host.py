"""What the pseudo-LiDAR stages share on the host, each written once: the argument normalisers, the calibration table (bytes, pointers to
its parts, cached upload), the workspace an object keeps, the offsets of a batch with their one read-back, and the recorded call that
makes a stage a node of the autograd graph.  The table, as mcav_pl_batch_project(_bwd) and mcav_ground_scale read it: the calibration,
B x 28 float64 (P in 12, T in 16 or zeros); then the sizes, B x (H, W) int32; then, optionally, the boxes, B x (y0, y1, x0, x1) int32.
"""
import weakref

import numpy as np
import torch

from mcav import lib as L


def _plane(m, what):
    """[B, h, w] or [B, 1, h, w] float32 on the GPU -> [B, h, w], contiguous"""
    if not torch.is_tensor(m):
        raise L.MCAVError("%s: m must be a tensor on the GPU" % what)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3:
        raise L.MCAVError("%s: m must be [B, h, w] or [B, 1, h, w], got %s" % (what, tuple(m.shape)))
    return L.dev(m.contiguous() if m.is_cuda else m, "m")


def _sizes(sizes, B, h, w, what):
    sz = np.asarray([(h, w)] * B if sizes is None else (sizes.cpu() if torch.is_tensor(sizes) else sizes), dtype=np.int32).reshape(-1, 2)
    if sz.shape[0] != B or (sz < 1).any():
        raise L.MCAVError("%s: sizes must be %d positive (H, W) pairs, got %r" % (what, B, sz.tolist()))
    return sz


def _matrices(M, B, shape, refusal):
    """one matrix or B of them (host values or a tensor) -> float64 [B, *shape]; what does not broadcast is refused with `refusal`"""
    try:
        return np.broadcast_to(np.asarray(M.cpu() if torch.is_tensor(M) else M, dtype=np.float64), (B,) + shape)
    except ValueError:
        raise L.MCAVError(refusal)


def pack_table(P, T, sizes, box=None):
    """The table's bytes from host arrays: P [3, 4] or [B, 3, 4], T likewise or None, sizes B pairs, box 4 ints or B of them or None"""
    sz = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 2)
    calib = np.zeros((len(sz), 7, 4), np.float64)
    calib[:, :3] = P
    if T is not None:
        calib[:, 3:] = T
    return calib.tobytes() + sz.tobytes() + (b"" if box is None else np.broadcast_to(np.asarray(box, dtype=np.int32), (len(sz), 4)).tobytes())


table_calib = L.ptr                            # the pointers to the three parts of a table of B images, as the C entries take them


def table_sizes(table, B):
    return L.c_p(table.data_ptr() + 224 * B)


def table_box(table, B):
    return L.c_p(table.data_ptr() + 232 * B)


def upload(holder, data, dev):
    """`data` (bytes) on the device, kept on the holder: the same bytes again (a replayed capture's warm-up) copy nothing; new ones go
    through one pinned buffer in one copy, made here and not inside the C call"""
    if holder._uploaded_bytes != data:
        holder._uploaded = torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)
        holder._uploaded_bytes = data
    return holder._uploaded


def grown(buf, nbytes, dev):
    """the workspace an object keeps (a captured call reuses it with out=): `buf` unless there is none or it is smaller than nbytes"""
    return buf if buf is not None and buf.numel() >= nbytes else torch.empty(nbytes, dtype=torch.uint8, device=dev)


class OffsetBatch:
    """`offsets` int32 [B + 1] on the device: image b owns rows offsets[b]:offsets[b+1] of the batch's buffers.  Rows beyond their capacity
    were not written (offsets stay exact).  Nothing is read back until asked."""

    def __init__(self, batch, device):
        self.offsets = torch.zeros(int(batch) + 1, dtype=torch.int32, device=device)
        self._host = None

    def __len__(self):
        return self.offsets.numel() - 1

    def counts(self):
        """offsets on the host (numpy int64 [B + 1]): the one read-back of the batch, kept until the next call into this object."""
        if self._host is None:
            self._host = self.offsets.cpu().numpy().astype(np.int64)
        return self._host

    def ranges(self, capacity):
        """-> B pairs (lo, hi), the rows of every image, clipped to the capacity"""
        o = np.minimum(self.counts(), capacity).tolist()
        return list(zip(o[:-1], o[1:]))


class _Recorded(torch.autograd.Function):
    """A stage as one node of the autograd graph: forward is the indexed call into the holder's buffers (the output returned as a new tensor
    on the same memory), backward the stage's plain backward on what that call recorded.  The node holds tensors, not the holder (which
    holds the node through its output); autograd refuses an in-place change of a saved tensor before backward, the stamp a refilled holder."""

    @staticmethod
    def forward(ctx, x, call):
        holder, out, idx, saved, run, ctx.bwd, ctx.again = call
        ctx.fwd, ctx.stamp, ctx.owner = holder._fwd, holder._stamp, weakref.ref(holder)
        run(idx)
        ctx.save_for_backward(*saved, idx)
        return out.detach()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        ctx.saved_tensors                                    # the version check
        holder = ctx.owner()
        if holder is not None and holder._stamp != ctx.stamp:
            raise L.MCAVError(ctx.again)
        return ctx.bwd(ctx.fwd, grad.to(torch.float32).contiguous(), None), None


def recorded(x, holder, out, idx, index_shape, provenance, run, record, saved, backward, again):
    """One call of a stage into `holder` (a CloudBatch, a PillarBatch) -> (out, idx), its output and int32 index tensors as the holder is
    to keep them.  x: the input a gradient may flow to; out, idx: the two as the holder has them; run(idx): the C call (it fills idx
    unless None); record(idx): what `backward(record, grad, None)` reads -- tensors and numbers, not the holder; saved: the tensors
    besides idx that must hold what they hold until backward; again: what a backward says whose holder was filled again.  With grad mode
    on and an x that requires a gradient out is a node of the graph; with that or `provenance` idx is filled and holder._fwd is the record."""
    wants_grad = torch.is_grad_enabled() and x.requires_grad
    if out.grad_fn is not None:
        out = out.detach()                                   # an earlier differentiable call's node: the buffer itself
    if not (wants_grad or provenance):
        idx = None                                           # nothing fills them in this call
    elif idx is None or tuple(idx.shape) != index_shape:
        idx = torch.empty(index_shape, dtype=torch.int32, device=out.device)
    holder._fwd = record(idx) if idx is not None else None
    holder._stamp += 1
    if wants_grad:
        return _Recorded.apply(x, (holder, out, idx, saved, run, backward, again)), idx
    run(idx)
    return out, idx
