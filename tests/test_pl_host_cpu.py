"""CPU: the host protocol the pseudo-LiDAR stages share (pseudo_lidar/_host.py), without a kernel or a library call: the calibration
table's bytes and the pointers to its parts against a literal restatement of the layout the C entries read; the offsets of a batch, their
one cached read-back and the clipped ranges under CloudBatch and PillarBatch; the recorded call on CPU tensors with a stand-in stage."""
import ctypes
import gc
import weakref

import numpy as np
import pytest
import torch

import mcav.lib as L
from pseudo_lidar import CloudBatch, PillarBatch
from pseudo_lidar import _host as H


# ---------------------------------------------------------------------------------------------- the calibration table
B = 3
RNG = np.random.default_rng(11)
P, T = RNG.standard_normal((B, 3, 4)), RNG.standard_normal((B, 4, 4))
SIZES = [(375, 1242), (370, 1224), (376, 1241)]
BOX = [(100, 190, 200, 440), (96, 192, 0, 640), (1, 2, 3, 4)]


def restated(P, T, sizes, box):
    """28 float64 per image (P in 12, T in 16), then the (H, W) int32 pairs, then the (y0, y1, x0, x1) int32 quadruples"""
    calib = np.zeros((B, 28), np.float64)
    for b in range(B):
        calib[b, :12] = np.asarray(P[b], np.float64).reshape(12)
        if T is not None:
            calib[b, 12:] = np.asarray(T[b], np.float64).reshape(16)
    data = calib.tobytes() + np.asarray(sizes, np.int32).tobytes()
    return data if box is None else data + np.asarray(box, np.int32).tobytes()


def test_table_bytes_are_the_layout_the_entries_read():
    data = H.pack_table(P, T, SIZES, BOX)
    assert isinstance(data, bytes) and len(data) == (224 + 8 + 16) * B
    assert data == restated(P, T, SIZES, BOX)
    assert H.pack_table(P, T, SIZES) == restated(P, T, SIZES, None) == data[:232 * B]                  # no box: no third part
    ground = H.pack_table(P, None, SIZES, BOX)                                                         # ground_scale's form: 16 zeros
    assert ground == restated(P, None, SIZES, BOX)
    assert np.frombuffer(ground[:224 * B], np.float64).reshape(B, 28)[:, 12:].tobytes() == bytes(128 * B)
    # one matrix, one box for the batch: the bytes of B copies
    assert H.pack_table(P[0], T[1], SIZES, BOX[2]) == restated([P[0]] * B, [T[1]] * B, SIZES, [BOX[2]] * B)
    assert H.pack_table(P[0], None, SIZES) == restated([P[0]] * B, None, SIZES, None)
    for bad in (dict(P=P[:2]), dict(T=T[:2]), dict(box=BOX[:2]), dict(box=(1, 2, 3))):                 # what is not 1 or B of them
        with pytest.raises(ValueError):
            H.pack_table(**dict(dict(P=P, T=T, sizes=SIZES, box=BOX), **bad))


def test_table_accessors_point_at_the_parts():
    table = torch.frombuffer(bytearray(H.pack_table(P, T, SIZES, BOX)), dtype=torch.uint8)
    base = table.data_ptr()
    calib, sizes, box = H.table_calib(table), H.table_sizes(table, B), H.table_box(table, B)
    assert all(isinstance(p, ctypes.c_void_p) for p in (calib, sizes, box))
    assert (calib.value, sizes.value, box.value) == (base, base + 224 * B, base + 232 * B)
    read = lambda p, ctype, n: np.ctypeslib.as_array((ctype * n).from_address(p.value))
    assert read(calib, ctypes.c_double, 28 * B).reshape(B, 28)[:, :12].tobytes() == P.tobytes()
    assert read(sizes, ctypes.c_int32, 2 * B).reshape(B, 2).tolist() == [list(s) for s in SIZES]
    assert read(box, ctypes.c_int32, 4 * B).reshape(B, 4).tolist() == [list(b) for b in BOX]


# ---------------------------------------------------------------------------------------------- the offsets of a batch
def test_offset_batch_counts_once_and_clips():
    cloud = CloudBatch(2, 5, "cpu")
    assert len(cloud) == 2 and cloud.points.shape == (5, 4)
    cloud.offsets.copy_(torch.tensor([0, 3, 9], dtype=torch.int32))
    counts = cloud.counts()
    assert counts.dtype == np.int64 and counts.tolist() == [0, 3, 9]
    cloud.offsets.zero_()
    assert cloud.counts() is counts and counts.tolist() == [0, 3, 9]                                   # the one read-back, kept
    assert cloud.ranges(5) == [(0, 3), (3, 5)]
    parts = cloud.split()
    assert [p.shape[0] for p in parts] == [3, 2] and parts[1].data_ptr() == cloud.points[3:].data_ptr()
    with pytest.raises(L.MCAVError, match="2 clouds"):
        cloud.save_bin(["a"])
    with pytest.raises(L.MCAVError, match="9 points, the buffer holds 5"):
        cloud.save_bin(["a", "b"])
    pillars = PillarBatch(2, 5, 3, 4, "cpu")
    assert len(pillars) == 2 and pillars._host is None
    pillars.offsets.copy_(torch.tensor([0, 3, 9], dtype=torch.int32))
    assert pillars.counts().tolist() == [0, 3, 9] and pillars._host is pillars.counts()
    assert pillars.ranges(5) == [(0, 3), (3, 5)]
    rows = pillars.split()
    assert [tuple(t.shape[0] for t in r) for r in rows] == [(3, 3, 3), (2, 2, 2)]
    assert rows[1][0].shape == (2, 3, 4) and rows[1][1].data_ptr() == pillars.coords[3:].data_ptr()
    with pytest.raises(L.MCAVError, match="9 pillars, the buffers hold 5"):
        pillars.save_npz(["a", "b"])


# ---------------------------------------------------------------------------------------------- the recorded call
AGAIN = "backward: the Holder was filled again after this forward"


class Holder:
    def __init__(self):
        self.out, self.idx, self._fwd, self._stamp = torch.zeros(4), None, None, 0


def stage(x, holder, provenance=False):
    """a stand-in stage: out = 3 x, written behind autograd's back as a kernel does; its backward is 3 grad, from the record"""
    fixed = torch.arange(4, dtype=torch.int32)

    def run(idx):
        holder.out.detach().numpy()[:] = 3.0 * x.detach().numpy()
        if idx is not None:
            idx.numpy()[:] = [3, 2, 1, 0]

    def backward(record, grad, out):
        assert out is None and record["idx"].tolist() == [3, 2, 1, 0] and record["fixed"] is fixed
        return record["factor"] * grad

    holder.out, holder.idx = H.recorded(x, holder, holder.out, holder.idx, index_shape=(4,), provenance=provenance, run=run, saved=(x, fixed),
                                        record=lambda idx: dict(factor=3.0, fixed=fixed, idx=idx), backward=backward, again=AGAIN)
    return holder


def test_recorded_call_node_holds_tensors_not_the_holder():
    x = torch.tensor([1.0, 2.0, 3.0, 4.0], requires_grad=True)
    y = stage(x, Holder()).out
    assert y.grad_fn is not None and y.tolist() == [3.0, 6.0, 9.0, 12.0]
    holder = stage(x, Holder())
    y, ref = holder.out, weakref.ref(holder)
    assert holder.idx.tolist() == [3, 2, 1, 0] and holder._fwd["idx"] is holder.idx and holder._stamp == 1
    gc.disable()
    try:
        del holder
        assert ref() is None                                       # freed by reference counting alone, the output still alive
    finally:
        gc.enable()
    (y * torch.tensor([1.0, 10.0, 100.0, 1000.0])).sum().backward()
    assert x.grad.tolist() == [3.0, 30.0, 300.0, 3000.0]


def test_recorded_call_refuses_a_refilled_holder_and_a_changed_input():
    x = torch.ones(4, requires_grad=True)
    holder = stage(x, Holder())
    first, buffer = holder.out, holder.out.data_ptr()
    stage(x, holder)
    assert holder._stamp == 2 and holder.out is not first and holder.out.data_ptr() == buffer          # a new node on the same buffer
    with pytest.raises(L.MCAVError, match=AGAIN):
        first.sum().backward()
    holder.out.sum().backward()                                    # the second node is the live one
    assert x.grad.tolist() == [3.0] * 4
    plane = x * 1.0
    loss = stage(plane, Holder()).out.sum()
    plane.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_recorded_call_without_a_gradient_records_nothing():
    x = torch.ones(4, requires_grad=True)
    with torch.no_grad():
        quiet = stage(x, Holder())
    assert quiet.out.grad_fn is None and quiet.idx is None and quiet._fwd is None and quiet.out.tolist() == [3.0] * 4
    plain = stage(torch.ones(4), Holder())                         # grad mode on, nothing to differentiate
    assert plain.out.grad_fn is None and plain.idx is None and plain._fwd is None and plain._stamp == 1
    kept = stage(torch.ones(4), Holder(), provenance=True)         # provenance: the record without a node
    assert kept.out.grad_fn is None and kept.idx.tolist() == [3, 2, 1, 0] and kept._fwd["factor"] == 3.0
    live = stage(x, Holder())
    buffer = live.out.data_ptr()
    stage(torch.ones(4), live)                                     # an object that carried a graph goes back to its plain buffer
    assert live.out.grad_fn is None and live.out.data_ptr() == buffer and live.idx is None and live._fwd is None
