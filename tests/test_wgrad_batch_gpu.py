"""GPU: the batched weight-gradient slab reduction at the ABI (include/mcav_conv.h: mcav_wgrad_deferred + mcav_wgrad_reduce_plan +
mcav_wgrad_reduce_multi), the path every weight gradient of a backward pass takes, on the bucket of tests/wgrad_batch_cases.py.

  1. batched == per-layer, bit for bit: the header promises "the per-layer kernels' bodies and summation order (bit-identical gradients)".  Each
     descriptor runs through mcav_wgrad and again through the deferred GEMM + ONE table + ONE mcav_wgrad_reduce_multi, in three launch orders;
     gradients live in guarded windows that start as NaN sentinels (tests/guarded.py), so a workgroup that lands on the wrong item, skips its
     item or reads another item's LDS size shows as a differing or unwritten element of that item.
  2. the reduction alone, on slabs the test writes: independent of any GEMM, against the float64 sum over the splits mapped to OIHW; bound
     derived from the summation order, not tuned.
  3. through the product's own plumbing (mcav.nn.WGRAD_BATCH / WGRAD_SIDE inside a backward pass of both networks): every parameter gradient is
     bit-equal with the batch and the side stream on or off.

Tolerances: bit equality between the two paths; the derived bound of test 2; against float64 the suite's existing bars for mcav_wgrad (5e-5; below
3e-6 for the split form; the bf16 form against its rounded-operand reference at 5e-5: tests/test_conv_contract_gpu.py)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import wgrad_batch_cases as C
from conftest import rel_err
from guarded import Guarded, P, band_for, is_sentinel, same_bits
from test_bf16_gpu import ref_conv64
from test_conv_contract_gpu import dev_nhwc, wgrad_desc, wgrad_operands

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                   # unit roundoff of float32


def window(shape, init=None):
    return Guarded(shape, init=init, band=band_for(shape))


class Operands:
    """Per case: the stored source and dy on the device, the float64 gradients of the case's input-channel window, and start values for the
    accumulating runs.  Computed once for the module and never modified."""

    def __init__(self):
        self.x, self.dy, self.want_w, self.want_b, self.start_w, self.start_b = {}, {}, {}, {}, {}, {}
        g = torch.Generator().manual_seed(404)
        for i, c in enumerate(C.BUCKET):
            if c.share is None:
                x, dy, ww, wb = wgrad_operands(c)
                self.x[i], self.dy[i], self.want_w[i], self.want_b[i] = x, dev_nhwc(dy), ww, wb
        dec = [i for i, c in enumerate(C.BUCKET) if c.share == "dec"]
        (isk, sk), (ium, um) = [(i, C.BUCKET[i]) for i in dec]
        assert (sk.upm, um.upm) == (0, 1) and sk.ci_offset == um.conv[3] and um.ci_offset == 0
        B, H, W, C2, Cout = sk.conv[:5]
        C1 = um.conv[3]
        a, skip = torch.randn(B, C1, H // 2, W // 2, generator=g), torch.randn(B, C2, H, W, generator=g)
        dy = torch.randn(B, Cout, H, W, generator=g)
        wr = torch.zeros(Cout, C1 + C2, 3, 3, dtype=torch.float64).requires_grad_()
        ref_conv64(torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), skip], 1), wr, None, 1, 1, 1).backward(dy.double())
        self.x[isk], self.x[ium] = dev_nhwc(skip), dev_nhwc(a)
        self.dy[isk] = self.dy[ium] = dev_nhwc(dy)
        self.want_w[isk], self.want_w[ium] = wr.grad[:, C1:], wr.grad[:, :C1]
        self.want_b[isk] = self.want_b[ium] = dy.double().sum((0, 2, 3))
        for i, c in enumerate(C.BUCKET):
            key = c.share or i
            if key not in self.start_w:
                self.start_w[key] = torch.randn(grad_shape(c), generator=g)
                self.start_b[key] = torch.randn(c.conv[4], generator=g)


def grad_shape(c):
    Cin, Cout, k = c.conv[3], c.conv[4], c.conv[5]
    return (Cout, c.cin_total or Cin, k, k)


@pytest.fixture(scope="module")
def ops():
    return Operands()


class Targets:
    """The gradient windows of one run.  shared: the launches of a decoder level write one tensor (as the product does); else every launch
    has a tensor of its own, so that a store outside its input-channel window lands on a sentinel.  start: initial values (accumulate)."""

    def __init__(self, ops, shared, start):
        self.dw, self.db = {}, {}
        by_key = {}
        for i, c in enumerate(C.BUCKET):
            key = c.share if (shared and c.share) else i
            if key not in by_key:
                sk = c.share or i
                by_key[key] = (window(grad_shape(c), init=ops.start_w[sk] if start else None),
                               window((c.conv[4],), init=ops.start_b[sk] if start else None))
            self.dw[i] = by_key[key][0]
            self.db[i] = by_key[key][1] if c.bias else None
        self.windows = [w for pair in by_key.values() for w in pair]

    def intact(self):
        return all(w.intact() for w in self.windows)


def desc(ops, tg, i, accumulate):
    from mcav import nn as N
    c = C.BUCKET[i]
    d = wgrad_desc(c, ops.x[i], ops.dy[i], c.conv[4], 0, tg.dw[i], tg.db[i], accumulate, c.mma)
    d.upm, d.Cin_total, d.ci_offset = c.upm, c.cin_total, c.ci_offset
    # the descriptor the CPU test asked the planner about, with device addresses in place of its constants
    same = C.plan_desc(N, c, P(ops.x[i]), P(ops.dy[i]), P(tg.dw[i]), P(tg.db[i]), accumulate)
    assert bytes(d) == bytes(same), c.name
    return d


def workspace(d):
    from mcav import lib as L
    nbytes = L.lib().mcav_wgrad_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0 and nbytes % 4 == 0
    return Guarded((nbytes // 4,), band=256), nbytes


def run_per_layer(ops, order, shared, accumulate):
    from mcav import lib as L
    tg = Targets(ops, shared, accumulate)
    wss = []
    for i in order:
        d = desc(ops, tg, i, accumulate)
        ws, nbytes = workspace(d)
        rc = L.lib().mcav_wgrad(ctypes.byref(d), P(ws), nbytes, L.stream())
        assert rc == 0, "%s: mcav_wgrad returned %d" % (C.BUCKET[i].name, rc)
        wss.append(ws)
    torch.cuda.synchronize()
    assert tg.intact() and all(w.intact() for w in wss)
    return tg


def defer(ops, tg, order, accumulate):
    """the GEMMs of the bucket, each into a workspace of exactly mcav_wgrad_workspace_bytes -> (items, workspaces); items as filled"""
    from mcav import lib as L
    from mcav import nn as N
    items, wss = [], []
    for i in order:
        c = C.BUCKET[i]
        d = desc(ops, tg, i, accumulate)
        ws, nbytes = workspace(d)
        it = N.WgradReduceItem()
        rc = L.lib().mcav_wgrad_deferred(ctypes.byref(d), P(ws), nbytes, ctypes.byref(it), L.stream())
        assert rc == 0, "%s: mcav_wgrad_deferred returned %d" % (c.name, rc)
        # what the CPU test derived from the planner's splits, now from the filled item
        assert (it.splits, it.groups, it.per_group) == (c.splits,) + c.groups, (c.name, it.splits, it.groups, it.per_group)
        assert (it.Ktot, it.slabN, it.Kp, it.taps) == (c.slab_taps * c.kp, C.up16(c.conv[4]), c.kp, c.taps_out), c.name
        assert it.elems == (it.Ktot + 1) * it.slabN and it.slab == P(ws) and (it.pre or 0) == (P(ws) + align256(4 * it.splits * it.elems) if it.groups else 0)
        assert (it.dw, it.dbias or 0, it.ci_off, it.cin_total) == (P(tg.dw[i]), P(tg.db[i]) or 0, c.ci_offset, c.cin_total or c.conv[3]), c.name
        items.append(it)
        wss.append(ws)
    return items, wss


def align256(v):
    return (v + 255) // 256 * 256


def reduce_all(items):
    """mcav_wgrad_reduce_plan on the host array, ONE copy of the table to the device, ONE mcav_wgrad_reduce_multi"""
    from mcav import lib as L
    from mcav import nn as N
    n = len(items)
    arr = (N.WgradReduceItem * n)(*items)
    pb, rb, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    assert L.lib().mcav_wgrad_reduce_plan(arr, n, ctypes.byref(pb), ctypes.byref(rb), ctypes.byref(lds)) == 0
    assert pb.value == sum(it.pre_bx * it.groups for it in items) and rb.value == sum(it.red_gx * it.red_gy for it in items)
    assert 0 < lds.value <= 64 * 1024
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    rc = L.lib().mcav_wgrad_reduce_multi(P(table), n, pb.value, rb.value, lds.value, L.stream())
    torch.cuda.synchronize()
    assert rc == 0, "mcav_wgrad_reduce_multi returned %d" % rc
    return table


def run_batched(ops, order, shared, accumulate):
    tg = Targets(ops, shared, accumulate)
    items, wss = defer(ops, tg, order, accumulate)
    reduce_all(items)
    assert tg.intact(), "the batched reduction wrote outside a gradient"
    assert all(w.intact() for w in wss), "a deferred GEMM or the batched reduction wrote outside a workspace"
    return tg


def check_windows(tg, i, what):
    """-> the launch's input-channel window of its gradient; nothing of it left unwritten, nothing outside it written (separate tensors)"""
    c = C.BUCKET[i]
    gw = tg.dw[i].cpu()
    inside = torch.zeros(gw.shape[1], dtype=torch.bool)
    inside[c.ci_offset:c.ci_offset + c.conv[3]] = True
    left = int(is_sentinel(gw[:, inside]).sum())
    assert left == 0, "%s, %s: %d elements of the launch's window were never stored" % (c.name, what, left)
    stray = int((~is_sentinel(gw[:, ~inside])).sum())
    assert stray == 0, "%s, %s: %d elements outside input channels [%d, %d) were stored" % (c.name, what, stray, c.ci_offset, c.ci_offset + c.conv[3])
    if c.bias:
        assert int(is_sentinel(tg.db[i].cpu()).sum()) == 0, "%s, %s: bias gradient elements were never stored" % (c.name, what)
    return gw[:, inside]


def first_difference(a, b):
    bad = (a.view(torch.int32) != b.view(torch.int32)).nonzero()
    return "%d elements differ, the first at %s: %r vs %r" % (len(bad), tuple(bad[0].tolist()), float(a[tuple(bad[0])]), float(b[tuple(bad[0])]))


@pytest.mark.parametrize("order_name", list(C.orders()))
def test_batched_reduction_equals_per_layer_bit_for_bit(ops, order_name):
    order = C.orders()[order_name]
    # accumulate = 0, every launch into a tensor of its own
    per, bat = run_per_layer(ops, order, False, 0), run_batched(ops, order, False, 0)
    for i in order:
        c = C.BUCKET[i]
        gp, gb = check_windows(per, i, "per layer"), check_windows(bat, i, "batched")
        assert same_bits(gb, gp), "%s (position %d of '%s'): dw, %s" % (c.name, order.index(i), order_name, first_difference(gb, gp))
        if c.bias:
            assert same_bits(bat.db[i].cpu(), per.db[i].cpu()), "%s (position %d of '%s'): dbias differs" % (c.name, order.index(i), order_name)
        err = rel_err(gb, ops.want_w[i])
        eb = rel_err(bat.db[i].cpu(), ops.want_b[i]) if c.bias else 0.0
        print("%-10s %-36s dw %.2e dbias %.2e" % (order_name, c.name, err, eb))
        bar = 3e-6 if c.mma >= 2 else 5e-5
        assert err < bar and eb < bar, (c.name, err, eb)
    # the decoder level's two launches into ONE tensor, as the product issues them: overwriting sentinels, then accumulating into initialised
    # windows (a bias among them)
    for acc in (0, 1):
        what = "accumulate" if acc else "overwrite, shared tensor"
        per, bat = run_per_layer(ops, order, True, acc), run_batched(ops, order, True, acc)
        tensors = {}                                         # gradient tensor -> [float64 dw, float64 dbias, per-layer and batched windows, a case]
        for i in order:
            c = C.BUCKET[i]
            key = c.share or i
            if key not in tensors:
                zw, zb = ops.start_w[key].double() * acc, ops.start_b[key].double() * acc
                tensors[key] = [zw.clone(), zb + ops.want_b[i], per.dw[i], bat.dw[i], None, None, c]
            tensors[key][0][:, c.ci_offset:c.ci_offset + c.conv[3]] += ops.want_w[i]
            if c.bias:
                tensors[key][4:6] = per.db[i], bat.db[i]
        for key, (ww, wb, pw, bw, pb, bb, c) in tensors.items():
            assert int(is_sentinel(bw.cpu()).sum()) == 0, "%s, %s: elements of the gradient were never stored" % (c.name, what)
            assert same_bits(bw.cpu(), pw.cpu()), "%s, %s ('%s'): dw, %s" % (c.name, what, order_name, first_difference(bw.cpu(), pw.cpu()))
            bar = 3e-6 if c.mma >= 2 else 5e-5
            assert rel_err(bw.cpu(), ww) < bar, (c.name, what, rel_err(bw.cpu(), ww))
            if bb is not None:
                assert same_bits(bb.cpu(), pb.cpu()), "%s, %s ('%s'): dbias differs" % (c.name, what, order_name)
                assert rel_err(bb.cpu(), wb) < bar, (c.name, what)


# merged tap a of parity class p that filter tap k belongs to (include/mcav_conv.h, mcav_pack_weights_upmerge: S(0,0) = {0}, S(0,1) = {1,2},
# S(1,0) = {0,1}, S(1,1) = {2}), restated: on the upsampled grid an even output row reads low-resolution rows (s - 1, s, s), an odd one (s, s, s + 1)
MERGED_TAP = {0: (0, 1, 1), 1: (0, 0, 1)}


def expected_from_slab(c, slab):
    """slab [splits][Ktot + 1][slabN] float64 -> (sum, sum of magnitudes, terms) of every OIHW element of the window [Cout][Cin][k][k] and the
    same for the bias row.  terms: float32 additions behind one element."""
    Cin, Cout, k = c.conv[3], c.conv[4], c.conv[5]
    Kp, Ktot = c.kp, c.slab_taps * c.kp
    rows, mag = slab.sum(0), slab.abs().sum(0)                       # [Ktot + 1][slabN]

    def oihw(t):
        if not c.upm:
            return t[:Ktot].view(c.taps_out, Kp, -1)[:, :Cin, :Cout].permute(2, 1, 0).reshape(Cout, Cin, k, k)
        m = t[:Ktot].view(2, 2, 2, 2, Kp, -1)                        # [py][px][a][b][ci][co]
        out = torch.zeros(Cout, Cin, 3, 3, dtype=t.dtype)
        for ky in range(3):
            for kx in range(3):
                for py in range(2):
                    for px in range(2):
                        out[:, :, ky, kx] += m[py, px, MERGED_TAP[py][ky], MERGED_TAP[px][kx], :Cin, :Cout].t()
        return out
    groups, per = c.groups
    terms = (per + groups if groups else c.splits) * (4 if c.upm else 1)
    return oihw(rows), oihw(mag), rows[Ktot, :Cout], mag[Ktot, :Cout], terms, per + groups if groups else c.splits


def test_reduction_alone_on_slabs_the_test_writes(ops):
    """After mcav_wgrad_deferred and a synchronize the workspace belongs to the caller until it is reduced: every slab is overwritten with random
    values whose scale differs per split; rows of padding input channels (ci >= Cin), the padding columns (co >= Cout), the group-sum area and
    the alignment gaps are NaN.  Bound per element, from the summation order: terms * 2^-24 * sum |terms|, terms = the additions behind an element
    -- the splits on the single-level path (x 4 classes for the merged-tap half), per_group + groups on the two-level path."""
    order = C.orders()["shuffled"]
    tg = Targets(ops, False, 0)
    items, wss = defer(ops, tg, order, 0)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(77)
    slabs = []
    for i, it, ws in zip(order, items, wss):
        c = C.BUCKET[i]
        Cin, Cout = c.conv[3], c.conv[4]
        slab = torch.randn(it.splits, it.Ktot + 1, it.slabN, generator=g)
        slab *= (10.0 ** torch.linspace(-3, 3, it.splits)[torch.randperm(it.splits, generator=g)]).view(-1, 1, 1)
        body = slab[:, :it.Ktot].view(it.splits, c.slab_taps, it.Kp, it.slabN)
        body[:, :, Cin:, :] = float("nan")
        slab[:, :, Cout:] = float("nan")
        full = torch.full((ws.t.numel(),), float("nan"))
        full[:slab.numel()] = slab.flatten()
        ws.t.copy_(full)
        slabs.append(torch.nan_to_num(slab.double(), nan=0.0))         # (the reference indexes real rows and columns only; zeros elsewhere never enter)
    reduce_all(items)
    assert tg.intact() and all(w.intact() for w in wss)
    for i, slab in zip(order, slabs):
        c = C.BUCKET[i]
        got = check_windows(tg, i, "synthetic slab").double()
        ww, wm, bw, bm, terms, bterms = expected_from_slab(c, slab)
        assert bool(torch.isfinite(got).all()), "%s: NaN in the gradient (the reduction read a padding row, a gap or group sums not yet written)" % c.name
        excess = (got - ww).abs() - terms * U * wm
        worst = float(((got - ww).abs() / (U * wm).clamp_min(1e-300)).max())
        print("%-36s splits %2d groups %s terms %2d: worst error %.2f x 2^-24 sum|terms|" % (c.name, c.splits, c.groups, terms, worst))
        at = tuple(int(v) for v in (excess == excess.max()).nonzero()[0])
        assert float(excess.max()) <= 0.0, "%s: dw%s = %r, the slab sums to %r (bound %g)" % (c.name, at, float(got[at]), float(ww[at]), terms * U * float(wm[at]))
        if c.bias:
            gb = tg.db[i].cpu().double()
            assert bool(torch.isfinite(gb).all()) and bool(((gb - bw).abs() <= bterms * U * bm).all()), "%s: dbias" % c.name


def test_backward_pass_gradients_do_not_depend_on_batch_or_side_stream():
    """Forward + loss + backward of both networks from identical state, four times: N.WGRAD_BATCH.enabled x N.WGRAD_SIDE.enabled.  Every
    parameter gradient must be bit-equal: the batched reduction against the per-layer launches, the duplicate-target flush in launch_wgrad (the
    pose network's and the depth passes' second launch into a gradient must see the first) and the grads_ready bucket cuts."""
    from losses import Losses
    from mcav import nn as N
    from models.depth.resnet_dispnet import DispResNet
    from models.pose.pose_net import PoseNet
    from oracle.step import synthetic_batch
    from seeding import reinit_by_name
    s = synthetic_batch(2, 64, 128, seed=9)
    tgt, refs, K = s["tgt"].to(DEV), [r.to(DEV) for r in s["ref_imgs"]], s["intrinsics"].to(DEV)
    d = reinit_by_name(DispResNet(), 141).to(DEV).train()
    p = reinit_by_name(PoseNet(), 121).to(DEV).train()
    with torch.no_grad():
        p.pose_pred.weight.mul_(0.1)
        p.pose_pred.bias.mul_(0.1)
    state = [dict((k, v.clone()) for k, v in m.state_dict().items()) for m in (d, p)]
    params = list(d.named_parameters()) + list(p.named_parameters())
    saved = (N.WGRAD_BATCH.enabled, N.WGRAD_SIDE.enabled)
    out = {}
    try:
        for batch in (True, False):
            for side in (True, False):
                N.WGRAD_BATCH.enabled, N.WGRAD_SIDE.enabled = batch, side
                d.load_state_dict(state[0])               # (in place: every packed filter copy is stale again, as after an optimiser step)
                p.load_state_dict(state[1])
                for _, q in params:
                    q.grad = None
                disps = list(d.forward_pair(tgt, refs[0]))
                loss = Losses().forward(tgt, refs, disps, p(tgt, refs), K, None)
                sum(loss).backward()
                torch.cuda.synchronize()
                assert N.WGRAD_BATCH.items == [] and not N.WGRAD_SIDE.in_backward
                out[(batch, side)] = dict((n, q.grad.clone()) for n, q in params if q.grad is not None)
    finally:
        N.WGRAD_BATCH.enabled, N.WGRAD_SIDE.enabled = saved
    base = out[(False, False)]
    assert len(base) > 60 and any(float(g.abs().max()) > 0 for g in base.values())
    for key, grads in out.items():
        assert grads.keys() == base.keys()
        for n in base:
            assert torch.isfinite(grads[n]).all(), (key, n)
            assert torch.equal(grads[n], base[n]), "batch %s, side stream %s: the gradient of %s differs from the per-layer, in-line run" % (key + (n,))
