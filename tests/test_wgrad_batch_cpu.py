"""No GPU: the host side of the batched weight-gradient slab reduction (include/mcav_conv.h: mcav_wgrad_reduce_plan) and the case table the
GPU test runs (tests/wgrad_batch_cases.py).

  * mcav_wgrad_reduce_plan is host code on a host array and launches nothing: on hand-filled items its first-block columns must be the exclusive
    prefix sums of pre_bx * groups and red_gx * red_gy, its two grids the full sums and its LDS size the largest 4 * 32 * (ci_t * taps + 1).
  * The bucket of the GPU test must hold both reduction levels.  What each case states (kernel family, pixel splits) is asked of
    mcav_wgrad_route, which plans without dereferencing a pointer."""
import ctypes
import random

import wgrad_batch_cases as C

E_INVALID = -1


def lib():
    from mcav import lib as L
    from mcav import nn as N
    return L.lib(), N


def item(N, groups, pre_bx, red_gx, red_gy, ci_t, taps):
    it = N.WgradReduceItem()
    it.groups, it.pre_bx, it.red_gx, it.red_gy, it.ci_t, it.taps = groups, pre_bx, red_gx, red_gy, ci_t, taps
    it.pre_first = it.red_first = -7              # the plan must overwrite both
    return it


def plan(h, N, items):
    arr = (N.WgradReduceItem * len(items))(*items)
    pb, rb, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = h.mcav_wgrad_reduce_plan(arr, len(items), ctypes.byref(pb), ctypes.byref(rb), ctypes.byref(lds))
    return rc, arr, pb.value, rb.value, lds.value


# (groups, pre_bx, red_gx, red_gy, ci_t, taps): grouped items first, in the middle and last; 49 taps x ci_t 8 is the largest LDS tile
HAND = [(5, 37, 2, 32, 2, 9), (0, 0, 8, 128, 2, 9), (0, 0, 1, 256, 1, 1), (8, 13, 2, 1, 8, 49), (0, 0, 4, 64, 1, 1), (0, 0, 2, 16, 4, 9), (6, 3, 1, 16, 1, 9)]


def check_plan(h, N, rows):
    rc, arr, pb, rb, lds = plan(h, N, [item(N, *r) for r in rows])
    assert rc == 0
    pre = red = 0
    for it, (groups, pre_bx, gx, gy, ci_t, taps) in zip(arr, rows):
        assert (it.pre_first, it.red_first) == (pre, red), rows
        pre += pre_bx * groups
        red += gx * gy
    assert (pb, rb) == (pre, red)
    assert lds == max(4 * 32 * (r[4] * r[5] + 1) for r in rows)
    return arr


def test_reduce_plan_prefix_sums_totals_and_lds():
    h, N = lib()
    arr = check_plan(h, N, HAND)
    # an item without a presum contributes no presum blocks: it shares pre_first with its successor
    for i, r in enumerate(HAND[:-1]):
        if r[0] == 0:
            assert arr[i].pre_first == arr[i + 1].pre_first
    assert arr[0].pre_first == 0 and arr[1].pre_first == 5 * 37 and arr[3].pre_first == 5 * 37 and arr[4].pre_first == 5 * 37 + 8 * 13
    rng = random.Random(5)
    for _ in range(20):
        rows = HAND[:]
        rng.shuffle(rows)
        check_plan(h, N, rows[:rng.randint(1, len(rows))])
    rc, _, pb, rb, lds = plan(h, N, [item(N, 0, 0, 3, 5, 32, 9)])                  # a bucket without any two-level item: no presum launch at all
    assert (rc, pb, rb, lds) == (0, 0, 15, 4 * 32 * (32 * 9 + 1))


def test_reduce_plan_leaves_the_other_fields_alone():
    h, N = lib()
    its = [item(N, *r) for r in HAND]
    for k, it in enumerate(its):
        it.slab, it.pre, it.dw, it.dbias, it.elems = 0x1000 + k, 0x2000 + k, 0x3000 + k, 0x4000 + k, 1 << 33
        it.splits, it.per_group, it.Ktot, it.slabN, it.Kp, it.Cout, it.Cin = 9, 2, 576, 64, 64, 64, 64
        it.accumulate, it.upm, it.cin_total, it.ci_off, it.reserved = 1, 1, 128, 64, 11
    before = [bytes(it) for it in its]
    rc, arr, _, _, _ = plan(h, N, its)
    assert rc == 0
    for b, it in zip(before, arr):
        c = N.WgradReduceItem.from_buffer_copy(b)
        c.pre_first, c.red_first = it.pre_first, it.red_first
        assert bytes(c) == bytes(it)


def test_reduce_plan_refuses_an_empty_bucket_and_null_pointers():
    h, N = lib()
    arr = (N.WgradReduceItem * 2)(item(N, *HAND[0]), item(N, *HAND[1]))
    pb, rb, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    ok = (arr, 2, ctypes.byref(pb), ctypes.byref(rb), ctypes.byref(lds))
    assert h.mcav_wgrad_reduce_plan(*ok) == 0
    for n in (0, -1):
        assert h.mcav_wgrad_reduce_plan(arr, n, ok[2], ok[3], ok[4]) == E_INVALID
    for k in (0, 2, 3, 4):
        args = list(ok)
        args[k] = None
        assert h.mcav_wgrad_reduce_plan(*args) == E_INVALID, k
    assert h.mcav_wgrad_reduce_multi(None, 2, 0, 1, 1024, None) == E_INVALID        # refused before anything is launched
    for n, pbk, rbk in ((0, 0, 1), (2, -1, 1), (2, 0, 0)):
        assert h.mcav_wgrad_reduce_multi(0x1000, n, pbk, rbk, 1024, None) == E_INVALID


def test_bucket_holds_both_reduction_levels():
    """The case table against the planner: family and splits as stated, at least two two-level items and three single-level ones, the decoder
    level's two launches, both forms of the patch kernel, 49-tap stems; and in every order tested a grouped item first, in the middle or last."""
    h, N = lib()
    for c in C.BUCKET:
        d = C.plan_desc(N, c)
        r = N.ConvRoute()
        assert h.mcav_wgrad_route(ctypes.byref(d), ctypes.byref(r)) == 0, c.name
        print("%-36s family %d variant %#6x splits %2d groups %s workspace %d" % (c.name, r.family, r.variant, r.splits, c.groups, r.workspace_bytes))
        assert (r.family, r.splits) == (c.family, c.splits), (c.name, r.family, r.splits)
        assert bool(r.variant & N.RV_UPM) == bool(c.upm) and bool(r.variant & N.RV_SPLIT) == (c.mma == 2), (c.name, hex(r.variant))
        assert h.mcav_wgrad_workspace_bytes(ctypes.byref(d)) == r.workspace_bytes
        # the slab and, on the two-level path, the group sums: each rounded up to 256 bytes (what the GPU test poisons beyond)
        elems = (c.slab_taps * c.kp + 1) * C.up16(c.conv[4])
        a256 = lambda v: (v + 255) // 256 * 256
        assert r.workspace_bytes == a256(4 * c.splits * elems) + a256(4 * c.groups[0] * elems), c.name
    grouped = [c.grouped for c in C.BUCKET]
    assert sum(grouped) >= 2 and len(grouped) - sum(grouped) >= 3
    assert C.BUCKET[0].groups == (5, 2), "9 splits: five groups of two, the last one holding a single split"
    assert {c.family for c in C.BUCKET} == {C.FP32, C.HALO, C.STEM, C.BF16_PATCH}
    assert sorted(c.mma for c in C.BUCKET if c.family == C.BF16_PATCH) == [1, 2]
    assert [c.upm for c in C.BUCKET if c.share == "dec"] == [0, 1]
    where = set()
    for name, order in C.orders().items():
        g = [grouped[i] for i in order]
        assert sorted(order) == list(range(len(C.BUCKET)))
        where |= {"first"} if g[0] else set()
        where |= {"last"} if g[-1] else set()
        where |= {"middle"} if any(g[1:-1]) else set()
        # a single-level item directly in front of a two-level one: the two share pre_first
        assert any(not a and b for a, b in zip(g, g[1:])), name
    assert where == {"first", "middle", "last"}
