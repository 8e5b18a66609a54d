"""No GPU: what tests/test_head_gpu.py rests on.

  * every row and column alignment class of tests/head_cases.py is hit by a base case for each of the four channel counts, and the walk cases
    make a workgroup take a second tile of another row count than its first, under the kernels' own tile decoding;
  * mcav.nn.narrow_ok sends exactly the head's shapes to the stencil kernels;
  * tests/head_ref.py against itself: the float32 evaluation lies inside the envelope of the float64 one, the kernel's formulation (the gather
    G with its border terms) equals the autograd definition in float64, and the adjoint identity holds;
  * the judge has teeth: the kernel's formulation with one border term dropped, with a walked tile skipped or with ky not mirrored, evaluated
    in float32, falls outside the envelope on the pixels (filter taps) that term feeds and nowhere else;
  * mcav_conv3x3r_c1_fwd / _bwd refuse what they must before any launch (csrc/narrow_conv.hip: every check precedes the first HIP call, so
    no device is needed and the stand-in addresses are never read)."""
import ctypes

import pytest
import torch

import head_cases as K
import head_ref as R


@pytest.fixture(scope="module")
def N():
    from mcav import nn
    return nn


# ------------------------------------------------------------------------------------------------ the cases
def test_every_alignment_class_is_hit_for_every_channel_count():
    missing, lines = [], []
    for cl in K.ROW_CLASSES + K.COL_CLASSES:
        row = []
        for C in K.CHANNELS:
            hit = [c for c in K.CASES if c.C == C and cl.pred(c)]
            if not hit:
                missing.append("%s at C = %d" % (cl.name, C))
            row.append(", ".join("%dx%dx%d" % c[:3] for c in hit))
        lines.append("%-40s | %s" % (cl.name, " | ".join(row)))
    print("\nclass | cases (B x H x W) at C = 16 | 32 | 64 | 128")
    print("\n".join(lines))
    assert not missing, missing
    assert len(K.CASES) == 48 and all(c.H <= 35 and c.W <= 2 * K.pxb(c.C) + 1 and 1 <= c.B <= 3 for c in K.CASES)
    for C in K.CHANNELS:        # several residues of the tile count, tiles with one row and with one column
        own = [c for c in K.CASES if c.C == C]
        assert len({K.tiles(c) % 4 for c in own}) >= 3, C
        assert any(K.tile_rows(c, K.tiles(c) - 1) == 1 for c in own) and any(c.W % K.pxb(C) == 1 and c.W > K.pxb(C) for c in own)


def test_tile_decoding_covers_every_pixel_once():
    for c in K.CASES:
        seen = torch.zeros(c.B, c.H, c.W, dtype=torch.int32)
        for k in range(K.tiles(c)):
            n, y0, x0 = K.tile_origin(c, k)
            seen[n, y0:y0 + K.TH, x0:x0 + K.pxb(c.C)] += 1
            assert int(K.support_mask(c, ("tile", k)).sum()) == K.tile_rows(c, k) * min(K.pxb(c.C), c.W - x0) > 0
        assert bool((seen == 1).all()), c
        assert K.supports(c)[-1] == "dense" and all(0 < int(K.support_mask(c, s).sum()) <= 16 * 64 for s in K.supports(c)[:-1])
        classes = {K.pixel_class(c, y, x) for y in range(c.H) for x in range(c.W)}
        assert "corner" in classes and classes <= {"corner", "second line", "border line", "tile seam", "interior"}


def test_walk_cases_make_a_workgroup_take_a_second_tile_of_another_row_count():
    for c in K.WALK_CASES:
        assert (K.tiles_x(c), K.tiles_y(c)) == (1, 3) and [K.tile_rows(c, k) for k in range(3)] == [16, 16, 1]
        for cap in (K.BWD_BLOCKS,) + ((K.FWD_BLOCKS,) if c == K.FWD_WALK_CASE else ()):
            per = K.tiles_per_workgroup(c, cap)
            assert len(per) == cap and sum(per) == K.tiles(c) > cap and min(per) >= 1 and max(per) >= 2
            walkers = [g for g in range(cap) if per[g] >= 2]
            assert any(K.tile_rows(c, g) != K.tile_rows(c, g + cap) for g in walkers), (c, cap)
            if cap == K.FWD_BLOCKS:                      # the forward runs dense: no tile supports
                continue
            first, second, last = K.walk_tiles(c, cap)
            assert first < cap and per[first] >= 2 and second == first + cap and second != last == K.tiles(c) - 1
            assert K.tile_rows(c, first) != K.tile_rows(c, second)
            for k in (first, second, last):             # the supports lie where claimed: the rows of that tile in that image, nothing else
                n, y0, x0 = K.tile_origin(c, k)
                m = K.support_mask(c, ("tile", k))
                assert int(m.sum()) == int(m[n, 0, y0:y0 + K.tile_rows(c, k)].sum()) == 3 * K.tile_rows(c, k)
            print("%s: %d tiles on %d workgroups, %d..%d tiles each; supports on tiles %s" % (K.case_id(c), K.tiles(c), cap, min(per), max(per), (first, second, last)))
    assert K.tiles(K.WALK_CASES[0]) == K.tiles(K.WALK_CASES[1]) == 2052 and K.tiles(K.FWD_WALK_CASE) == 16386
    assert K.tiles_per_workgroup(K.WALK_CASES[0], K.BWD_BLOCKS).count(2) == 4 and K.tiles_per_workgroup(K.FWD_WALK_CASE, K.FWD_BLOCKS).count(2) == 2
    assert set(K.tiles_per_workgroup(K.FWD_WALK_CASE, K.BWD_BLOCKS)) == {8, 9}
    assert max(c.B * c.H * c.W * c.C for c in K.WALK_CASES) * 4 < 36e6


# ------------------------------------------------------------------------------------------------ mcav.nn.narrow_ok
def test_narrow_ok_truth_table(N):
    def ok(cin=16, cout=1, k=3, stride=1, pad=1, mode=None, H=8, W=8, cx=None):
        spec = N.ConvSpec(torch.nn.Parameter(torch.zeros(cout, cin, k, k)), None, stride, pad, N.PAD_REFLECT if mode is None else mode)
        return bool(N.narrow_ok(spec, torch.empty(1, H, W, cin if cx is None else cx, device="meta")))

    for cin in range(1, 260):
        assert ok(cin=cin) == (cin in (16, 32, 64, 128)), cin
    assert ok(H=2, W=2) and ok(H=2) and ok(W=2)
    assert not ok(H=1) and not ok(W=1)
    assert not ok(cout=2) and not ok(cout=16)
    assert not ok(k=1, pad=0) and not ok(k=5, pad=2) and not ok(k=1)
    assert not ok(stride=2) and not ok(pad=0) and not ok(pad=2) and not ok(mode=N.PAD_ZERO)
    assert not ok(cx=32)


# ------------------------------------------------------------------------------------------------ the reference against itself
FORMS = (("fused", True), ("pre-multiplied", False))


def _backward(c, support, fused, dtype, **kw):
    i = K.inputs(c)
    dy = i["dy"] * K.support_mask(c, support)
    return R.backward(i["x"], i["w"], dy, i["y"] if fused else None, R.ACT_SIGMOID if fused else R.ACT_NONE, addend=i["addend"], dtype=dtype, **kw)


def test_float32_evaluation_lies_inside_the_envelope_of_float64():
    worst = {}

    def note(name, got, want, env):
        r = float(R.ratio(got, want, env).max())
        worst[name] = max(worst.get(name, 0.0), r)
        assert not bool(R.outside(got, want, env).any()), (name, r)

    for c in K.CASES:
        i = K.inputs(c)
        for b in (i["b"], None):
            (w64, env), (w32, _) = R.forward(i["x"], i["w"], b), R.forward(i["x"], i["w"], b, dtype=R.F32)
            note("forward", w32, w64, env)
        for support in K.supports(c):
            for name, fused in FORMS:
                r64, r32 = _backward(c, support, fused, R.F64), _backward(c, support, fused, R.F32)
                note("dx " + name, r32["dx"], r64["dx"], r64["edx"])
                note("dw " + name, r32["dw"], r64["dw"], r64["edw"])
                note("db " + name, r32["db"], r64["db"], r64["edb"])
                assert bool((r64["dx"].float() == i["addend"])[(r64["S"] == 0).expand_as(r64["dx"])].all())      # no output reaches the pixel: the addend
    print("\nfloat32 torch against float64, worst |difference| / envelope:")
    for name in sorted(worst):
        print("  %-22s %.3f" % (name, worst[name]))
    assert worst and max(worst.values()) <= 1.0


def test_kernel_formulation_equals_the_definition_in_float64():
    for c in K.CASES:
        i = K.inputs(c)
        for support in K.supports(c):
            for name, fused in FORMS:
                for x_act in (R.ACT_ELU, R.ACT_RELU, R.ACT_NONE):
                    r = _backward(c, support, fused, R.F64, x_act=x_act)
                    dy = i["dy"] * K.support_mask(c, support)
                    dpre = R.pre_gradient(dy, i["y"] if fused else None, R.ACT_SIGMOID)
                    dx, dw, db = R.restate(i["x"], i["w"], dpre, x_act, i["addend"])
                    a = R.act_bwd(i["x"].double(), x_act).abs()
                    assert bool(((dx - r["dx"]).abs() <= 1e-12 * (a * r["S"] + i["addend"].double().abs())).all()), (c, support, name, "dx")
                    assert bool(((dw - r["dw"]).abs() <= 1e-12 * r["Sw"]).all()), (c, support, name, "dw")
                    assert bool(((db - r["db"]).abs() <= 1e-12 * r["Sb"]).all()), (c, support, name, "db")


def test_adjoint_identity_in_float64():
    """<conv(x), dy> = <x, adjoint(dy)>: the definition of dx is the transpose of the definition of the forward"""
    for c in K.CASES:
        i = K.inputs(c)
        pre, _ = R.forward(i["x"], i["w"], None)
        r = R.backward(i["x"], i["w"], i["dy"], x_act=R.ACT_NONE)
        lhs, rhs = float((pre * i["dy"].double()).sum()), float((i["x"].double() * r["dx"]).sum())
        scale = float((pre.abs() * i["dy"].double().abs()).sum())
        assert abs(lhs - rhs) <= 1e-12 * scale, (c, lhs, rhs)
        assert abs(float((r["dw"] * i["w"].double()).sum()) - lhs) <= 1e-12 * scale       # ... and dw is the transpose in the other operand


# ------------------------------------------------------------------------------------------------ the judge has teeth
def _region(c, drop):
    """[H, W] bool: the pixels of dx that the dropped term feeds"""
    m = torch.zeros(c.H, c.W, dtype=torch.bool)
    rows, cols = {"yt": 1, "yb": c.H - 2}, {"xl": 1, "xr": c.W - 2}
    if drop == "swap ky":
        m[:] = True
    elif drop in rows:
        m[rows[drop]] = True
    elif drop in cols:
        m[:, cols[drop]] = True
    else:
        a, b = drop.split("&")
        m[rows[a], cols[b]] = True
    return m


TAPS = {"yt": {0, 1, 2}, "yb": {6, 7, 8}, "xl": {0, 3, 6}, "xr": {2, 5, 8}, "yt&xl": {0}, "yt&xr": {2}, "yb&xl": {6}, "yb&xr": {8},
        "swap ky": {0, 1, 2, 6, 7, 8}}


def _classes(c, mask):
    return {K.pixel_class(c, int(y), int(x)) for y, x in mask.nonzero()}


def test_every_mutant_falls_outside_the_envelope_where_it_should():
    """dx with dense dy, dw with dy on the border band (the pre-multiplied form: dy is dpre)"""
    for c in K.CASES:
        i = K.inputs(c)
        dense, band = _backward(c, "dense", False, R.F64), _backward(c, "band", False, R.F64)
        dy_band = i["dy"] * K.support_mask(c, "band")
        # the unmutated formulation in float32 is inside: what falls outside below is the mutation's doing
        dx, _, _ = R.restate(i["x"], i["w"], i["dy"], R.ACT_ELU, i["addend"], R.F32)
        _, dw, db = R.restate(i["x"], i["w"], dy_band, R.ACT_ELU, i["addend"], R.F32)
        assert not bool(R.outside(dx, dense["dx"], dense["edx"]).any()) and not bool(R.outside(dw, band["dw"], band["edw"]).any())
        assert not bool(R.outside(db, band["db"], band["edb"]).any())
        for drop in R.MUTANTS:
            dx, _, _ = R.restate(i["x"], i["w"], i["dy"], R.ACT_ELU, i["addend"], R.F32, drop=drop)
            bad = R.outside(dx, dense["dx"], dense["edx"]).any(1)                       # [B, H, W]
            region = _region(c, drop)
            assert bool(bad.any()), "dx: mutant %r stays inside the envelope at %s" % (drop, K.case_id(c))
            assert not bool((bad & ~region).any()), "dx: mutant %r moves pixels it does not feed at %s" % (drop, K.case_id(c))
            assert _classes(c, bad.any(0)) == _classes(c, region), (drop, K.case_id(c), _classes(c, bad.any(0)), _classes(c, region))
            if drop != "swap ky":
                assert bool(bad.all(0)[region].all()), "dx: mutant %r is not seen on every pixel it feeds in every image at %s" % (drop, K.case_id(c))
            _, dw, _ = R.restate(i["x"], i["w"], dy_band, R.ACT_ELU, i["addend"], R.F32, drop=drop)
            taps = {int(t) for t in R.outside(dw, band["dw"], band["edw"]).reshape(c.C, 9).any(0).nonzero().flatten()}
            assert taps == TAPS[drop], "dw: mutant %r is seen on taps %s, it feeds %s, at %s" % (drop, sorted(taps), sorted(TAPS[drop]), K.case_id(c))


def test_a_skipped_second_tile_falls_outside_the_envelope():
    """the walk cases: the tile a workgroup should walk second is never visited -- its dx is never stored, its pixels are missing in dw / db"""
    for c in K.WALK_CASES[:2]:
        i = K.inputs(c)
        for k in K.walk_tiles(c)[1:]:
            n, y0, x0 = K.tile_origin(c, k)
            rows = K.tile_rows(c, k)
            one = K.Case(1, c.H, c.W, c.C)
            dy = (i["dy"] * K.support_mask(c, ("tile", k)))[n:n + 1]
            x, add = i["x"][n:n + 1], i["addend"][n:n + 1]
            want = R.backward(x, i["w"], dy, addend=add)
            good = R.restate(x, i["w"], dy, R.ACT_ELU, add, R.F32)
            got = R.restate(x, i["w"], dy, R.ACT_ELU, add, R.F32, skip=(0, y0, y0 + rows, x0, x0 + K.pxb(c.C)))
            for name, g, m in zip(("dx", "dw", "db"), good, got):
                assert not bool(R.outside(g, want[name], want["e" + name]).any()), (name, K.case_id(c), k)
                bad = R.outside(m, want[name], want["e" + name])
                assert bool(bad.any()), "%s: a skipped tile %d stays inside the envelope at %s" % (name, k, K.case_id(c))
                if name == "dx":
                    region = torch.zeros(c.H, c.W, dtype=torch.bool)
                    region[y0:y0 + rows] = True
                    assert torch.equal(bad[0].any(0), region) and _classes(one, bad[0].any(0)) == _classes(one, region)


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
E_INVALID, E_WORKSPACE = -1, -2
A = 0x10000       # a stand-in address: a refusing call returns before anything is read or launched


def _fwd(h, x=A, B=1, H=8, W=8, C=16, w=A + 0x1000, bias=A + 0x2000, act=0, y=A + 0x3000):
    return h.mcav_conv3x3r_c1_fwd(x, B, H, W, C, w, bias, act, y, None)


def _bwd(h, x=A, B=1, H=8, W=8, C=16, w=A + 0x1000, dy=A + 0x2000, y=A + 0x3000, act=3, x_act=2, addend=None, dx=A + 0x4000, dw=A + 0x5000,
         db=A + 0x6000, acc=1, ws=A + 0x7000, ws_bytes=None):
    need = h.mcav_conv3x3r_c1_bwd_workspace_bytes(C)
    return h.mcav_conv3x3r_c1_bwd(x, B, H, W, C, w, dy, y, act, x_act, addend, dx, dw, db, acc, ws, need if ws_bytes is None else ws_bytes, None)


def test_workspace_bytes(N):
    h = N.L.lib()
    for C in range(0, 300):
        want = (4 * K.BWD_BLOCKS * (9 * C + 1) + 255) // 256 * 256 if C in K.CHANNELS else 0
        assert h.mcav_conv3x3r_c1_bwd_workspace_bytes(C) == want, C
    assert h.mcav_conv3x3r_c1_bwd_workspace_bytes(-16) == 0


def test_forward_refusals(N):
    h = N.L.lib()
    for kw in ([dict(C=C) for C in (8, 48, 256, 0, -16, 17)] + [dict(H=1), dict(W=1), dict(H=0), dict(W=-3), dict(B=0), dict(B=-1), dict(x=None), dict(w=None),
               dict(y=None), dict(B=1 << 15, H=256, W=256)]):
        assert _fwd(h, **kw) == E_INVALID, kw


def test_backward_refusals(N):
    h = N.L.lib()
    for kw in ([dict(C=C) for C in (8, 48, 256, 0, -16, 17)] + [dict(H=1), dict(W=1), dict(H=0), dict(B=0), dict(B=-1)] +
               [{name: None} for name in ("x", "w", "dy", "dx", "dw", "ws")] +
               [dict(y=None, act=act) for act in (R.ACT_RELU, R.ACT_ELU, R.ACT_SIGMOID)] + [dict(B=1 << 15, H=256, W=256)]):
        assert _bwd(h, **kw) == E_INVALID, kw
    for C in K.CHANNELS:
        need = h.mcav_conv3x3r_c1_bwd_workspace_bytes(C)
        assert _bwd(h, C=C, ws_bytes=need - 1) == E_WORKSPACE and _bwd(h, C=C, ws_bytes=0) == E_WORKSPACE
        assert _bwd(h, C=C, ws_bytes=need - 1, y=None, act=R.ACT_SIGMOID) == E_INVALID       # the argument check comes first
