"""No GPU: what tests/test_halo_gpu.py rests on.

  * the planner (mcav_igemm_route / mcav_wgrad_route: they never dereference a pointer) takes every (case, form) of tests/halo_cases.py to the
    halo family, with the expected variant bits and with the workgroups / splits of that file's own tile arithmetic -- so the GPU test
    never silently tests another kernel, and the Python tile constants are the library's;
  * every alignment class, template instantiation and grid residue is hit by at least one case of every form it applies to;
  * the elementwise envelope is only used on dy supports of at most 512 pixels, and the walk cases have workgroups with two tiles and with one;
  * tests/halo_ref.py against itself: the float32 torch evaluation of every form lies inside the envelope of the float64 one."""
import ctypes

import pytest

import halo_cases as K
import halo_ref as R


@pytest.fixture(scope="module")
def N():
    from mcav import nn
    return nn


def _route(N, query, d):
    r = N.ConvRoute()
    rc = query(ctypes.byref(d), ctypes.byref(r))
    return rc, r


def pairs(kinds):
    return [(f, c) for f in K.FORMS if f.kind in kinds for c in K.CASES if K.applies(f, c)]


def test_planner_takes_every_forward_and_adjoint_case_to_the_halo_kernels(N):
    h = N.L.lib()
    checked = 0
    for form, c in pairs(("fwd", "adj")):
        for n_begin in ((0, 16) if form.name == "adj n_begin 0|16" else (0,)):
            rc, r = _route(N, h.mcav_igemm_route, K.igemm_desc(N, form, c, n_begin=n_begin))
            assert rc == 0, (form.name, c, "refused")
            family, variant, wgs = K.expected_igemm_route(N, form, c)
            assert (r.family, r.variant, r.workgroups, r.ntiles) == (family, variant, wgs, K.launches(form, c)), (form.name, c, r.family, r.variant, r.workgroups)
            # ... and bit 9 takes the same descriptor to the general fp32 kernels (the comparison runs)
            rc, r = _route(N, h.mcav_igemm_route, K.igemm_desc(N, form, c, tile=form.tile | K.T_GENERAL, n_begin=n_begin))
            assert rc == 0 and r.family == N.IGEMM_FP32, (form.name, c, rc, r.family)
            checked += 1
    assert checked >= 150


def test_planner_takes_every_weight_gradient_case_to_the_halo_kernels(N):
    h = N.L.lib()
    todo = pairs(("wgrad",)) + [(K.FORM[name], c) for c, names in K.WALK_CASES for name in names]
    for form, c in todo:
        assert K.applies(form, c), (form.name, c)
        rc, r = _route(N, h.mcav_wgrad_route, K.wgrad_desc(N, form, c))
        assert rc == 0, (form.name, c, "refused")
        assert (r.family, r.variant, r.workgroups, r.splits) == K.expected_wgrad_route(N, form, c), (form.name, c, r.family, r.variant, r.workgroups, r.splits)
    assert len(todo) >= 100


def _classes(form):
    out = [cl for cl in K.ROW_CLASSES + K.COL_CLASSES if cl.even_ok or not form.even]
    return out + (list(K.UP_CLASSES) if form.up else [])


def test_every_class_instantiation_and_residue_is_hit_by_every_form():
    lines, missing = [], []
    for form in K.FORMS:
        cases = [c for c in K.CASES if K.applies(form, c)]
        row = []
        for cl in _classes(form):
            n = sum(1 for c in cases if cl.pred(c))
            row.append(n)
            if not n:
                missing.append((form.name, cl.name))
        inst = {i: sum(1 for c in cases if K.instantiation(form, c) == i) for i in K.instantiations_of(form)}
        missing += [(form.name, i) for i, n in inst.items() if not n]
        res = ""
        if form.kind != "wgrad":                      # the forward / adjoint grid goes through xcd_remap: every residue of the grid modulo 8
            hit = sorted({K.tiles(c) % 8 for c in cases})
            missing += [(form.name, "grid %% 8 == %d" % r) for r in range(8) if r not in hit]
            res = "  grid residues %s" % hit
        lines.append("%-22s %3d cases  classes %s  %s%s" % (form.name, len(cases), row, inst, res))
    print("\nform, cases, cases per class (%s; merged-tap forms: + %s), cases per instantiation" % (
        ", ".join(cl.name for cl in K.ROW_CLASSES + K.COL_CLASSES), ", ".join(cl.name for cl in K.UP_CLASSES)))
    print("\n".join(lines))
    assert not missing, missing
    assert {c.C for c in K.CASES} == {16, 32} and {c.Cout for c in K.CASES} == {8, 16, 24, 32}
    assert all(c.H <= 17 and c.W <= 66 for c in K.CASES) and len(K.CASES) <= 36


def test_elementwise_supports_hold_at_most_512_pixels():
    for c in K.CASES:
        for s in K.supports(c)[:-1]:
            assert 0 < int(K.support_mask(c, s).sum()) <= 512, (c, s)
        assert K.supports(c)[-1] == "dense"
    for c, _ in K.WALK_CASES:
        for k in K.WALK_TILES:
            assert int(K.support_mask(c, ("tile", k)).sum()) == K.HT_H * K.HT_W


def test_walk_cases_have_workgroups_with_two_tiles_and_with_one():
    for c, names in K.WALK_CASES:
        per = K.tiles_per_workgroup(c)
        assert len(per) == K.MAX_SPLITS and set(per) == {1, 2} and sum(per) == K.tiles(c) > K.MAX_SPLITS
        first, second, last = K.WALK_TILES
        assert first < K.MAX_SPLITS and per[first] == 2                         # walked first by a workgroup that goes on
        assert second >= K.MAX_SPLITS and second != K.tiles(c) - 1               # walked second
        assert last == K.tiles(c) - 1
        assert K.tile_origin(c, K.MAX_SPLITS)[0] == c.B - 1                      # the second tiles lie in the last image
    assert any("wgrad up merged" in names and (c.C, c.Cout) == (16, 16) for c, names in K.WALK_CASES)


def _self_check(name, want32, want64, env, worst):
    r = float(R.ratio(want32, want64, env).max())
    worst[name] = max(worst.get(name, 0.0), r)
    assert not bool(R.outside(want32, want64, env).any()), (name, r)


def test_float32_evaluation_lies_inside_the_envelope_of_float64():
    """the reference alone satisfies the bound, before any kernel is judged"""
    worst = {}
    for c in K.CASES:
        i = K.inputs(c)
        for form in K.FORMS:
            if not K.applies(form, c):
                continue
            if form.kind == "fwd":
                x = i["xl"] if form.up else i["x"]
                (w64, env), (w32, _) = R.forward(x, i["w"], i["b"], form.reflect, form.up), R.forward(x, i["w"], i["b"], form.reflect, form.up, R.F32)
                _self_check(form.name, w32, w64, env, worst)
            elif form.kind == "adj":
                kw = dict(pool=True, aux=i["aux"], addend=i["add"]) if form.name.startswith("adj pool") else {}
                (w64, env), (w32, _) = R.adjoint(i["dy"], i["w"], **kw), R.adjoint(i["dy"], i["w"], dtype=R.F32, **kw)
                _self_check(form.name, w32, w64, env, worst)
            else:
                x = i["xl"] if form.up else i["x"]
                for s in K.supports(c)[:-1]:
                    dy = i["dy"] * K.support_mask(c, s)
                    dw64, ew, db64, eb = R.wgrad(x, dy, form.reflect, form.up)
                    dw32, _, db32, _ = R.wgrad(x, dy, form.reflect, form.up, R.F32)
                    _self_check(form.name, dw32, dw64, ew, worst)
                    _self_check(form.name + " (bias)", db32, db64, eb, worst)
    print("\nfloat32 torch against float64, worst |difference| / envelope per form:")
    for name in sorted(worst):
        print("  %-32s %.3f" % (name, worst[name]))
    assert worst and max(worst.values()) <= 1.0
