"""CPU: oriented-box overlap and greedy suppression (include/mcav_depth.h: mcav_box_iou, mcav_box_nms; pseudo_lidar.boxes_iou_bev,
boxes_iou3d, nms).  The restatement (tests/box_ref.py) against its float64 formulation within the bound its docstring gives, and against
nine wrong definitions that must each exceed it or change a kept set; the header csrc/box_math.h compiled for the host against the
restatement, bit for bit, on the pairs and the cases the GPU tests run (tests/box_cases.py), once more as a stand-alone program under the
address and undefined-behaviour sanitizers; box_sincos against the float64 functions and against C's fmaf; the select order against
numpy.lexsort; the refusals; the workspace formula; what is exported, declared and bound; what the Python side refuses without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import box_cases as C
import box_ref as R
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "box_hostcheck", "box_hostcheck.cpp")
F = np.float32
ENTRIES = ("mcav_box_iou", "mcav_box_nms_workspace_bytes", "mcav_box_nms")
MODES = ("bev", "3d")


# ---------------------------------------------------------------------------------------------- restatement vs the float64 formulation
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", C.PAIR_FAMILIES)
def test_restatement_within_the_bound_of_float64(family, mode):
    (inter, iou), ref = C.pair_reference(family, mode)
    a, b = C.pair_family(family)
    ok = R.valid(a) & R.valid(b)
    err = np.abs(inter.astype(np.float64) - ref["inter"])
    assert (err <= ref["bound_inter"]).all(), float((err / np.maximum(ref["bound_inter"], 1e-300)).max())
    err = np.abs(iou.astype(np.float64) - ref["iou"])
    assert (err <= ref["bound_iou"]).all(), float((err / np.maximum(ref["bound_iou"], 1e-300)).max())
    assert not inter[~ok].view(np.uint32).any() and not iou[~ok].view(np.uint32).any()         # +0.0 with everything, itself included
    assert (iou >= 0).all() and (iou <= 1).all() and (inter <= np.minimum(a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]))[ok].all()
    if family == "invalid":
        assert not ok.any() and len(ok) == 2 * len(C.INVALID)
    elif family not in ("touching-corner", "shared-edge", "cm-against-50m"):
        assert (ref["inter"] > 1e-3).sum() >= len(a) // 3                                       # the family overlaps
    if family == "identical":                                 # iou(A, A) within the bound of 1
        assert (np.abs(iou.astype(np.float64) - 1.0) <= ref["bound_iou"]).all() and (ref["bound_iou"] < 1e-4).all()
    if family == "axis-aligned":                              # the float64 formulation itself against the exact closed form
        exact = R.inter_axis_aligned(a, b)
        assert np.abs(ref["inter"] - exact).max() <= 1e-12 * 40 and (exact > 0).sum() > 100


@pytest.mark.parametrize("mode", MODES)
def test_overlap_is_symmetric_within_twice_the_bound(mode):
    for family in ("random", "wide-heading", "inside", "cm-against-50m", "far-small"):
        a, b = C.pair_family(family)
        (_, ab), ref = C.pair_reference(family, mode)
        _, ba = R.pairs_iou(b, a, mode)
        assert (np.abs(ab.astype(np.float64) - ba) <= 2 * ref["bound_iou"]).all(), family
        assert (ab != ba).any() or family != "random"                                           # not symmetric bit for bit: the order is part of the rule


@pytest.mark.parametrize("mutant", R.PAIR_MUTANTS)
def test_wrong_pair_definitions_exceed_the_bound(mutant):
    """each mutant of the restatement lies further than 100 x the bound from the float64 formulation, somewhere.  `no-translation` does so
    on the small far boxes only (and stays within the bound near the origin); `no-clamp` cannot -- the clamp corrects last-place errors --
    so it is told by what the clamp guarantees: without it some intersection exceeds the smaller area and some overlap exceeds 1."""
    if mutant == "no-clamp":
        a, b = C.pair_family("identical")
        inter, iou = R.pairs_iou(a, b, "3d", mutant=mutant)
        assert (inter > a[:, 3] * a[:, 4]).any() and (iou > 1).any()
        inter, iou = R.pairs_iou(a, b, "3d")
        assert (inter <= a[:, 3] * a[:, 4]).all() and (iou <= 1).all()
        return
    family = "far-small" if mutant == "no-translation" else "random"
    a, b = C.pair_family(family)
    _, ref = C.pair_reference(family, "bev")
    inter, iou = R.pairs_iou(a, b, "bev", mutant=mutant)
    if mutant == "union-without-inter":
        assert (np.abs(iou.astype(np.float64) - ref["iou"]) > 100 * ref["bound_iou"]).sum() > 10
    else:
        assert (np.abs(inter.astype(np.float64) - ref["inter"]) > 100 * ref["bound_inter"]).sum() > 10
    if mutant == "no-translation":                            # the same boxes moved to the origin: nothing to lose
        shift = a[:, :2].copy()
        a0, b0 = a.copy(), b.copy()
        a0[:, :2] -= shift
        b0[:, :2] -= shift
        ref0 = R.iou_f64(a0, b0, "bev")
        inter0, _ = R.pairs_iou(a0, b0, "bev", mutant=mutant)
        assert (np.abs(inter0.astype(np.float64) - ref0["inter"]) <= ref0["bound_inter"]).all()


def ge_case():
    """two overlapping boxes and the overlap of the pair as the threshold: `>` keeps both, `>=` only the first"""
    boxes = np.array([[[10, 0, -1, 4, 1.8, 1.5, 0.3], [11, 0.2, -1, 4, 1.8, 1.5, 0.4], [30, 5, -1, 4, 1.8, 1.5, 0.0]]], F)
    scores = np.array([[0.9, 0.8, 0.7]], F)
    p = R.prepare(boxes[0])
    thresh = float(R.iou(R.take(p, [0]), R.take(p, [1]), "bev")[0])
    return dict(boxes=boxes, scores=scores, score_thresh=0.1, iou_thresh=thresh, pre_max=16, post_max=16, mode="bev")


@pytest.mark.parametrize("mutant", R.RULE_MUTANTS)
def test_wrong_rules_change_a_kept_set(mutant):
    case = {">=": None, "all-earlier": "chain-over-chunk", "index-descending": "cut-4096-ties", "classes-ignored": "classes"}[mutant]
    if case is None:
        a = ge_case()
        assert 0.2 < a["iou_thresh"] < 0.8
        right = R.nms(**a)
    else:
        C.check_non_trivial(case)
        a, right = C.call_args(case), C.reference(case)
    wrong = R.nms(mutant=mutant, **a)
    assert not np.array_equal(wrong["keep"], right["keep"])
    if mutant == ">=":
        assert right["num"].tolist() == [3] and wrong["num"].tolist() == [2]
    if mutant == "all-earlier":
        assert C.build(case)["chain"]["k"] not in wrong["keep"][0].tolist()


@pytest.mark.parametrize("case", C.CASES)
def test_float64_rule_keeps_the_same_rows(case):
    C.check_non_trivial(case)
    assert np.array_equal(C.reference_f64(case)["keep"], C.reference(case)["keep"])
    assert np.array_equal(C.reference_f64(case)["num"], C.reference(case)["num"])


# ---------------------------------------------------------------------------------------------- csrc/box_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("box_hostcheck") / "libbox_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, f, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_size_t
    lib.box_host_constants.argtypes = [p, p]
    lib.box_host_sincos.argtypes = [p, p, p, ll]
    lib.box_host_prepare.argtypes = [p, ll, p]
    lib.box_host_pairs.argtypes = [p, p, ll, i, p, p]
    lib.box_host_iou.argtypes = [p, ll, p, ll, i, p]
    lib.box_host_workspace_bytes.restype = sz
    lib.box_host_workspace_bytes.argtypes = [i, ll, i]
    lib.box_host_select.argtypes = [p, p, i, ll, f, i, p, p]
    lib.box_host_nms.argtypes = [p, p, p, i, ll, f, f, i, i, i, p, p, p, p, p, sz]
    lib.box_host_sincos_scan.restype = ctypes.c_double
    lib.box_host_sincos_scan.argtypes = [ctypes.c_uint32] * 3 + [p]
    return lib


def workspace_bytes(B, A, pre_max):
    up = lambda v: (v + 255) // 256 * 256
    rows = B * pre_max
    return up(4 * B) + 2 * up(4 * rows) + up(80 * rows) + up(8 * rows * ((pre_max + 63) // 64))


def host_nms(host, a, **change):
    boxes, scores = np.ascontiguousarray(a["boxes"]), np.ascontiguousarray(a["scores"])
    B, A = scores.shape
    arg = dict(boxes=boxes, scores=scores, classes=None if a.get("classes") is None else np.ascontiguousarray(a["classes"]), B=B, A=A,
               score_thresh=a["score_thresh"], iou_thresh=a["iou_thresh"], mode=R.MODES[a["mode"]], pre_max=a["pre_max"], post_max=a["post_max"])
    arg.update({k: v for k, v in change.items() if k in ("pre_max", "post_max", "B", "A")})
    post = max(int(arg["post_max"]), 1) if arg["post_max"] < 1 << 20 else 1
    arg.update(keep=np.full((B, post), -7, np.int32), num=np.full(B, -7, np.int32), out_boxes=np.full((B, post, 7), -7, F),
               out_scores=np.full((B, post), -7, F))
    nbytes = workspace_bytes(B, A, a["pre_max"])
    raw = np.zeros(nbytes + 256, np.uint8)
    arg.update(ws=raw[(-raw.ctypes.data) % 256:][:nbytes], nbytes=nbytes)
    arg.update(change)
    ptr = lambda v: v if v is None or isinstance(v, int) else v.ctypes.data
    rc = host.box_host_nms(ptr(arg["boxes"]), ptr(arg["scores"]), ptr(arg["classes"]), arg["B"], arg["A"], arg["score_thresh"], arg["iou_thresh"],
                           arg["mode"], arg["pre_max"], arg["post_max"], ptr(arg["keep"]), ptr(arg["num"]), ptr(arg["out_boxes"]),
                           ptr(arg["out_scores"]), ptr(arg["ws"]), arg["nbytes"])
    return rc, arg


def test_constants_are_the_headers(host):
    ints, floats = np.zeros(4, np.int32), np.zeros(5, F)
    host.box_host_constants(ints.ctypes.data, floats.ctypes.data)
    assert ints.tolist() == [8, R.NMS_MAX_CANDIDATES, 80, 7]
    assert floats.tolist() == [R.MIN_EXTENT, R.MAX_EXTENT, R.MAX_HEADING, R.CIRCLE_SLACK, R.BOX_SINCOS_MAX_ULP] and floats[4] <= 2.0 and floats[2] >= 8 * np.pi


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", C.PAIR_FAMILIES)
def test_header_matches_restatement_on_pairs(host, family, mode):
    a, b = C.pair_family(family)
    (inter, iou), _ = C.pair_reference(family, mode)
    got_inter, got_iou = np.empty(len(a), F), np.empty(len(a), F)
    host.box_host_pairs(a.ctypes.data, b.ctypes.data, len(a), R.MODES[mode], got_inter.ctypes.data, got_iou.ctypes.data)
    C.same_bits(got_inter, inter)
    C.same_bits(got_iou, iou)
    prep = np.empty((len(a), 20), F)
    host.box_host_prepare(a.ctypes.data, len(a), prep.ctypes.data)
    p = R.prepare(a)
    want = np.concatenate([np.stack([p["cx"], p["cy"], p["zlo"], p["zhi"]], 1), p["px"], p["py"],
                           np.stack([p["area"], p["vol"], p["r"], p["ok"], p["c"], p["s"], p["hx"], p["hy"]], 1)], 1)
    C.same_bits(prep, want)


@pytest.mark.parametrize("mode", MODES)
def test_header_iou_matrix(host, mode):
    a, b = C.iou_matrix_operands()
    out = np.full((len(a), len(b)), -7, F)
    assert host.box_host_iou(a.ctypes.data, len(a), b.ctypes.data, len(b), R.MODES[mode], out.ctypes.data) == 0
    C.same_bits(out, C.iou_matrix_reference(mode))
    assert (out > 0).sum() > 100 and (out > 0.3).sum() >= 10 and (out == 0).sum() > out.size // 2
    for bad in (dict(a=None), dict(b=None), dict(out=None), dict(na=-1), dict(nb=65535 * 64 + 1), dict(mode=2), dict(mode=-1),
                dict(a=a.ctypes.data + 2), dict(out=out.ctypes.data + 1)):
        arg = dict(a=a.ctypes.data, na=len(a), b=b.ctypes.data, nb=len(b), mode=0, out=out.ctypes.data)
        arg.update(bad)
        before = out.copy()
        assert host.box_host_iou(arg["a"], arg["na"], arg["b"], arg["nb"], arg["mode"], arg["out"]) == -1, bad
        C.same_bits(out, before)


@pytest.mark.parametrize("case", C.CASES)
def test_header_matches_restatement_on_cases(host, case):
    a, want = C.call_args(case), C.reference(case)
    rc, arg = host_nms(host, a)
    assert rc == 0
    assert np.array_equal(arg["keep"], want["keep"]) and np.array_equal(arg["num"], want["num"])
    C.same_bits(arg["out_boxes"], want["boxes"])
    C.same_bits(arg["out_scores"], want["scores"])
    rc, plain = host_nms(host, a, out_boxes=None, out_scores=None)
    assert rc == 0 and np.array_equal(plain["keep"], want["keep"]) and np.array_equal(plain["num"], want["num"])


@pytest.mark.parametrize("case", ["cut-4096-ties", "radix-20000", "zeros-and-nans", "invalid-on-top", "batch-3-empty-middle"])
def test_select_order_is_numpy_lexsort(host, case):
    a = C.call_args(case)
    B, A = a["scores"].shape
    order, count = np.full((B, a["pre_max"]), -7, np.int32), np.full(B, -7, np.int32)
    host.box_host_select(a["boxes"].ctypes.data, a["scores"].ctypes.data, B, A, a["score_thresh"], a["pre_max"], order.ctypes.data, count.ctypes.data)
    for b in range(B):
        s = a["scores"][b]
        with np.errstate(invalid="ignore"):
            cand = np.nonzero(R.valid(a["boxes"][b]) & (s >= F(a["score_thresh"])))[0]
        want = cand[np.lexsort((cand, -(s[cand].astype(np.float64) + 0.0)))][:a["pre_max"]]
        assert count[b] == len(want) and np.array_equal(order[b, :len(want)], want) and (order[b, len(want):] == -1).all()
        assert np.array_equal(want, R.order_of(a["boxes"][b], s, a["score_thresh"], a["pre_max"]))


# ---------------------------------------------------------------------------------------------- box_sincos
def test_box_sincos_bits_and_ulp_bound(host):
    """The header's box_sincos is the restatement's (numpy with an emulated fmaf: so it is held to C's fmaf) bit for bit on 300 000
    headings: random ones over [-32, 32], the first 2000 floats from zero, the last 2000 below the limit, 2000 on either side of every
    multiple of pi / 4 up to the limit and of the exhaustive scan's worst argument.  Its error against the float64 sine and cosine stays
    within the header's BOX_SINCOS_MAX_ULP on a stated subset -- every 1021st float32 of [0, 32] with both signs (2.2 million headings)
    and the 2^17 floats on either side of the worst argument -- which the exhaustive scan (`box_hostcheck --sincos-ulp`, the stand-alone
    build) covers in full."""
    rng = np.random.RandomState(11)
    bits_of = lambda v: int(np.array([v], F).view(np.uint32)[0])
    worst, top = bits_of(float.fromhex("0x1.9f8aaep+4")), bits_of(32.0)
    marks = [worst] + [bits_of(k * np.pi / 4) for k in range(1, 41)]
    bits = np.concatenate([np.arange(0, 2000), np.arange(top - 2000, top + 1)] + [np.arange(m - 2000, min(m + 2000, top + 1)) for m in marks])
    h = np.concatenate([bits.astype(np.uint32).view(F), -bits.astype(np.uint32).view(F), rng.uniform(-32, 32, 130000).astype(F),
                        (10.0 ** rng.uniform(-30, 0, 3000)).astype(F)])
    s, c = np.empty_like(h), np.empty_like(h)
    host.box_host_sincos(h.ctypes.data, s.ctypes.data, c.ctypes.data, len(h))
    ws, wc = R.box_sincos(h)
    C.same_bits(s, ws)
    C.same_bits(c, wc)
    for got, want in ((s, np.sin(h.astype(np.float64))), (c, np.cos(h.astype(np.float64)))):
        live = want != 0
        ulp = 2.0 ** (np.floor(np.log2(np.abs(want[live]))) - 23)
        assert (np.abs(got[live].astype(np.float64) - want[live]) / ulp).max() <= R.BOX_SINCOS_MAX_ULP
        assert not got[~live].any()
    at = ctypes.c_float(0)
    assert 1.0 < host.box_host_sincos_scan(0, top, 1021, ctypes.addressof(at)) <= R.BOX_SINCOS_MAX_ULP
    near = host.box_host_sincos_scan(worst - (1 << 17), worst + (1 << 17), 1, ctypes.addressof(at))
    assert abs(near - 1.552836) < 1e-6 and near <= R.BOX_SINCOS_MAX_ULP and abs(at.value) == float.fromhex("0x1.9f8aaep+4")


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(host):
    a = C.call_args("classes")
    nan = float("nan")
    rc, ok = host_nms(host, a)
    assert rc == 0
    off = lambda v, n: v.ctypes.data + n
    bad = [dict(boxes=None), dict(scores=None), dict(keep=None), dict(num=None), dict(ws=None), dict(B=0), dict(B=-1), dict(B=65536), dict(A=0),
           dict(A=-5), dict(B=4, A=1 << 29), dict(pre_max=0), dict(pre_max=4097), dict(post_max=0), dict(post_max=a["pre_max"] + 1),
           dict(score_thresh=nan), dict(iou_thresh=nan), dict(mode=2), dict(mode=-1), dict(boxes=off(ok["boxes"], 2)),
           dict(scores=off(ok["scores"], 1)), dict(classes=off(ok["classes"], 2)), dict(keep=off(ok["keep"], 2)), dict(num=off(ok["num"], 1)),
           dict(out_boxes=off(ok["out_boxes"], 2)), dict(out_scores=off(ok["out_scores"], 3)), dict(ws=off(ok["ws"], 8))]
    for change in bad:
        rc, arg = host_nms(host, a, **change)
        assert rc == -1, change
        for name in ("keep", "num", "out_boxes", "out_scores"):
            if not isinstance(arg[name], (int, type(None))):
                assert (arg[name] == -7).all(), change
    rc, arg = host_nms(host, a, nbytes=ok["nbytes"] - 1)
    assert rc == -2 and all((arg[name] == -7).all() for name in ("keep", "num", "out_boxes", "out_scores"))


def test_workspace_formula(host):
    import mcav.lib as L
    import pseudo_lidar  # noqa: F401
    for B, A, pre_max in ((12, 321408, 4096), (1, 1, 1), (3, 20000, 3000), (2, 77, 65)):
        assert host.box_host_workspace_bytes(B, A, pre_max) == workspace_bytes(B, A, pre_max) == L.lib().mcav_box_nms_workspace_bytes(B, A, pre_max)
    for refused in ((0, 10, 10), (65536, 10, 10), (1, 0, 10), (1, 10, 0), (1, 10, 4097), (8, 1 << 28, 10), (1, -1, 1)):
        assert host.box_host_workspace_bytes(*refused) == 0 == L.lib().mcav_box_nms_workspace_bytes(*refused)


# ---------------------------------------------------------------------------------------------- the stand-alone program
def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the hardest case (more survivors than pre_max,
    equal scores across the cut, 4096 candidates walked) with and without classes and gathered outputs: every buffer is exactly as large
    as the call may touch, and a finding ends the program with a non-zero status."""
    exe = str(tmp_path / "box_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      "-DBOX_STANDALONE"]) + ["-o", exe])
    a, want = C.call_args(C.HARDEST), C.reference(C.HARDEST)
    B, A = a["scores"].shape
    classes = np.zeros((B, A), np.int32)
    for full in (1, 0):
        head = np.array([B, A, a["pre_max"], a["post_max"], R.MODES[a["mode"]], full, full, workspace_bytes(B, A, a["pre_max"])], np.int64)
        with open(str(tmp_path / "in.bin"), "wb") as f:
            for part in (head, np.array([a["score_thresh"], a["iou_thresh"]], F), a["boxes"], a["scores"]) + ((classes,) if full else ()):
                f.write(np.ascontiguousarray(part).tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        raw = open(str(tmp_path / "out.bin"), "rb").read()
        n = B * a["post_max"]
        assert np.frombuffer(raw, np.int32, 1)[0] == 0 and len(raw) == 4 + 4 * n + 4 * B + (32 * n if full else 0)
        assert np.array_equal(np.frombuffer(raw, np.int32, n, 4).reshape(B, -1), want["keep"])
        assert np.array_equal(np.frombuffer(raw, np.int32, B, 4 + 4 * n), want["num"])
        if full:
            C.same_bits(np.frombuffer(raw, F, 7 * n, 4 + 4 * n + 4 * B).reshape(want["boxes"].shape), want["boxes"])
            C.same_bits(np.frombuffer(raw, F, n, 4 + 4 * n + 4 * B + 28 * n).reshape(want["scores"].shape), want["scores"])


# ---------------------------------------------------------------------------------------------- exported, declared, bound
def test_new_entries_are_exported_declared_and_bound():
    import mcav.lib as L
    import pseudo_lidar  # noqa: F401
    header = open(os.path.join(REPO, "include", "mcav_depth.h")).read()
    handle = ctypes.CDLL(os.path.join(PKG, "mcav", "libmcav_depth.so"))
    for name in ENTRIES:
        assert name + "(" in header and hasattr(handle, name) and name in L._SIGNATURES, name
        assert hasattr(L.lib(), name)
    assert len(L._SIGNATURES["mcav_box_iou"][1]) == 7 and len(L._SIGNATURES["mcav_box_nms"][1]) == 17
    assert "#define MCAV_NMS_MAX_CANDIDATES 4096" in header


# ---------------------------------------------------------------------------------------------- the Python side without a GPU
def test_python_refuses_bad_arguments_without_a_gpu():
    import torch
    import inference
    import mcav.lib as L
    import pseudo_lidar
    from pseudo_lidar import DetectionBatch, boxes_iou3d, boxes_iou_bev, nms
    boxes, scores = torch.zeros(2, 8, 7), torch.zeros(2, 8)
    for fn in (boxes_iou_bev, boxes_iou3d):
        for a, b in ((boxes[0], boxes[1]), (np.zeros((3, 7), F), boxes[0]), (torch.zeros(3, 6), boxes[0]), (boxes, boxes[0]), (boxes[0], None)):
            with pytest.raises(L.MCAVError):
                fn(a, b)
    bad = [dict(boxes=boxes, scores=scores),                                                   # CPU tensors
           dict(boxes=np.zeros((2, 8, 7), F), scores=scores), dict(boxes=torch.zeros(2, 8, 6), scores=scores),
           dict(boxes=torch.zeros(8, 7), scores=scores), dict(boxes=boxes, scores=torch.zeros(2, 9)), dict(boxes=boxes, scores=torch.zeros(2, 8, 0)),
           dict(boxes=boxes, scores=scores, iou="xy"), dict(boxes=boxes, scores=scores, pre_max=4097), dict(boxes=boxes, scores=scores, post_max=0),
           dict(boxes=boxes, scores=scores, pre_max=10, post_max=11), dict(boxes=boxes, scores=scores, score_thresh=float("nan")),
           dict(boxes=boxes, scores=scores, iou_thresh=float("nan")), dict(boxes=torch.zeros(0, 8, 7), scores=torch.zeros(0, 8))]
    for kw in bad:
        with pytest.raises(L.MCAVError):
            nms(**kw)
    assert callable(inference.Inference.detections) and pseudo_lidar.DetectionBatch is DetectionBatch
