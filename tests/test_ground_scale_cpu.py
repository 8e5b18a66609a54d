"""CPU: the ground-plane scale estimator (include/mcav_depth.h: mcav_ground_scale, pseudo_lidar.ground_scale).  The header
csrc/ground_math.h compiled for the host against the float32 restatement (tests/ground_scale_ref.py), bit for bit, on the cases the GPU
tests run (tests/ground_scale_cases.py), once more as a stand-alone program under the address and undefined-behaviour sanitizers; the
float32 restatement against the same definition in float64; the analytic answer of the scenes; properties of the restatement; the
entry points' refusals, which happen before anything touches a device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import ground_scale_cases as C
import ground_scale_ref as G
from conftest import PKG, REPO

SRC = os.path.join(REPO, "tests", "ground_hostcheck", "ground_hostcheck.cpp")
TIE = 1e-4                     # |n.y - cos_max| below this in float64: float32 may fall on the other side


def bits_equal(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


def test_cases_hold_what_they_promise():
    counts = np.concatenate([C.reference(c)[0][:, 2] for c in C.CASES]).astype(int)
    assert (counts % 2 == 0).any() and (counts % 2 == 1).any() and (counts == 0).any()
    rows = C.reference("noground")[0]
    assert rows[:, 3].tolist() == [1, 0, 1] and rows[1, 2] == 0 and np.isnan(rows[1, :2]).all()
    h, w = C.SPECS["tiles"]["hw"]
    assert (h - 2) % 8 and (w - 2) % 32 and h - 2 > 16 and w - 2 > 64              # the kernel's 8 x 32 tiles over the interior
    assert C.reference("full")[0][:, 2].min() > 50000
    a = C.build("special")
    rows, mask = C.reference("special")[:2]
    assert np.isfinite(rows).all() and (rows[:, 3] == 1).all()
    for b, pts in enumerate(a["special"]):
        assert np.isnan(a["m"][b]).sum() == 1 and np.isposinf(a["m"][b]).sum() == 1 and (a["m"][b] == np.float32(-0.05)).sum() == 1
        # a NaN takes its whole neighbourhood out (every difference to it is NaN); +inf is depth 0 and -0.05 a depth of -2 m: finite
        # points far from the road, which are never ground themselves and leave a neighbour in only where its other normals outvote them
        (r, c) = pts[0]
        assert not mask[b, r - 1:r + 2, c - 1:c + 2].any()
        for r, c in pts:
            assert not mask[b, r, c] and mask[b, r - 2:r + 3, c - 2:c + 3].any()                                 # planted on the ground
    assert C.reference("box")[1][:, :C.SPECS["box"]["hw"][0] // 2].sum() == 0
    assert C.reference("min_at")[0][:, 3].tolist() == [1, 1, 1] and C.reference("min_above")[0][:, 3].sum() == 2


# ---------------------------------------------------------------------------------------------- csrc/ground_math.h on the host
def host_flags(extra=()):
    return ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc")] + list(extra) + [SRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ground_hostcheck") / "libground_hostcheck.so")
    subprocess.check_call(host_flags(["-O2", "-shared", "-fPIC"]) + ["-o", so])
    lib = ctypes.CDLL(so)
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.gs_host_ground_scale.argtypes = [p, i, i, i, p, p, p, f, f, i, f, i, p, p, p]
    lib.gs_host_scalars_ok.argtypes = [f, f, i, i]
    return lib


def flat_args(a):
    m = np.ascontiguousarray(a["m"], np.float32)
    B = m.shape[0]
    sizes = np.ascontiguousarray(a["sizes"], np.int32).reshape(B, 2)
    calib = np.ascontiguousarray(np.concatenate([np.reshape(a["P"], (B, 12)), np.reshape(a["T"], (B, 16))], axis=1), np.float64)
    boxes = None if a["boxes"] is None else np.ascontiguousarray(a["boxes"], np.int32).reshape(B, 4)
    return m, sizes, calib, boxes


@pytest.mark.parametrize("case", C.CASES)
def test_header_matches_restatement(host, case):
    a = C.build(case)
    want_rows, want_mask, want_hgt, _ = C.reference(case)
    m, sizes, calib, boxes = flat_args(a)
    B, h, w = m.shape
    rows = np.full((B, 4), -7.0, np.float32)
    mask = np.full((B, h, w), 9, np.uint8)
    hgt = np.zeros((B, h, w), np.float32)
    rc = host.gs_host_ground_scale(m.ctypes.data, B, h, w, sizes.ctypes.data, calib.ctypes.data, None if boxes is None else boxes.ctypes.data,
                                   a["camera_height"], G.cos_max_of(a["max_angle_deg"]), a["min_ground"], a["fallback"],
                                   1 if a["input"] == "depth" else 0, rows.ctypes.data, mask.ctypes.data, hgt.ctypes.data)
    assert rc == 0
    assert np.array_equal(mask, want_mask)
    bits_equal(hgt[mask == 1], want_hgt[want_mask == 1])
    bits_equal(rows, want_rows)


def test_standalone_program_under_sanitizers(tmp_path):
    """The same source as a program of its own, built with -fsanitize=address,undefined, on the case with three images of different
    sizes and a box that reaches outside the plane: a finding ends the program with a non-zero status."""
    exe = str(tmp_path / "ground_hostcheck")
    subprocess.check_call(host_flags(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGS_STANDALONE"]) +
                          ["-o", exe])
    case = "box"
    a = C.build(case)
    m, sizes, calib, boxes = flat_args(a)
    B, h, w = m.shape
    head = np.array([B, h, w, a["min_ground"], 0, 1, 0, 0], np.int32)
    sc = np.array([a["camera_height"], G.cos_max_of(a["max_angle_deg"]), a["fallback"], 0], np.float32)
    with open(str(tmp_path / "in.bin"), "wb") as f:
        for part in (head, sc, sizes, calib, boxes, m):
            f.write(part.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    want_rows, want_mask, want_hgt, _ = C.reference(case)
    assert np.frombuffer(raw, np.int32, 1)[0] == 0
    bits_equal(np.frombuffer(raw, np.float32, 4 * B, 4).reshape(B, 4), want_rows)
    mask = np.frombuffer(raw, np.uint8, B * h * w, 4 + 16 * B).reshape(B, h, w)
    hgt = np.frombuffer(raw, np.float32, B * h * w, 4 + 16 * B + B * h * w).reshape(B, h, w)
    assert np.array_equal(mask, want_mask)
    bits_equal(hgt[mask == 1], want_hgt[want_mask == 1])
    assert (hgt[mask == 0].view(np.uint32) == 0xFFFFFFFF).all()


# ---------------------------------------------------------------------------------------------- float32 against float64
def test_float32_definition_against_float64():
    """The float32 definition against the same definition in float64, per image of every case: the masks agree outside the tie pixels
    (|n.y - cos_max| < 1e-4 in float64), the ties are at most 1 % of the interior, and the scales differ by at most 2.8e-6 relative: four
    times the largest difference measured on these cases, 7.0e-7 (the test prints the figures before it asserts)."""
    worst_scale, worst_tie = 0.0, 0.0
    for case in C.CASES:
        a = C.build(case)
        r32, m32 = C.reference(case)[:2]
        r64, m64, _, ny64 = C.reference(case, np.float64)
        cm = np.float64(G.cos_max_of(a["max_angle_deg"]))
        for b in range(len(r32)):
            tie = np.abs(ny64[b] - cm) < TIE
            share = tie[1:-1, 1:-1].mean()
            differ = int(((m32[b] != m64[b]) & ~tie).sum())
            both = r32[b, 3] == 1 and r64[b, 3] == 1
            rel = abs(float(r32[b, 0]) / float(r64[b, 0]) - 1.0) if both else 0.0
            print("%s[%d]: tie share %.4f, masks differ outside ties at %d pixels, counts %d / %d, scale difference %.3g"
                  % (case, b, share, differ, r32[b, 2], r64[b, 2], rel))
            worst_scale, worst_tie = max(worst_scale, rel), max(worst_tie, share)
            assert differ == 0 and share <= 0.01, (case, b)
            assert r32[b, 3] == r64[b, 3] or abs(int(r32[b, 2]) - int(r64[b, 2])) <= tie.sum(), (case, b)
            assert rel <= 2.8e-6, (case, b, rel)
    print("largest scale difference %.3g, largest tie share %.4f" % (worst_scale, worst_tie))


def test_scale_is_the_analytic_one():
    """Within 1 % of s_true * sqrt(1 + 0.03^2 + 0.01^2) (times camera_height / 1.65 where a case changes it) on every image with ground
    and sigma <= 1e-3, for s_true in {0.37, 1, 5.3}: the estimate follows the prediction's scale."""
    seen = set()
    for case in C.SPECS:
        a = C.build(case)
        rows = C.reference(case)[0]
        for b, s_true in enumerate(a["s_true"]):
            if not a["valid"][b]:
                continue
            want = s_true * C.ANALYTIC * a["camera_height"] / C.CAMERA_HEIGHT
            print("%s[%d]: scale %.6f, analytic %.6f" % (case, b, rows[b, 0], want))
            assert rows[b, 3] == 1 and abs(rows[b, 0] / want - 1.0) <= 0.01, (case, b)
            seen.add(s_true)
    assert seen == {0.37, 1.0, 5.3}


# ---------------------------------------------------------------------------------------------- properties of the restatement
def test_mirrored_input_gives_the_same_ground():
    a = C.build("odd")
    rows = C.reference("odd")[0]
    P = a["P"].copy()
    for b, (Hb, Wb) in enumerate(a["sizes"]):
        P[b, 0, 2] = Wb - 1 - P[b, 0, 2]
    got = G.ground_scale(a["m"][:, :, ::-1], **dict(C.call_kw(a), P=P))[0]
    assert np.array_equal(got[:, 2:], rows[:, 2:])
    assert np.abs(got[:, 1] / rows[:, 1] - 1.0).max() <= 1e-6


def test_box_restricts_the_count():
    a = C.build("odd")
    h, w = a["m"].shape[1:]
    full_rows, full_mask = C.reference("odd")[:2]
    rows, mask = G.ground_scale(a["m"], **dict(C.call_kw(a), boxes=(0, h, 0, w // 2), min_ground=1))[:2]
    assert (mask[:, :, w // 2:] == 0).all() and np.array_equal(mask[:, :, :w // 2], full_mask[:, :, :w // 2])
    assert (rows[:, 2] < full_rows[:, 2]).all() and (rows[:, 2] > 0).all()
    empty = G.ground_scale(a["m"], **dict(C.call_kw(a), boxes=(5, 5, 0, w)))[0]
    assert (empty[:, 2] == 0).all() and (empty[:, 3] == 0).all()


def test_min_ground_boundary():
    at, above, plain = C.reference("min_at")[0], C.reference("min_above")[0], C.reference("odd")[0]
    k = int(np.argmin(plain[:, 2]))
    bits_equal(at, plain)
    assert above[k, 3] == 0 and above[k, 0] == np.float32(-3.0) and above[k, 1] == plain[k, 1] and above[k, 2] == plain[k, 2]
    keep = np.arange(len(plain)) != k
    bits_equal(above[keep], plain[keep])


# ---------------------------------------------------------------------------------------------- the entry points without a device
def test_entry_rejects_bad_arguments_without_a_device(host):
    import mcav.lib as L
    import pseudo_lidar  # noqa: F401  (registers the signatures)
    h = L.lib()
    fake = ctypes.c_void_p(0x1000)             # never dereferenced: the checks fail first
    ok = dict(m=fake, B=2, h=8, w=16, sizes=fake, calib=fake, boxes=None, camera_height=1.65, cos_max=0.99, min_ground=100,
              fallback=float("nan"), flags=0, rows=fake, mask=None, ws=fake, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return h.mcav_ground_scale(a["m"], a["B"], a["h"], a["w"], a["sizes"], a["calib"], a["boxes"], a["camera_height"], a["cos_max"],
                                   a["min_ground"], a["fallback"], a["flags"], a["rows"], a["mask"], a["ws"], a["ws_bytes"], None)
    bad = [dict(m=None), dict(sizes=None), dict(calib=None), dict(rows=None), dict(ws=None), dict(h=2), dict(w=2), dict(B=0), dict(B=-1),
           dict(B=1 << 15, h=256, w=256), dict(camera_height=0.0), dict(camera_height=-1.0), dict(camera_height=float("nan")),
           dict(camera_height=float("inf")), dict(cos_max=0.0), dict(cos_max=1.0000001), dict(cos_max=float("nan")), dict(min_ground=0),
           dict(flags=2), dict(flags=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    need = h.mcav_ground_scale_workspace_bytes(2, 8, 16)
    assert need >= 4 * 2 * 6 * 14 and call(ws_bytes=need - 1) == -2
    assert h.mcav_ground_scale_workspace_bytes(2, 2, 16) == 0 and h.mcav_ground_scale_workspace_bytes(1 << 15, 256, 256) == 0
    assert host.gs_host_scalars_ok(1.65, 1.0, 1, 1) == 1 and host.gs_host_scalars_ok(1.65, 1.0, 1, 3) == 0
    # the scaled entries refuse what the plain ones refuse
    assert h.mcav_pl_batch_project_scaled(None, 1, 8, 16, 8, 16, fake, fake, None, None, None, 0, 0, 1.0, fake, 1.0, 1.0, 0, 0, fake, 128,
                                          fake, fake, 1 << 20, None) == -1
    import evaluate  # noqa: F401
    assert h.mcav_eval_depth_scaled(None, fake, 1, 8, 16, 8, 16, fake, fake, 1e-3, 80.0, 1.0, fake, 0, fake, fake, 1 << 20, None) == -1


def test_python_surface_refuses_without_a_gpu():
    import torch
    import inference
    import mcav.lib as L
    from pseudo_lidar import PseudoLiDAR, ground_scale
    P = C.scaled_P(C.DATES[0], 8, 16)
    with pytest.raises(L.MCAVError):
        ground_scale(torch.zeros(1, 8, 16), P=P)                                     # a CPU tensor
    with pytest.raises(L.MCAVError):
        ground_scale(np.zeros((1, 8, 16), np.float32), P=P)
    with pytest.raises(L.MCAVError):
        PseudoLiDAR.from_matrices(C.velo_T(C.DATES[0]), P, 0).ground_scale(torch.zeros(8, 16))
    assert inference.scale_argument("ground") == "ground" and inference.scale_argument("5.4") == 5.4
    with pytest.raises(ValueError):
        inference.scale_argument("road")
    from trainer import Trainer
    v = Trainer.validation_config({})
    assert v["scaling"] == "median" and v["median_scaling"] is True and v["camera_height"] == 1.65
    assert Trainer.validation_config({"median_scaling": False})["scaling"] == "none"
    v = Trainer.validation_config({"scaling": "ground", "camera_height": 1.7})
    assert v["scaling"] == "ground" and v["median_scaling"] is False and math.isclose(v["camera_height"], 1.7)
    assert Trainer.validation_config({"scaling": "none"})["median_scaling"] is False
    assert Trainer.validation_config({"scaling": "none", "median_scaling": False})["scaling"] == "none"
    for bad in ({"scaling": "lidar"}, {"camera_height": 0}, {"scaling": "median", "median_scaling": False},
                {"scaling": "ground", "median_scaling": True}, {"scaling": "none", "median_scaling": True}):
        with pytest.raises(ValueError):
            Trainer.validation_config(bad)


def test_reduce_rows_reports_the_ground_statistics():
    import torch
    import evaluate as E
    rows = torch.rand(4, 11)
    rows[:, 9] = 5
    g = torch.tensor([[1.0, 1.6, 300, 1], [float("nan"), float("nan"), 0, 0], [3.0, 0.5, 200, 1], [2.0, 0.8, 150, 1]])
    plain, with_g = E.reduce_rows(rows), E.reduce_rows(rows, [g[:1], g[1:]])
    assert {k: with_g[k] for k in plain} == plain
    assert with_g["ground_fallbacks"] == 1 and with_g["ground_scale_mean"] == 2.0
    assert math.isclose(with_g["ground_scale_std"], float(np.std([1.0, 3.0, 2.0])))
