"""CPU: the float64 definitions of tests/warp_ops_ref.py pinned to the committed goldens (the reference's own float32 results) and to
oracle.geometry / oracle.losses evaluated in float64, what the cases of tests/warp_ops_cases.py promise, and the error bounds applied to a
float32 evaluation known to be right (the CPU oracle): a bound that evaluation missed would be wrong, not tight."""
import math

import numpy as np
import pytest
import torch

import warp_ops_cases as C
import warp_ops_ref as R
from conftest import rel_err
from oracle import geometry as og
from oracle import losses as ol

F64 = torch.float64
WARP_CASES = [(s, k, inv) for s in C.SHAPES for k in C.POSE_KINDS for inv in (0, 1)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close64(a, b, tol=1e-10):
    a, b = torch.as_tensor(a).detach().to(F64), torch.as_tensor(b).detach().to(F64)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------- the definitions are the reference's
def test_geometry_definitions_match_the_goldens(golden):
    g = golden("loss_small.npz")
    K, Dt, p = T(g["K"]), T(g["depth_t"]), T(g["poses"])
    assert rel_err(R.disp_to_depth(T(g["disp_t"]))[:, 0], Dt) < 1e-6
    X = R.reconstruct(Dt, K)
    assert rel_err(X, g["cam_points"]) < 1e-6
    assert rel_err(R.pose_to_matrix(p[:, 0]), g["Tcw0"]) < 1e-6
    assert rel_err(R.pose_to_matrix(p[:, 0], True), g["Tcw0_inv"]) < 1e-6
    assert rel_err(R.invert_pose(T(g["Tcw0"])), g["Tcw0_inv"]) < 1e-6
    assert rel_err(R.project(X, K, R.pose_to_matrix(p[:, 0])), g["grid0"]) < 1e-6
    Dr = R.disp_to_depth(T(g["disp_r"]))[:, 0]
    assert rel_err(R.inverse_warp(T(g["ref0"]), Dt, p[:, 0], K, False), g["warp0"]) < 1e-5
    assert rel_err(R.inverse_warp(T(g["ref1"]), Dt, p[:, 1], K, False), g["warp1"]) < 1e-5
    assert rel_err(R.inverse_warp(T(g["tgt"]), Dr, p[:, 0], K, True), g["warp2"]) < 1e-5
    e = golden("warp_edge.npz")
    assert rel_err(R.inverse_warp(T(e["img"]), T(e["depth"]), T(e["pose_big"]), T(e["K"]), False), e["warp_big"]) < 1e-4
    assert rel_err(R.inverse_warp(T(e["img"]), T(e["depth"]), T(e["pose_big"]), T(e["K"]), True), e["warp_big_inv"]) < 1e-4


def test_ssim_and_smoothness_definitions_match_the_goldens(golden):
    g = golden("ssim.npz")
    x, y = T(g["x"]), T(g["y"])
    x, y = x.reshape(-1, *x.shape[2:]), y.reshape(-1, *x.shape[2:])
    # the golden is a float32 evaluation: E[x^2] - mu^2 cancels in it, so it is held to the bound of that cancellation, per element
    err = (T(g["ssim"]).reshape(x.shape).to(F64) - R.ssim(x, y)).abs()
    assert bool((err <= R.ssim_bound(x, y)).all()), float((err / R.ssim_bound(x, y)).max())
    assert float(err.max()) < 1e-4
    assert float(R.ssim(x, x).max()) == 0.0
    s = golden("smooth.npz")
    depths = [R.disp_to_depth(T(s["disp%d" % i])).float() for i in range(2)]
    loss = sum(R.smooth(D, 1.0 / 2.3 ** i)[0] for i, D in enumerate(depths))
    assert abs(loss - float(s["loss"])) < 1e-5 * abs(float(s["loss"]))


@pytest.mark.parametrize("shape,kind,inv", WARP_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_geometry_definitions_are_the_oracle_in_float64(shape, kind, inv):
    c = C.warp_case(*shape, kind)
    D, p, K, img = c["depth"].to(F64), c["pose"].to(F64), c["K"], c["img"].to(F64)
    assert close64(R.pose_to_matrix(p, inv), og.pose_to_matrix(p, invert=bool(inv)))
    assert close64(R.invert_pose(og.pose_to_matrix(p)), og.invert_rigid(og.pose_to_matrix(p)))
    assert close64(R.reconstruct(D, K), og.reconstruct(D, K))
    X, Tcw = og.reconstruct(D, K), og.pose_to_matrix(p, invert=bool(inv))
    if kind != "away":
        assert close64(R.project(X, K, Tcw), og.project(X, K, Tcw), 1e-9)
    Dg, pg = D.clone().requires_grad_(), p.clone().requires_grad_()
    Do, po = D.clone().requires_grad_(), p.clone().requires_grad_()
    a, b = R.inverse_warp(img, Dg, pg, K, inv), og.inverse_warp(img, Do, po, K, inv)
    assert close64(a, b, 1e-9)
    go = c["grad_out"].to(F64)
    (a * go).sum().backward()
    (b * go).sum().backward()
    assert close64(Dg.grad, Do.grad, 1e-8) and close64(pg.grad, po.grad, 1e-8)


@pytest.mark.parametrize("angle", C.ANGLES)
def test_pose_definition_is_the_oracle_in_float64(angle):
    p = C.pose_vectors(65, angle, 5).to(F64)
    for inv in (False, True):
        assert close64(R.pose_to_matrix(p, inv), og.pose_to_matrix(p, invert=inv))
    if angle == 0.0:
        assert torch.equal(R.pose_to_matrix(p)[:, :3, :3], torch.eye(3, dtype=F64).repeat(65, 1, 1))


def test_ssim_and_smoothness_definitions_are_the_oracle_in_float64():
    for (B, H, W) in C.SHAPES:
        for kind in ("random", "same", "constant", "conditioned"):
            x, y = (t.to(F64) for t in C.ssim_case(3 * B, H, W, kind))
            c1, c2 = float(np.float32(1e-4)), float(np.float32(9e-4))      # (the entry takes them as floats)
            assert close64(R.ssim(x, y), ol.ssim_distance(x[None], y[None], c1, c2)[0], 1e-11), (B, H, W, kind)
    for (B, H, W) in C.SMOOTH_SHAPES:
        D = C.dyadic_depth(B, H, W).to(F64).requires_grad_()
        want = ol.smooth_loss(D)
        want.backward()
        loss, grad = R.smooth(D.detach())
        assert abs(loss - float(want.detach())) <= 1e-12 * float(want.detach()) and close64(grad, D.grad, 1e-12)


# ---------------------------------------------------------------------------------------------- the cases keep their promises
def positions32(c, inv):
    """the float32 CPU oracle's sampling positions, un-normalised in float32 as F.grid_sample does"""
    B, H, W = c["depth"].shape
    grid = og.project(og.reconstruct(c["depth"], c["K"]), c["K"], og.pose_to_matrix(c["pose"], invert=bool(inv)))
    return (grid[..., 0] + 1) / 2 * (W - 1), (grid[..., 1] + 1) / 2 * (H - 1)


def measured_delta(shape, kind, inv):
    c = C.warp_case(*shape, kind)
    B, H, W = shape
    ix, iy = R.warp_position(c["depth"], c["pose"], c["K"], inv)
    jx, jy = positions32(c, inv)
    near = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    d = (jx.to(F64) - ix).abs() + (jy.to(F64) - iy).abs()
    return float(d[near].max()) if bool(near.any()) else 0.0


def round_up_two_digits(v):
    if v == 0.0:
        return 0.0
    e = 10.0 ** (math.floor(math.log10(v)) - 1)
    return math.ceil(v / e) * e


def test_recorded_deltas():
    for shape, kind, inv in WARP_CASES:
        want = round_up_two_digits(2 * measured_delta(shape, kind, inv))
        got = C.DELTAS[(shape, kind, inv)]
        assert abs(got - want) <= 1e-9 * max(want, 1e-30), "DELTAS[%s] = %.2g, measured %.2g" % ((shape, kind, inv), got, want)


def test_cases_cover_what_they_are_for():
    B, H, W = 3, 17, 70
    for inv in (0, 1):
        c = C.warp_case(B, H, W, "roll")
        ix, iy = R.warp_position(c["depth"], c["pose"], c["K"], inv)
        ok_y, ok_x = (iy > 0) & (iy < H - 1), (ix > 0) & (ix < W - 1)
        assert bool(((ix > -1) & (ix < 0) & ok_y).any()) and bool(((ix > W - 1) & (ix < W) & ok_y).any())       # a tap straddling the left / right border
        assert bool(((iy > -1) & (iy < 0) & ok_x).any()) and bool(((iy > H - 1) & (iy < H) & ok_x).any())       # ... the top / bottom border
    for shape in C.SHAPES:
        for inv in (0, 1):
            c = C.warp_case(*shape, "away")
            ix, iy = R.warp_position(c["depth"], c["pose"], c["K"], inv)
            assert bool(((ix <= -1) | (ix >= shape[2])).all())                                                    # every pixel out of view
            for kind in ("zero", "small", "roll"):
                c = C.warp_case(*shape, kind)
                _, cam = R._camera(R.reconstruct(c["depth"], c["K"]), c["K"], R.pose_to_matrix(c["pose"], inv))
                assert float(cam[:, 2].min()) >= 0.5                                                              # the bounded project cases
    c = C.warp_case(B, H, W, "zero")
    _, cam = R._camera(R.reconstruct(c["depth"], c["K"]), c["K"], R.pose_to_matrix(C.behind_camera_pose(B)))
    assert bool((cam[:, 2] < 0).any()) and bool(torch.isfinite(cam).all())
    for (B, H, W) in C.SHAPES:
        x, y = (t.to(F64)[None] for t in C.ssim_case(3 * B, H, W, "conditioned"))
        box = lambda t: torch.nn.functional.avg_pool2d(R._reflect_pad(t), 3, 1)
        if H >= 3 and W >= 3:
            assert float((box(x * x) - box(x) ** 2).min()) >= 0.01 and float((box(y * y) - box(y) ** 2).min()) >= 0.01
    for (B, H, W) in C.SMOOTH_SHAPES:
        D = C.dyadic_depth(B, H, W)
        for a, b in zip(R.smooth_terms(D), R.smooth_terms(D.to(F64))):
            assert torch.equal(a.to(F64), b)                                                                      # exact in float32
        assert bool((R.smooth_terms(D)[0] == 0).any()) and bool((R.smooth_terms(D)[3] == 0).any())              # exact zeros occur
        assert R.smooth(C.dyadic_depth(B, H, W, constant=True))[0] == 0.0


# ---------------------------------------------------------------------------------------------- the bounds, on a float32 evaluation known to be right
@pytest.mark.parametrize("shape,kind,inv", WARP_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_bounds_hold_for_the_float32_oracle(shape, kind, inv):
    c = C.warp_case(*shape, kind)
    D, p, K, img = c["depth"], c["pose"], c["K"], c["img"]
    X32 = og.reconstruct(D, K)
    assert bool(((X32.to(F64) - R.reconstruct(D, K)).abs() <= R.reconstruct_bound(D, K)).all())
    T32 = og.pose_to_matrix(p, invert=bool(inv))
    rot, tb, _ = R.pose_bounds(p, inv)
    err = (T32.to(F64) - R.pose_to_matrix(p, inv)).abs()
    assert float(err[:, :3, :3].max()) <= rot and bool((err[:, :3, 3] <= tb).all())
    if kind != "away":
        g32 = og.project(X32, K, T32)
        assert bool(((g32.to(F64) - R.project(X32, K, T32)).abs() <= R.project_bound(X32, K, T32)).all())
    w32 = og.inverse_warp(img, D, p, K, inv)
    bound = R.inverse_warp_bound(img, D, p, K, inv, C.DELTAS[(shape, kind, inv)])
    assert bool(((w32.to(F64) - R.inverse_warp(img, D, p, K, inv)).abs() <= bound).all())


def test_ssim_bound_holds_for_the_float32_oracle():
    for (B, H, W) in C.SHAPES:
        if H < 3 or W < 3:
            continue
        x, y = C.ssim_case(3 * B, H, W, "conditioned")
        got = ol.ssim_distance(x[None], y[None])[0]
        assert bool(((got.to(F64) - R.ssim(x, y)).abs() <= R.ssim_bound(x, y)).all()), (B, H, W)
