"""GPU: the standalone geometry, SSIM and smoothness entry points of csrc/warp_loss.hip through the C ABI on guarded windows, against the
float64 definitions of tests/warp_ops_ref.py at the cases of tests/warp_ops_cases.py: per-element bounds where the operation is smooth
(derived in warp_ops_ref), the arbiter rule (HIP as close to float64 as the float32 CPU oracle is, 1e-6 perturbation envelope, factor 2,
floor 2e-6) where it is only piecewise smooth or cancels.  Each test prints its worst figure (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import warp_ops_cases as C
import warp_ops_ref as R
from arbiter import Verdicts, perturb_tensor
from guarded import Guarded
from oracle import geometry as og
from oracle import losses as ol

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
U = R.U
INVALID = -1
ids = lambda v: str(v).replace(" ", "")


@pytest.fixture(scope="module")
def h():
    from mcav import lib as L
    import geometry.pose_geometry  # noqa: F401  (registers the pose entry points' signatures)
    return L.lib()


def P(t):
    from mcav import lib as L
    return L.ptr(t.t if isinstance(t, Guarded) else t)


def stream():
    from mcav import lib as L
    return L.stream()


def workspace(h, B, H, W):
    return Guarded((h.mcav_warp_loss_workspace_bytes(B, H, W),), torch.uint8, init=0, band=256)


def done(*windows):
    torch.cuda.synchronize()
    for g in windows:
        assert g.intact(), "a store outside a window of shape %s" % (tuple(g.t.shape),)
    return [g.cpu() for g in windows]


def k_arg(K, f64):
    K = K.to(F64 if f64 else torch.float32).to(DEV).contiguous()
    return K, (1 if f64 else 0)


def within(name, got, want, bound):
    """|got - want| <= bound per element; prints the worst ratio."""
    err = (got.to(F64) - want).abs()
    assert bool(torch.isfinite(got).all()), "%s: an element was not written" % name
    ratio = float((err / bound.clamp_min(1e-300)).max()) if torch.is_tensor(bound) else float(err.max()) / max(bound, 1e-300)
    print("%s: worst |err| %.3e, %.2f of its bound" % (name, float(err.max()), ratio))
    assert bool((err <= bound).all()), "%s: %.2f of the bound at %s" % (name, ratio, (err > bound).nonzero()[:4].tolist())


# ---------------------------------------------------------------------------------------------- poses
def pose_case(h, angle, invert, B):
    pose = C.pose_vectors(B, angle, 11)
    if angle == 0.0:
        pose[:, 3:] = C.pose_vectors(B, 1.0, 12)[:, 3:]
    out = Guarded((B, 4, 4))
    assert h.mcav_pose_to_matrix(P(pose.to(DEV)), B, invert, P(out), stream()) == 0
    return pose, done(out)[0]


@pytest.mark.parametrize("B", C.POSE_BATCHES)
@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("angle", C.ANGLES)
def test_pose_to_matrix(h, angle, invert, B):
    """Rotation entries within 16 u; the translation exact when not inverted, and inverted within 8 u sum_j |R_ji t_j| + 16 u sum_j |t_j|
    (warp_ops_ref.pose_bounds: the product sum, and the rotation's own error times the translation); the zero vector gives exactly the
    identity and the exact translation."""
    pose, T = pose_case(h, angle, invert, B)
    want = R.pose_to_matrix(pose, invert)
    rot, tb, _ = R.pose_bounds(pose, invert)
    assert torch.equal(T[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).repeat(B, 1))
    if angle == 0.0:
        assert torch.equal(T[:, :3, :3], torch.eye(3).repeat(B, 1, 1))
        assert torch.equal(T[:, :3, 3], -pose[:, 3:] if invert else pose[:, 3:])
    within("pose_to_matrix angle %g invert %d B %d rotation (u = %.1e)" % (angle, invert, B, U), T[:, :3, :3], want[:, :3, :3], rot)
    within("pose_to_matrix angle %g invert %d B %d translation" % (angle, invert, B), T[:, :3, 3], want[:, :3, 3], tb)


@pytest.mark.parametrize("B", C.POSE_BATCHES)
@pytest.mark.parametrize("angle", C.ANGLES)
def test_inverse_translation_within_8u_of_its_product_sum(h, angle, B):
    """The translation of the inverted pose held to 8 u sum_j |R_ji t_j| ALONE, against float64.  Formed from the float32 rotation, as the
    kernel first did, t' = -R^T t missed this at angle pi - 1e-3, B = 65 (measured on MI355X: 9.7 u sum_j |R_ji t_j|, |err| 1.9e-7,
    samples 10 and 61): the rotation's entries are 7.3 u off there (inside their own 16 u; the argument of sinf / cosf carries the error
    of the norm), and where a column of R is small that error times t is larger than the whole product sum.  The entry now forms t' from
    a float64 Rodrigues and rounds once (csrc/warp_loss.hip: inverse_translation_f64)."""
    pose, T = pose_case(h, angle, 1, B)
    _, _, products = R.pose_bounds(pose, 1)
    within("inverse translation angle %g B %d (product sum alone)" % (angle, B), T[:, :3, 3], R.pose_to_matrix(pose, 1)[:, :3, 3], products)


@pytest.mark.parametrize("B", C.POSE_BATCHES)
@pytest.mark.parametrize("angle", C.ANGLES)
def test_invert_pose(h, angle, B):
    """[R | t] -> [R^T | -R^T t]: the rotation block is a copy, the translation within 8 u sum_j |R_ji t_j|."""
    T = R.pose_to_matrix(C.pose_vectors(B, angle, 13)).float()
    out = Guarded((B, 4, 4))
    assert h.mcav_invert_pose(P(T.to(DEV)), B, P(out), stream()) == 0
    (Ti,) = done(out)
    want = R.invert_pose(T)
    assert torch.equal(Ti[:, :3, :3], T[:, :3, :3].transpose(1, 2).contiguous()) and torch.equal(Ti[:, 3], T[:, 3])
    bound = 8 * U * (T[:, :3, :3].transpose(1, 2).to(F64).abs() * T[:, None, :3, 3].to(F64).abs()).sum(2)
    within("invert_pose angle %g B %d translation" % (angle, B), Ti[:, :3, 3], want[:, :3, 3], bound)


def test_pose_entries_refuse_bad_arguments(h):
    out = Guarded((1, 4, 4))
    pose = torch.zeros(1, 6, device=DEV)
    assert h.mcav_pose_to_matrix(P(pose), 0, 0, P(out), stream()) == INVALID
    assert h.mcav_pose_to_matrix(None, 1, 0, P(out), stream()) == INVALID
    assert h.mcav_invert_pose(P(out), 0, P(out), stream()) == INVALID
    torch.cuda.synchronize()
    assert out.untouched()


# ---------------------------------------------------------------------------------------------- reconstruct / project
@pytest.mark.parametrize("f64", [1, 0])
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_reconstruct(h, shape, f64):
    B, H, W = shape
    c = C.warp_case(B, H, W, "zero")
    K, flag = k_arg(c["K"], f64)
    out, ws = Guarded((B, 3, H, W)), workspace(h, B, H, W)
    assert h.mcav_reconstruct(P(c["depth"].to(DEV)), P(K), B, H, W, flag, P(out), P(ws), ws.t.numel(), stream()) == 0
    X, _ = done(out, ws)
    Kc = K.cpu()
    within("reconstruct %s K f%d" % (shape, 64 if f64 else 32), X, R.reconstruct(c["depth"], Kc), R.reconstruct_bound(c["depth"], Kc))


@pytest.mark.parametrize("f64", [1, 0])
@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("kind", ["zero", "small", "roll"])
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_project(h, shape, kind, inv, f64):
    B, H, W = shape
    c = C.warp_case(B, H, W, kind)
    K, flag = k_arg(c["K"], f64)
    X = R.reconstruct(c["depth"], c["K"]).float()
    Tcw = R.pose_to_matrix(c["pose"], inv).float()
    out = Guarded((B, H, W, 2))
    assert h.mcav_project(P(X.to(DEV)), P(K), P(Tcw.to(DEV)), B, H, W, flag, P(out), stream()) == 0
    (grid,) = done(out)
    Kc = K.cpu()
    within("project %s %s inv %d K f%d" % (shape, kind, inv, 64 if f64 else 32), grid, R.project(X, Kc, Tcw), R.project_bound(X, Kc, Tcw))


def test_project_behind_the_camera(h):
    """z < 0, finite: c / (z + 1e-5) has no bound worth stating near z = 0, so the arbiter rule against the float32 CPU oracle."""
    B, H, W = 3, 17, 70
    c = C.warp_case(B, H, W, "zero")
    X = R.reconstruct(c["depth"], c["K"]).float()
    Tcw = R.pose_to_matrix(C.behind_camera_pose(B)).float()
    out = Guarded((B, H, W, 2))
    assert h.mcav_project(P(X.to(DEV)), P(c["K"].to(DEV)), P(Tcw.to(DEV)), B, H, W, 1, P(out), stream()) == 0
    (grid,) = done(out)
    assert bool(torch.isfinite(grid).all())
    v = Verdicts(factor=2.0, floor=2e-6)
    v.add("project behind the camera", grid, og.project(X, c["K"], Tcw), R.project(X, c["K"], Tcw),
          [R.project(perturb_tensor(X.to(F64), 1e-6, 100 + e), c["K"], perturb_tensor(Tcw.to(F64), 1e-6, 200 + e)) for e in range(2)])
    v.check("test_project_behind_the_camera")


def test_geometry_entries_refuse_small_shapes(h):
    """H < 2 or W < 2 (project, inverse warp: the normalisation divides by size - 1): MCAV_E_INVALID, nothing written."""
    B = 1
    depth, img, pose = torch.ones(B, 4, 4, device=DEV), torch.ones(B, 3, 4, 4, device=DEV), torch.zeros(B, 6, device=DEV)
    K, T = C.intrinsics(B, 4, 4).to(DEV), torch.eye(4, device=DEV).repeat(B, 1, 1)
    out, gd, gp, grid, ws = Guarded((B, 3, 4, 4)), Guarded((B, 4, 4)), Guarded((B, 6)), Guarded((B, 4, 4, 2)), workspace(h, B, 4, 4)
    for H, W in ((1, 4), (4, 1)):
        assert h.mcav_project(P(img), P(K), P(T), B, H, W, 1, P(grid), stream()) == INVALID
        assert h.mcav_inverse_warp_fwd(P(img), P(depth), P(pose), P(K), B, H, W, 0, 1, P(out), P(ws), ws.t.numel(), stream()) == INVALID
        assert h.mcav_inverse_warp_bwd(P(img), P(depth), P(pose), P(K), P(img), B, H, W, 0, 1, P(gd), P(gp), P(ws), ws.t.numel(), stream()) == INVALID
        assert h.mcav_ssim_fwd(P(img), P(img), 3, H, W, 1e-4, 9e-4, P(out), stream()) == INVALID
    for H, W in ((2, 4), (4, 2)):
        acc = Guarded((1,))
        assert h.mcav_smooth_loss_fwd_bwd(P(depth), B, H, W, 1.0, None, P(acc), P(gd), 0, P(ws), ws.t.numel(), stream()) == INVALID
        assert acc.untouched()
    torch.cuda.synchronize()
    for g in (out, gd, gp, grid):
        assert g.untouched()
    assert int(ws.t.max()) == 0


# ---------------------------------------------------------------------------------------------- inverse warp
def warp_inputs(c):
    return [c[k].to(DEV).contiguous() for k in ("img", "depth", "pose")]


def warp_fwd(h, c, inv, f64=1):
    B, _, H, W = c["img"].shape
    K, flag = k_arg(c["K"], f64)
    out, ws = Guarded((B, 3, H, W)), workspace(h, B, H, W)
    img, depth, pose = warp_inputs(c)
    assert h.mcav_inverse_warp_fwd(P(img), P(depth), P(pose), P(K), B, H, W, inv, flag, P(out), P(ws), ws.t.numel(), stream()) == 0
    return done(out, ws)[0]


def warp_bwd(h, c, inv, f64=1):
    B, _, H, W = c["img"].shape
    K, flag = k_arg(c["K"], f64)
    gd, gp, ws = Guarded((B, H, W)), Guarded((B, 6)), workspace(h, B, H, W)
    img, depth, pose = warp_inputs(c)
    go = c["grad_out"].to(DEV).contiguous()
    assert h.mcav_inverse_warp_bwd(P(img), P(depth), P(pose), P(K), P(go), B, H, W, inv, flag, P(gd), P(gp), P(ws), ws.t.numel(), stream()) == 0
    return done(gd, gp, ws)[:2]


def warp_refs(c, inv, backward):
    """-> [(float32 CPU oracle, float64 definition, [float64 on inputs perturbed by 1e-6] x 2)] per output tensor"""
    def run(fn, dtype, e=None):
        pt = (lambda t, k: t.to(dtype)) if e is None else (lambda t, k: perturb_tensor(t.to(F64), 1e-6, 1000 * (e + 1) + k))
        img, go = pt(c["img"], 0), pt(c["grad_out"], 3)
        D, p = pt(c["depth"], 1).clone().requires_grad_(), pt(c["pose"], 2).clone().requires_grad_()
        out = fn(img, D, p, c["K"], inv)
        if not backward:
            return [out.detach()]
        (out * go).sum().backward()
        return [D.grad, p.grad]
    r32, r64 = run(og.inverse_warp, torch.float32), run(R.inverse_warp, F64)
    envs = [run(R.inverse_warp, F64, e) for e in range(2)]
    return [(r32[i], r64[i], [e[i] for e in envs]) for i in range(len(r64))]


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("kind", C.POSE_KINDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_inverse_warp_fwd(h, shape, kind, inv):
    """The arbiter rule, and per element |err| <= spread * delta + 8 u max|texel| (warp_ops_ref.inverse_warp_bound; delta recorded per case
    in warp_ops_cases.DELTAS).  A translation that takes every pixel out of view gives exactly zero."""
    c = C.warp_case(*shape, kind)
    out = warp_fwd(h, c, inv)
    if kind == "away":
        assert bool((out == 0).all())
        return
    (r32, r64, envs), = warp_refs(c, inv, False)
    name = "inverse_warp_fwd %s %s inv %d" % (shape, kind, inv)
    v = Verdicts(factor=2.0, floor=2e-6)
    v.add(name, out, r32, r64, envs)
    v.check(name)
    within(name, out, r64, R.inverse_warp_bound(c["img"], c["depth"], c["pose"], c["K"], inv, C.DELTAS[(shape, kind, inv)]))


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("kind", C.POSE_KINDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_inverse_warp_bwd(h, shape, kind, inv):
    """d_depth and d_pose by the arbiter rule; (1, 16, 32) and (1, 24, 32) give the finalize kernel 2 and 3 workgroups' partial sums for its
    four strided parts, (3, 17, 70) gives it 9."""
    c = C.warp_case(*shape, kind)
    gd, gp = warp_bwd(h, c, inv)
    if kind == "away":
        assert bool((gd == 0).all()) and bool((gp == 0).all())
        return
    refs = warp_refs(c, inv, True)
    name = "inverse_warp_bwd %s %s inv %d" % (shape, kind, inv)
    v = Verdicts(factor=2.0, floor=2e-6)
    for n, got, (r32, r64, envs) in zip(("d_depth", "d_pose"), (gd, gp), refs):
        v.add(name + " " + n, got, r32, r64, envs)
    v.check(name)


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("angle", [1e-8, 1e-4, 1.0, math.pi - 1e-3])
def test_inverse_warp_at_the_pose_angles(h, angle, inv):
    """Forward and backward at rotations from 1e-8 rad to almost a half turn (most pixels leave the view at the large ones), K as float32."""
    B, H, W = 3, 17, 70
    c = C.warp_case(B, H, W, "zero")
    c["pose"] = C.pose_vectors(B, angle, 21)
    c["pose"][:, 3:] *= 0.1
    c["K"] = c["K"].float()
    out, (gd, gp) = warp_fwd(h, c, inv, f64=0), warp_bwd(h, c, inv, f64=0)
    name = "inverse_warp angle %g inv %d" % (angle, inv)
    v = Verdicts(factor=2.0, floor=2e-6)
    v.add(name + " out", out, *warp_refs(c, inv, False)[0])
    for n, got, ref in zip(("d_depth", "d_pose"), (gd, gp), warp_refs(c, inv, True)):
        v.add(name + " " + n, got, *ref)
    v.check(name)


# ---------------------------------------------------------------------------------------------- SSIM
def ssim_run(h, x, y):
    N, H, W = x.shape
    out = Guarded((N, H, W))
    assert h.mcav_ssim_fwd(P(x.to(DEV)), P(y.to(DEV)), N, H, W, 1e-4, 9e-4, P(out), stream()) == 0
    return done(out)[0]


@pytest.mark.parametrize("kind", ["random", "same", "constant", "conditioned"])
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_ssim(h, shape, kind):
    """x == y gives exactly 0; otherwise the arbiter rule against the float32 avg_pool2d formulation (E[x^2] - mu^2 cancels in any float32
    evaluation); the well-conditioned case (window variances >= 0.01) also per element within warp_ops_ref.ssim_bound."""
    B, H, W = shape
    x, y = C.ssim_case(3 * B, H, W, kind)
    out = ssim_run(h, x, y)
    name = "ssim %s %s" % (shape, kind)
    assert bool(((out >= 0) & (out <= 1)).all())
    if kind == "same":
        assert bool((out == 0).all())
        return
    want = R.ssim(x, y)
    v = Verdicts(factor=2.0, floor=2e-6)
    v.add(name, out, ol.ssim_distance(x[None], y[None])[0], want,
          [R.ssim(perturb_tensor(x.to(F64), 1e-6, 10 + e), perturb_tensor(y.to(F64), 1e-6, 20 + e)) for e in range(2)])
    v.check(name)
    if kind == "conditioned" and H >= 3 and W >= 3:
        within(name, out, want, R.ssim_bound(x, y))


# ---------------------------------------------------------------------------------------------- smoothness
def smooth_run(h, D, weight=1.0, upstream=None, start=0.0, prefill=None):
    B, _, H, W = D.shape
    n = h.mcav_smooth_workspace_bytes(B, H, W)
    ws = Guarded((n,), torch.uint8, init=0, band=256)
    acc, gd = Guarded((1,), init=start), Guarded((B, 1, H, W), init=prefill)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
    assert h.mcav_smooth_loss_fwd_bwd(P(D.to(DEV)), B, H, W, weight, None if up is None else P(up), P(acc), P(gd), 0 if prefill is None else 1,
                                      P(ws), n, stream()) == 0
    loss, grad, _ = done(acc, gd, ws)
    return float(loss), grad


SMOOTH_VARIANTS = ["plain", "weight", "upstream", "accumulate", "loss_start", "constant"]


def smooth_case(h, shape, variant):
    """-> (loss, gradient, float64 loss with the start, float64 gradient with the prefill, weight, upstream, |prefilled total| or None)"""
    B, H, W = shape
    D = C.dyadic_depth(B, H, W, constant=(variant == "constant"))
    weight = 0.37 if variant == "weight" else 1.0
    upstream = 1.7 if variant == "upstream" else None
    start = 2.5 if variant == "loss_start" else 0.0
    prefill = None
    if variant == "accumulate":
        prefill = (torch.randint(-64, 64, (B, 1, H, W), generator=C.gen(3)).float() / 64).to(DEV)
    loss, grad = smooth_run(h, D, weight, upstream, start, prefill)
    want_loss, want_grad = R.smooth(D, weight, 1.0 if upstream is None else upstream)
    if prefill is not None:
        want_grad = want_grad + prefill.cpu().to(F64)
    return D, loss, grad, want_loss + start, want_grad, weight, (1.0 if upstream is None else upstream), prefill is not None


@pytest.mark.parametrize("variant", [v for v in SMOOTH_VARIANTS if v != "constant"])
@pytest.mark.parametrize("shape", C.SMOOTH_SHAPES, ids=ids)
def test_smooth_gradient_within_8u_of_the_largest_coefficient(h, shape, variant):
    """The gradient held to 8 u of the largest coefficient a sign carries (warp_ops_ref.smooth_coefficient), plus one rounding of the sum
    where it accumulates onto a prefilled gradient.  A pixel's gradient is a sum of TEN signed coefficients, 4 cxx + 4 cyy + 4 cxy = 7 to 8
    times the largest in magnitude.  Summed in float32, as the kernel first did, the rounding of weight / (float)n and of the nine
    additions missed this in 11 of 30 cases (measured on MI355X, worst |err| in units of u times that coefficient: (1, 3, 40) and
    (1, 40, 3) weight 9.8; (2, 8, 32) plain 15.1, upstream 13.6; (2, 9, 33) weight 13.8; (1, 17, 70) plain 17.4, upstream 18.9).  The
    kernel now sums each group's signs as integers, weights them in float64 and rounds once: u of at most 8 coefficients."""
    B, H, W = shape
    D, loss, grad, want_loss, want_grad, weight, upstream, prefilled = smooth_case(h, shape, variant)
    bound = 8 * U * R.smooth_coefficient(B, H, W, weight, upstream)
    within("smooth %s %s gradient (8 u of the largest coefficient)" % (shape, variant), grad, want_grad,
           bound + U * want_grad.abs() if prefilled else bound)


@pytest.mark.parametrize("variant", SMOOTH_VARIANTS)
@pytest.mark.parametrize("shape", C.SMOOTH_SHAPES, ids=ids)
def test_smooth_loss(h, shape, variant):
    """Depths on a dyadic grid: every second difference is exact in float32 and every sign is float64's, exact zeros included, so the
    gradient differs from float64 by the rounding of its ten-term sum alone: 11 u (4 cxx + 4 cyy + 4 cxy) (and one rounding of the sum
    where it accumulates onto a prefilled gradient); the loss to 16 u (a product and two additions per pixel, eight levels of the
    workgroup's tree, the conversion, the add into loss_accum).  A constant depth gives exactly zero."""
    B, H, W = shape
    D, loss, grad, want_loss, want_grad, weight, upstream, prefilled = smooth_case(h, shape, variant)
    name = "smooth %s %s" % (shape, variant)
    if variant == "constant":
        assert loss == 0.0 and bool((grad == 0).all())
        return
    bound = R.smooth_gradient_bound(B, H, W, weight, upstream)
    within(name + " gradient", grad, want_grad, bound + U * want_grad.abs() if prefilled else bound)
    print("%s loss %.9g float64 %.9g" % (name, loss, want_loss))
    assert abs(loss - want_loss) <= 16 * U * want_loss
    if variant == "upstream":
        again, g1 = smooth_run(h, D, weight, None)
        assert again == loss                                               # upstream scales the gradient only
        assert float((g1.to(F64) * float(np.float32(1.7)) - grad.to(F64)).abs().max()) <= 2 * U * float(grad.abs().max())


# ---------------------------------------------------------------------------------------------- disparity -> depth
def test_disp_to_depth_and_backward_past_one_grid_stride(h):
    """n = 4096 * 256 + 3: the grid-stride loop takes a second trip.  8 ulp relative: at most five roundings on positive operands."""
    n = C.DISP_N
    g = C.gen(1)
    disp, dD = torch.rand(n, generator=g), torch.randn(n, generator=g)
    out, back = Guarded((n,)), Guarded((n,))
    assert h.mcav_disp_to_depth(P(disp.to(DEV)), P(out), n, stream()) == 0
    assert h.mcav_disp_to_depth_bwd(P(disp.to(DEV)), P(dD.to(DEV)), P(back), n, stream()) == 0
    depth, dd = done(out, back)
    a, b = R.ulps(depth, R.disp_to_depth(disp)), R.ulps(dd, R.disp_to_depth_bwd(disp, dD))
    print("disp_to_depth: %.2f ulp, backward %.2f ulp" % (a, b))
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(dd).all())
    assert a <= 8 and b <= 8


# ---------------------------------------------------------------------------------------------- the Python wrappers
@pytest.mark.parametrize("kdtype", [torch.float32, torch.float64])
def test_wrappers_take_non_contiguous_inputs(h, kdtype):
    """A channel-sliced [B,1,H,W] depth, a transposed-then-restored image view, K as float32 and as float64: the drop-in modules give the bits
    the C ABI gives on contiguous copies."""
    from geometry.pose_geometry import inverse_warp
    from geometry.transform import Transform
    from losses import SSIM
    from mcav.multiscale import smooth_loss
    B, H, W = 3, 17, 70
    c = C.warp_case(B, H, W, "small")
    K = c["K"].to(kdtype)
    c["K"] = K
    two = torch.stack([c["depth"], c["depth"] + 1], 1).to(DEV).requires_grad_()      # [B,2,H,W]
    depth = two[:, :1]                                                     # channel-sliced, not contiguous
    img = c["img"].permute(0, 1, 3, 2).contiguous().to(DEV).permute(0, 1, 3, 2)      # transposed, then restored as a view
    assert not depth.is_contiguous() and not img.is_contiguous()
    f64 = 1 if kdtype == F64 else 0
    p = c["pose"].to(DEV).requires_grad_()
    out = inverse_warp(img, depth, p, K.to(DEV), False)
    assert torch.equal(out.detach().cpu(), warp_fwd(h, c, 0, f64))
    go = c["grad_out"].to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    out.backward(go)
    gd, gp = warp_bwd(h, c, 0, f64)
    assert torch.equal(two.grad[:, 0].cpu(), gd) and torch.equal(p.grad.cpu(), gp) and float(two.grad[:, 1].abs().max()) == 0.0
    depth = depth.detach()
    X = Transform().reconstruct(depth, K.to(DEV))
    ws, o = workspace(h, B, H, W), Guarded((B, 3, H, W))
    assert h.mcav_reconstruct(P(c["depth"].to(DEV)), P(K.to(DEV)), B, H, W, f64, P(o), P(ws), ws.t.numel(), stream()) == 0
    assert torch.equal(X.cpu(), done(o)[0])
    Tcw = R.pose_to_matrix(c["pose"]).float().to(DEV)
    grid = Transform().project(X.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), K.to(DEV), Tcw)
    o = Guarded((B, H, W, 2))
    assert h.mcav_project(P(X.contiguous()), P(K.to(DEV)), P(Tcw), B, H, W, f64, P(o), stream()) == 0
    assert torch.equal(grid.cpu(), done(o)[0])
    x, y = C.ssim_case(3 * B, H, W, "random")
    xv = x.view(B, 3, H, W).permute(0, 1, 3, 2).contiguous().to(DEV).permute(0, 1, 3, 2)
    assert torch.equal(SSIM().standard_loss(xv, y.view(B, 3, H, W).to(DEV)).cpu().view(3 * B, H, W), ssim_run(h, x, y))
    D = C.dyadic_depth(B, H, W)
    Dv = torch.stack([D[:, 0], D[:, 0]], 1).to(DEV)[:, 1:].requires_grad_()
    loss = smooth_loss(Dv)
    want_loss, want_grad = smooth_run(h, D)
    assert float(loss) == want_loss
    (g,) = torch.autograd.grad(loss, Dv)
    assert torch.equal(g.cpu(), want_grad)
