"""GPU: the depth-pyramid kernels alone (include/mcav_depth.h: mcav_depth_pyramid_fwd / _bwd) against the composition of the existing
entry points they replace and against the float64 definition (tests/pyramid_ref.py)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import pyramid_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3           # stacked batch: a wrong batch stride fails every case

# name -> (H, W, [(h, w) per level], dyadic)
SHAPES = {
    "three_levels": (32, 64, [(16, 32), (8, 16), (4, 8)], True),       # one call; at 4x8 every pixel is a border pixel
    "non_dyadic": (30, 50, [(13, 21)], False),                          # W % 4 != 0: the scalar load / store path as well
    "identity": (32, 64, [(32, 64)], True),                             # h = H
    "wide_ratio": (20, 1200, [(3, 40)], False),                         # two column tiles, four column chunks and two row chunks per tile
}
RANGES = {"unit": (0.0, 1.0), "inner": (0.05, 0.95)}
ORDERS = {"depth": 0, "disparity": 1}


def lib():
    from mcav import lib as L
    from mcav import tape  # noqa: F401  (registers the resize entry points)
    return L, L.lib()


@functools.lru_cache(maxsize=None)
def case(shape, rng):
    """Inputs and float64 references, computed once: ({level: disp}, d_out, {order: per-level (out64, scale, grad64, S, N)})."""
    H, W, levels, _ = SHAPES[shape]
    lo, hi = RANGES[rng]
    g = torch.Generator().manual_seed(17)
    disps = [lo + (hi - lo) * torch.rand(B, h, w, generator=g) for h, w in levels]
    d_out = torch.randn(len(levels), B, H, W, generator=g)
    ref = {}
    for order, rtd in ORDERS.items():
        ref[order] = []
        for l, d in enumerate(disps):
            out64, scale = R.forward64(d, H, W, bool(rtd), fma=True)          # the device's taps: one fused multiply-add, rounded once
            grad64, S, N = R.backward64(d, d_out[l], bool(rtd), fma=True)
            ref[order].append((out64, scale, grad64, S, N))
    return disps, d_out, ref


def pyramid(disps, H, W, flags, d_out=None, out=None):
    """The new entries.  Forward alone, or (given d_out) the backward as well -> (out, [d_disp per level])."""
    L, h = lib()
    n = len(disps)
    if out is None:
        out = torch.full((n, B, H, W), float("nan"), device=DEV)
        lv = (L.PyrLevel * n)(*[L.PyrLevel(d.data_ptr(), 0, d.shape[1], d.shape[2]) for d in disps])
        L.check(h.mcav_depth_pyramid_fwd(lv, n, B, H, W, flags, L.ptr(out), L.stream()), "mcav_depth_pyramid_fwd")
    if d_out is None:
        return out, None
    dd = [torch.full_like(d, float("nan")) for d in disps]
    lv = (L.PyrLevel * n)(*[L.PyrLevel(d.data_ptr(), g.data_ptr(), d.shape[1], d.shape[2]) for d, g in zip(disps, dd)])
    L.check(h.mcav_depth_pyramid_bwd(lv, n, B, H, W, flags, L.ptr(out), L.ptr(d_out), L.stream()), "mcav_depth_pyramid_bwd")
    return out, dd


def composition(d, H, W, rtd, g):
    """One level through the existing entry points in the matching order -> (out, d_disp)."""
    L, lb = lib()
    _, h, w = d.shape
    st = L.stream()
    n_lo, n_hi = d.numel(), B * H * W
    new = lambda *s: torch.empty(s, device=DEV)
    if not rtd:
        D, out, r, dd = new(B, h, w), new(B, H, W), new(B, h, w), new(B, h, w)
        L.check(lb.mcav_disp_to_depth(L.ptr(d), L.ptr(D), n_lo, st), "disp_to_depth")
        L.check(lb.mcav_resize_bilinear_fwd(L.ptr(D), B, h, w, L.ptr(out), H, W, 0.0, 0.0, st), "resize_fwd")
        L.check(lb.mcav_resize_bilinear_bwd(L.ptr(g), B, h, w, L.ptr(r), H, W, 0.0, 0.0, 0, st), "resize_bwd")
        L.check(lb.mcav_disp_to_depth_bwd(L.ptr(d), L.ptr(r), L.ptr(dd), n_lo, st), "disp_to_depth_bwd")
    else:
        u, out, t, dd = new(B, H, W), new(B, H, W), new(B, H, W), new(B, h, w)
        L.check(lb.mcav_resize_bilinear_fwd(L.ptr(d), B, h, w, L.ptr(u), H, W, 0.0, 0.0, st), "resize_fwd")
        L.check(lb.mcav_disp_to_depth(L.ptr(u), L.ptr(out), n_hi, st), "disp_to_depth")
        L.check(lb.mcav_disp_to_depth_bwd(L.ptr(u), L.ptr(g), L.ptr(t), n_hi, st), "disp_to_depth_bwd")
        L.check(lb.mcav_resize_bilinear_bwd(L.ptr(t), B, h, w, L.ptr(dd), H, W, 0.0, 0.0, 0, st), "resize_bwd")
    return out, dd


def worst(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("n_in,n_out", [(13, 30), (21, 50), (3, 20), (40, 1200), (8, 64)])
def test_reference_weights_are_the_devices(n_in, n_out):
    """The float64 references stand on this: tests/pyramid_ref.py's taps with fma=True are the device's bil_src bit for bit.  The existing
    resize of the unit vectors along one row (B = n_in maps of 1 x n_in) returns each weight untouched: x * (1 - lx) + 0 * lx, then * 1."""
    L, lb = lib()
    eye = torch.eye(n_in, device=DEV).reshape(n_in, 1, n_in).contiguous()
    got = torch.empty(n_in, 1, n_out, device=DEV)
    L.check(lb.mcav_resize_bilinear_fwd(L.ptr(eye), n_in, 1, n_in, L.ptr(got), 1, n_out, 0.0, 0.0, L.stream()), "resize_fwd")
    # (float32 on both sides: where both taps clamp onto the last source the device returns (1 - lam) + lam rounded once more)
    assert torch.equal(got[:, 0].T.cpu(), R.axis_matrix(n_in, n_out, fma=True).float())


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("rng", list(RANGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_and_backward(shape, rng, order):
    """Forward: |out - want| <= 1e-6 * (largest of the four contributing depths), against the composition of the existing entry points for
    every shape and against float64 F.interpolate for the dyadic ones (float32 weights alone move a non-dyadic result by more, so those are
    judged against the kernels that share bil_src).  Backward: |got - want| <= (N + 8) 2^-24 S per element -- the worst-case rounding of a
    float32 sum of N terms in any order, S the same adjoint of |d_out| |dD/d.| in float64 -- against the existing composition's backward
    for every shape, against the float64 adjoint with the device's own weights (pyramid_ref's taps with fma=True) for every shape, and against float64 autograd through
    F.interpolate for the dyadic ones."""
    H, W, levels, dyadic = SHAPES[shape]
    disps, d_out, ref = case(shape, rng)
    rtd = ORDERS[order]
    x = [d.to(DEV) for d in disps]
    g = d_out.to(DEV)
    out, dd = pyramid(x, H, W, rtd, g)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t).all()) for t in dd)
    for l, d in enumerate(disps):
        out64, scale, grad64, S, N = ref[order][l]
        c_out, c_dd = composition(x[l], H, W, rtd, g[l])
        f_err = (out[l].cpu().double() - c_out.cpu().double()).abs()
        print("%s %s %s level %d: forward vs composition %.2f of the bound" % (shape, rng, order, l, worst(f_err, 1e-6 * scale)))
        assert bool((f_err <= 1e-6 * scale).all()), worst(f_err, 1e-6 * scale)
        bound = R.backward_bound(S, N)
        b_err = (dd[l].cpu().double() - c_dd.cpu().double()).abs()
        print("    backward vs composition %.2f, vs float64 %.2f of the bound" % (worst(b_err, bound), worst((dd[l].cpu().double() - grad64).abs(), bound)))
        assert bool((b_err <= bound).all()), worst(b_err, bound)
        assert bool(((dd[l].cpu().double() - grad64).abs() <= bound).all())
        if dyadic:
            t = d.double().requires_grad_()
            up = lambda v: F.interpolate(v[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
            want = R.depth_of(up(t)) if rtd else up(R.depth_of(t))
            want.backward(d_out[l].double())
            assert bool(((out[l].cpu().double() - want.detach()).abs() <= 1e-6 * scale).all())
            assert bool(((dd[l].cpu().double() - t.grad).abs() <= bound).all())


@pytest.mark.parametrize("order", list(ORDERS))
def test_two_launches_give_identical_bits(order):
    H, W, _, _ = SHAPES["three_levels"]
    disps, d_out, _ = case("three_levels", "unit")
    x, g = [d.to(DEV) for d in disps], d_out.to(DEV)
    a_out, a_dd = pyramid(x, H, W, ORDERS[order], g)
    b_out, b_dd = pyramid(x, H, W, ORDERS[order], g)
    assert torch.equal(a_out, b_out)
    for a, b in zip(a_dd, b_dd):
        assert torch.equal(a, b)


@pytest.mark.parametrize("order", list(ORDERS))
def test_capture_and_replay_on_new_inputs(order):
    """Both entries under torch.cuda.graph; the replay, after every input buffer was overwritten, equals an eager call on the new inputs."""
    L, h = lib()
    H, W, levels, _ = SHAPES["three_levels"]
    flags = ORDERS[order]
    disps, d_out, _ = case("three_levels", "unit")
    x, g = [d.to(DEV) for d in disps], d_out.to(DEV)
    pyramid(x, H, W, flags, g)                              # (code objects loaded before the capture)
    n = len(x)
    out = torch.zeros((n, B, H, W), device=DEV)
    dd = [torch.zeros_like(d) for d in x]
    lv = (L.PyrLevel * n)(*[L.PyrLevel(d.data_ptr(), q.data_ptr(), d.shape[1], d.shape[2]) for d, q in zip(x, dd)])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(h.mcav_depth_pyramid_fwd(lv, n, B, H, W, flags, L.ptr(out), L.stream()), "mcav_depth_pyramid_fwd")
        L.check(h.mcav_depth_pyramid_bwd(lv, n, B, H, W, flags, L.ptr(out), L.ptr(g), L.stream()), "mcav_depth_pyramid_bwd")
    gen = torch.Generator().manual_seed(23)
    for d in x:
        d.copy_(torch.rand(d.shape, generator=gen))
    g.copy_(torch.randn(g.shape, generator=gen))
    graph.replay()
    torch.cuda.synchronize()
    want_out, want_dd = pyramid(x, H, W, flags, g)
    assert torch.equal(out, want_out)
    for a, b in zip(dd, want_dd):
        assert torch.equal(a, b)


def test_argument_errors():
    L, h = lib()
    H, W = 32, 64
    d = torch.rand(B, 16, 32, device=DEV)
    big = torch.rand(B, 33, 64, device=DEV)
    out = torch.empty(4, B, H, W, device=DEV)
    q = torch.empty_like(d)
    INVALID = -1
    level = lambda t, grad=None, hh=None, ww=None: L.PyrLevel(t.data_ptr() if t is not None else 0, grad.data_ptr() if grad is not None else 0,
                                                              t.shape[1] if hh is None else hh, t.shape[2] if ww is None else ww)
    arr = lambda *ls: (L.PyrLevel * len(ls))(*ls)
    fwd = lambda lv, n, o=out, flags=0: h.mcav_depth_pyramid_fwd(lv, n, B, H, W, flags, L.ptr(o), L.stream())
    bwd = lambda lv, n, o=out, g=out, flags=0: h.mcav_depth_pyramid_bwd(lv, n, B, H, W, flags, L.ptr(o), L.ptr(g), L.stream())
    assert fwd(arr(level(d)), 1) == 0 and bwd(arr(level(d, q)), 1) == 0
    assert fwd(arr(level(big)), 1) == INVALID                               # h > H: downsampling
    assert fwd(arr(level(d, None, 16, 65)), 1) == INVALID                   # w > W
    assert bwd(arr(level(big, torch.empty_like(big))), 1) == INVALID
    four = arr(level(d, q), level(d, q), level(d, q), level(d, q))
    assert fwd(four, 4) == INVALID and bwd(four, 4) == INVALID              # nlevels > 3
    assert fwd(four, 0) == INVALID
    assert fwd(None, 1) == INVALID and bwd(None, 1) == INVALID              # null pointers
    assert fwd(arr(level(d)), 1, None) == INVALID
    assert fwd(arr(L.PyrLevel(0, 0, 16, 32)), 1) == INVALID
    assert bwd(arr(level(d, q)), 1, out, None) == INVALID
    assert bwd(arr(level(d, None)), 1) == INVALID
    assert bwd(arr(level(d, q)), 1, None, out, 1) == INVALID                # resize-then-depth reads the stored depths
    assert fwd(arr(level(d)), 1, out, 2) == INVALID                         # unknown flag bits
    assert h.mcav_depth_pyramid_fwd(arr(level(d)), 1, 0, H, W, 0, L.ptr(out), L.stream()) == INVALID
    torch.cuda.synchronize()
