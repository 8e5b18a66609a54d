"""GPU: the fused L1 loss kernels (csrc/warp_loss_l1_body.h) where a workgroup WALKS tiles -- several tiles per workgroup, staged gradients
flushed mid-walk, workgroups of one pass with different tile counts, one workgroup per pass, the ticket capacity -- through the C ABI on
guarded windows.

The method keeps the CPU side tiny.  Samples are independent, so a launch batch of B = S k samples (k a power of two) whose sample b is a
copy of distinct sample b % S computes, per pixel, exactly 1 / k of what the B = S launch computes: every factor that depends on the launch
geometry (invN, cxx, cyy, cxy) is a reciprocal of B times a constant, 1 / (float)(k n) == (1 / (float)n) / k exactly, and a pixel's gradient
is formed by one thread from its sample's data alone.  The B = S launch runs one tile per workgroup, the regime the existing tests pin to
float64, and is pinned to the float64 restatement here as well (tests/minreproj_ref.py, tests/stereo_ref.py), so the chain ends at float64
inside this module.  The query mcav_warp_loss_l1_grid tells which B puts the kernels into which regime on the device at hand; each test
prints B, G0, G1 and the tiles per workgroup it ran (pytest -s).

Pose gradients and loss scalars of the two launches are the same fp32 sums in another order: held to 2e-6 of the largest entry, the bar
tests/test_loss_gpu.py holds two orderings of these sums to (measured on MI355X over all cases: d_poses 2.4e-7 at most, the loss scalars
1.2e-7; the per-pixel gradients and selections are bit-identical everywhere)."""
import ctypes
import functools

import pytest
import torch

import minreproj_ref as MR
import stereo_ref as SR
from arbiter import Verdicts, perturb_tensor
from guarded import Guarded
from test_minreproj_gpu import check_selection, network_like

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 4
UP = (0.7, 1.3)
MODES = {"plain": {}, "min": dict(min_reprojection=True), "auto": dict(automask=True), "both": dict(min_reprojection=True, automask=True)}
BITS = {"plain": 0, "min": 32, "auto": 64, "both": 96}
INSTS = [(m, st) for st in (0, 1) for m in MODES]
INST_IDS = ["%s-%s" % (m, "stereo" if st else "mono") for m, st in INSTS]
EXTRAS = {"": 0, "depth": 8, "nosmooth": 4}           # MCAV_WL_INPUT_DEPTH, MCAV_WL_NO_SMOOTH
K_F64 = 1
WALK_SHAPE = (72, 130)                                # 5 x 5 tiles: the last tile row holds its upper half only, the last column 2 pixels
RAGGED_SHAPES = [(72, 130), (104, 70), (200, 40)]
BATCHES = [4 << m for m in range(10)]                 # 4 .. 2048
# The arbiter's envelope here: float64 on images perturbed by 1e-6 (as everywhere) and on disparities and poses perturbed by 1e-5.
# At 37 k pixels ONE bilinear cell or L1 sign decided the other way moves the pose gradient by 1.5e-3 .. 7e-3 of its norm (and d disp_t without
# the smoothness term by 7e-3), and which pixels an fp32 evaluation decides the other way is set by the error of its sampling positions:
# up to 5e-5 .. 1e-4 px (tests/flip_finder.py's cell margin, tests/test_minreproj_gpu.py's check_selection).  A relative perturbation r of
# disparity and pose moves a position by r times the parallax, 4 px here (fx t / D = 75 * 0.01 / 0.2): r = 1e-6 gives 4e-6 px and reaches a
# pixel in one draw of six (measured on the CPU, 72 x 130 plain: 2e-6, 1.5e-3, 2e-6, 3e-6, 2e-6, 3e-6), r = 1e-5 gives the fp32 evaluations' own
# 4e-5 px and a steady 3e-3 .. 7e-3.  The host build of the kernel's arithmetic (flip_finder.host_taps) on these inputs: 3.2e-3 from float64,
# two pixels decided differently, float64 margins 8e-6 px and 6e-6; 3.6e-6 with float64 taking their side.  The plain kernel on MI355X:
# 3.6e-3, four pixels, 3.3e-6 with float64 taking their side; test_plain_kernel_differs_from_float64_at_named_ties_only holds it to that.
# Measured |HIP - float64| of d_poses at 4 x 72x130 over the eight instantiations: 2.6e-3 .. 9.3e-3, 0.5 .. 0.8 of this envelope.
GEOMETRY_NOISE = 1e-5


def distinct_samples(B, H, W, seed):
    """network_like's inputs with a different K per sample and a stereo frame and baseline (test_stereo_gpu.stereo_inputs')."""
    tgt, refs, dt, dr, poses, K = network_like(B, H, W, seed)
    i = (torch.arange(B) % 7).double()
    K = K.clone()
    K[:, 0, 0] *= 1 + 0.03 * i
    K[:, 1, 1] *= 1 - 0.02 * i
    K[:, 0, 2] += 0.7 * i
    K[:, 1, 2] -= 0.4 * i
    g = torch.Generator().manual_seed(seed + 2)
    st = (0.9 * torch.roll(tgt, 1, dims=3) + 0.1 * torch.rand(tgt.shape, generator=g)).contiguous()
    b = (0.54 * torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0) * (0.9 + 0.2 * torch.rand(B, generator=g))).float()
    return dict(tgt=tgt, ref0=refs[0], ref1=refs[1], dt=dt, dr=dr, poses=poses, K=K, st=st, b=b)


@functools.lru_cache(maxsize=None)
def samples(H, W, extra="", B=S):
    d = distinct_samples(B, H, W, 7 * H + W)
    if extra == "depth":
        d["dt"], d["dr"] = (1.0 / (10.0 * d[k] + 0.01) for k in ("dt", "dr"))
    return d


@functools.lru_cache(maxsize=None)
def reference(H, W, mode, stereo, extra="", B=S):
    """The float64 restatement on the distinct samples, the same in float32, and float64 on inputs perturbed by 1e-6 (the envelope).
    MCAV_WL_NO_SMOOTH: the smoothness term has no gradient and its loss scalar is 0."""
    d = samples(H, W, extra, B)
    m = dict(MODES[mode], inputs_are_depth=(extra == "depth"))
    up = (UP[0], 0.0 if extra == "nosmooth" else UP[1])

    def run(dtype, e=None):
        pt = (lambda t, k, r=0: t) if e is None else (lambda t, k, r=1e-6: perturb_tensor(t.double(), r, 1000 * (e + 1) + k))
        a = (pt(d["tgt"], 3), [pt(d["ref0"], 4), pt(d["ref1"], 5)])
        z = (pt(d["dt"], 0, GEOMETRY_NOISE), pt(d["dr"], 1, GEOMETRY_NOISE), pt(d["poses"], 2, GEOMETRY_NOISE), d["K"])
        if stereo:
            return SR.run(*a, pt(d["st"], 6), d["b"], *z, dtype, upstream=up, **m)
        return MR.run(*a, *z, dtype, upstream=up, **m)
    r64, r32 = run(torch.float64), run(torch.float32)
    envs = [run(torch.float64, e)[1] for e in range(2 if B > 64 else 6)]
    return r64, r32, envs


def grid_of(h, B, H, W, mode, stereo):
    g0, g1 = ctypes.c_int(0), ctypes.c_int(0)
    assert h.mcav_warp_loss_l1_grid(B, H, W, K_F64 | BITS[mode], stereo, 0, ctypes.byref(g0), ctypes.byref(g1)) == 0
    return g0.value, g1.value


def ntiles_of(H, W):
    return ((W + 31) // 32) * ((H + 15) // 16)


def describe(tag, B, H, W, g0, g1):
    n = ntiles_of(H, W)
    per = lambda G: "%d" % (n // G) if n % G == 0 else "%d / %d" % (-(-n // G), n // G)
    return "%-34s B %4d  %3d x %3d (%2d tiles)  G0 %2d  G1 %2d  tiles per workgroup: pass 0 %s, pass 1 %s" % (tag, B, H, W, n, g0, g1, per(g0), per(g1))


class Launch:
    """One call of the entry of (mode, stereo) on B = S k samples, sample b a copy of distinct sample b % S.  Every output is a guarded window
    that starts as sentinels; the zero-filled workspace is a guarded window of exactly the queried size unless one is passed in."""

    def __init__(self, h, d, k, mode, stereo, extra="", upstream=UP, ws=None, B=None):
        from mcav import lib as L
        n = d["tgt"].shape[0]
        self.B = B = n * k if B is None else B
        H, W = d["tgt"].shape[-2:]
        rep = lambda t: t.to(DEV).repeat(k, *([1] * (t.dim() - 1))).contiguous()
        self.inp = {key: rep(t) for key, t in d.items()}
        self.losses, self.d_dt, self.d_dr = Guarded((2,)), Guarded((B, 1, H, W)), Guarded((B, 1, H, W))
        self.d_p, self.sel = Guarded((B, 2, 6)), Guarded((B, 2, H, W), torch.uint8)
        self.ws = ws if ws is not None else Guarded((h.mcav_warp_loss_workspace_bytes(B, H, W),), torch.uint8, init=0, band=256)
        self.up = torch.tensor(upstream, dtype=torch.float32, device=DEV) if upstream is not None else None
        i = self.inp
        args = [L.ptr(i[key]) for key in ("tgt", "ref0", "ref1", "dt", "dr", "poses", "K")] + [
            B, H, W, K_F64 | BITS[mode] | EXTRAS[extra], L.ptr(self.up), None,
            *[L.ptr(g.t) for g in (self.losses, self.d_dt, self.d_dr, self.d_p)], L.ptr(self.ws.t), self.ws.t.numel(), L.stream(),
            L.ptr(self.sel.t), self.sel.t.numel()]
        if stereo:
            self.rc = h.mcav_warp_loss_stereo_fwd_bwd(*args, L.ptr(i["st"]), L.ptr(i["b"]))
        else:
            self.rc = h.mcav_warp_loss_masked_fwd_bwd(*args)
        torch.cuda.synchronize()
        self.outputs = (self.losses, self.d_dt, self.d_dr, self.d_p, self.sel)

    def ok(self):
        assert self.rc == 0, self.rc
        for g in self.outputs + (self.ws,):
            assert g.intact(), "a store outside a window of shape %s" % (tuple(g.t.shape),)
        for g in self.outputs[:4]:
            assert bool(torch.isfinite(g.t).all()), "an element of a window of shape %s was not written" % (tuple(g.t.shape),)
        assert int(self.sel.t.max()) <= 3, "a selection code was not written"
        return self


def check_against_float64(tag, base, H, W, mode, stereo, extra="", B=S):
    """The B = S launch (one tile per workgroup) against the float64 restatement: arbiter rule for the gradients (factor 2, floor 2e-6),
    1e-5 relative for the loss scalars, the selection planes equal to float64's except at ties."""
    (l64, g64, s64, gap64), (_, g32, s32, _), envs = reference(H, W, mode, stereo, extra, B)
    got = base.losses.cpu().tolist()
    print("%s losses %s float64 %s" % (tag, got, l64))
    assert abs(got[0] - l64[0]) <= 1e-5 * abs(l64[0]), (got, l64)
    if extra == "nosmooth":
        assert got[1] == 0.0
    else:
        assert abs(got[1] - l64[1]) <= 1e-5 * abs(l64[1]), (got, l64)
    check_selection(tag, [base.sel.cpu()], s64, gap64, s32)
    v = Verdicts(factor=2.0, floor=2e-6)
    for i, (n, g) in enumerate((("d disp_t", base.d_dt), ("d disp_r", base.d_dr), ("d poses", base.d_p))):
        v.add("%s %s" % (tag, n), g.cpu(), g32[i], g64[i], [env[i] for env in envs])
    v.check(tag)


def check_walk(tag, big, base, k):
    """The launch on S k samples against the launch on the S distinct ones."""
    split = lambda g: g.t.view(k, S, *g.t.shape[1:])
    # 1. every copy agrees with the first copy of its sample, bit for bit
    for n, g in (("d_disp_t", big.d_dt), ("d_disp_r0", big.d_dr), ("d_poses", big.d_p), ("selection", big.sel)):
        v = split(g)
        assert torch.equal(v, v[:1].expand_as(v)), "%s: %s differs between copies of one sample" % (tag, n)
    # 2. the walk does not change a pixel's result (no denormal in play: the scaling by k is exact)
    for n, g, b in (("d_disp_t", big.d_dt, base.d_dt), ("d_disp_r0", big.d_dr, base.d_dr)):
        v = split(g)[0]
        mag = v.abs()
        assert float(mag[mag > 0].min()) > 2.0 ** -100, "%s: %s holds a gradient below 2^-100" % (tag, n)
        same = (v * float(k)) == b.t
        assert bool(same.all()), "%s: k * %s differs from the one-tile-per-workgroup launch at %d of %d pixels, first %s" % (
            tag, n, int((~same).sum()), same.numel(), (~same).nonzero()[:4].tolist())
    assert torch.equal(split(big.sel)[0], base.sel.t), "%s: the selection differs from the one-tile-per-workgroup launch" % tag
    # 3. the same fp32 sums in another order
    p, q = split(big.d_p)[0].double().cpu() * k, base.d_p.cpu().double()
    gap = float((p - q).abs().max() / q.abs().max())
    la, lb = big.losses.cpu().double(), base.losses.cpu().double()
    lgap = [float(abs(x - y) / abs(y)) if float(y) != 0.0 else float(abs(x)) for x, y in zip(la, lb)]
    print("%s reorder gaps: k d_poses %.2e of the largest entry, losses %.2e %.2e" % (tag, gap, lgap[0], lgap[1]))
    assert gap <= 2e-6, gap
    assert max(lgap) <= 2e-6, lgap


def base_launch(h, H, W, mode, stereo, extra=""):
    tag = "%dx%d %s %s %s B = %d" % (H, W, mode, "stereo" if stereo else "mono", extra, S)
    base = Launch(h, samples(H, W, extra), 1, mode, stereo, extra).ok()
    check_against_float64(tag, base, H, W, mode, stereo, extra)
    return base


@pytest.fixture(scope="module")
def h():
    from mcav import lib as L
    return L.lib()


def one_workgroup_batch(h, mode, stereo):
    H, W = WALK_SHAPE
    table = [(B,) + grid_of(h, B, H, W, mode, stereo) for B in BATCHES]
    found = [B for B, g0, g1 in table if g0 == 1 and g1 == 1]
    assert found, "no B <= 2048 gives G0 == G1 == 1 at %dx%d: %s" % (H, W, table)
    return found[0]


CASES = [(m, st, "") for m, st in INSTS] + [(m, st, e) for e in ("depth", "nosmooth") for st in (0, 1) for m in ("plain", "both")]
CASE_IDS = ["%s-%s%s" % (m, "stereo" if st else "mono", "-" + e if e else "") for m, st, e in CASES]


@pytest.mark.parametrize("mode,stereo,extra", CASES, ids=CASE_IDS)
def test_all_tiles_in_one_workgroup_per_pass(h, mode, stereo, extra):
    """G0 = G1 = 1 (more samples than resident slots: the per_sample = 1 branch of the planner): one workgroup walks all 25 tiles of
    72 x 130, 50 pixels per thread = three full flushes of the staged gradients and a tail of 2."""
    H, W = WALK_SHAPE
    B = one_workgroup_batch(h, mode, stereo)
    tag = "one workgroup %s %s %s" % (mode, "stereo" if stereo else "mono", extra)
    print(describe(tag, B, H, W, 1, 1))
    base = base_launch(h, H, W, mode, stereo, extra)
    big = Launch(h, samples(H, W, extra), B // S, mode, stereo, extra).ok()
    check_walk(tag, big, base, B // S)


def ragged_case(h, mode, stereo):
    table = []
    for H, W in RAGGED_SHAPES:
        n = ntiles_of(H, W)
        for B in BATCHES:
            g0, g1 = grid_of(h, B, H, W, mode, stereo)
            table.append((B * H * W, B, H, W, g0, g1, g0 >= 2 and n % g0 != 0 and -(-n // g0) >= 9))
    found = sorted(r for r in table if r[-1])
    assert found, "no launch with G0 >= 2, ntiles %% G0 != 0 and a pass-0 walk of 9 tiles:\n%s" % "\n".join(
        describe("", B, H, W, g0, g1) for _, B, H, W, g0, g1, _ in table)
    return found[0][1:6]


@pytest.mark.parametrize("mode,stereo", INSTS, ids=INST_IDS)
def test_workgroups_of_one_pass_walk_different_tile_counts(h, mode, stereo):
    """G0 >= 2 with ntiles % G0 != 0 and at least 9 tiles (18 pixels per thread: past the first flush) for some pass-0 workgroup."""
    B, H, W, g0, g1 = ragged_case(h, mode, stereo)
    tag = "ragged %s %s" % (mode, "stereo" if stereo else "mono")
    print(describe(tag, B, H, W, g0, g1))
    base = base_launch(h, H, W, mode, stereo)
    big = Launch(h, samples(H, W), B // S, mode, stereo).ok()
    check_walk(tag, big, base, B // S)


def test_plain_kernel_differs_from_float64_at_named_ties_only(h):
    """The B = S launch of the plain kernel, upstream (1, 1), and its per-pixel-dump instantiation (flip_finder.hip_taps: the same sums in
    other code) on the same inputs: d_poses within 2e-6 of the largest entry (measured on MI355X: 2.7e-8).  The dump against float64 names
    every pixel decided differently; each must be a tie (sampling position within 5e-5 px of a cell edge, or a residual below 1e-5), and
    with float64 taking the kernel's side at exactly those pixels the pose gradient agrees to 2e-5, tests/test_loss_gpu.py's bar."""
    import flip_finder as ff
    H, W = WALK_SHAPE
    d = samples(H, W)
    base = Launch(h, d, 1, "plain", 0, upstream=None).ok()
    t = {k: v.to(DEV) for k, v in d.items()}
    taps, dposes, _ = ff.hip_taps(t["tgt"], [t["ref0"], t["ref1"]], t["dt"], t["dr"], t["poses"], t["K"])
    gap = float((base.d_p.cpu() - dposes).abs().max() / dposes.abs().max())
    print("plain kernel against its diagnostic instantiation at %d x %dx%d: d_poses gap %.2e of the largest entry" % (S, H, W, gap))
    assert gap <= 2e-6, gap
    o64 = ff.oracle_taps(d["tgt"], [d["ref0"], d["ref1"]], d["dt"], d["dr"], d["poses"], d["K"], torch.float64, 0.0)
    flips, before, after, bad = ff.report("%d x %dx%d plain kernel" % (S, H, W), taps, dposes, o64)
    assert not bad, "pixels decided differently from float64 without a tie to explain it: %s" % bad
    assert after < 2e-5, (before, after)


@pytest.mark.parametrize("mode", ["plain", "both"])
def test_ticket_capacity(h, mode):
    """B = 4095 = WL_MAX_B distinct 3 x 3 samples straight against float64: the last ticket word and the last sample's sum over every
    sample's loss.  B = 4096 is refused with every window untouched."""
    B, H, W = 4095, 3, 3
    g0, g1 = grid_of(h, B, H, W, mode, 0)
    print(describe("ticket capacity %s" % mode, B, H, W, g0, g1))
    d = samples(H, W, "", B)
    run = Launch(h, d, 1, mode, 0).ok()
    check_against_float64("%d x 3x3 %s" % (B, mode), run, H, W, mode, 0, "", B)
    over = Launch(h, d, 1, mode, 0, B=4096)
    assert over.rc == -1                                                    # MCAV_E_INVALID
    for g in over.outputs:
        assert g.untouched()
    assert int(over.ws.t.max()) == 0 and over.ws.intact()


def test_one_workspace_serves_different_shapes(h):
    """A 4095 x 3x3 launch, a walking 72 x 130 launch and the first again, back to back on one workspace that is zero-filled once and sized
    for the larger: the ticket region sits at a fixed place, whatever the shape, and every launch leaves it at zero (ws_layout's comment).
    Each result is bit-identical to the same launch on a fresh workspace."""
    mode = "both"
    small = samples(3, 3, "", 4095)
    B, H, W, g0, g1 = ragged_case(h, mode, 0)
    print(describe("shared workspace", B, H, W, g0, g1))
    n = max(h.mcav_warp_loss_workspace_bytes(4095, 3, 3), h.mcav_warp_loss_workspace_bytes(B, H, W))
    ws = Guarded((n,), torch.uint8, init=0, band=256)
    fresh = [Launch(h, small, 1, mode, 0).ok(), Launch(h, samples(H, W), B // S, mode, 0).ok()]
    shared = [Launch(h, small, 1, mode, 0, ws=ws).ok(), Launch(h, samples(H, W), B // S, mode, 0, ws=ws).ok(),
              Launch(h, small, 1, mode, 0, ws=ws).ok()]
    for a, b in zip(shared, fresh + fresh[:1]):
        for x, y in zip(a.outputs, b.outputs):
            assert torch.equal(x.t, y.t)
    assert int(ws.t[:4 * 4096].max()) == 0, "a launch left a ticket behind"
