"""GPU: the voxels' moments (include/mcav_depth.h: mcav_pillar_moments, pseudo_lidar.pillar_moments) against math.fsum of the exact products,
their adjoint (mcav_pillar_moments_bwd, pillar_moments_backward) against float64 numpy, and PillarFeatureLayer(batch_stats=True) stage by
stage -- the fold, the canvas and the features, the buffers, the parameters' gradients, the voxels' gradient, eval() -- on the cases of
tests/pfn_stats_cases.py; every output a window between sentinel bands (tests/guarded.py); repeatability; NaNs wherever the definition does
not read; graph capture and replay on new contents; the C ABI's refusals."""
import numpy as np
import pytest
import torch

import pfn_bwd_ref as BR
import pfn_cases as C
import pfn_ref as R
import pfn_stats_cases as SC
import pfn_stats_ref as SR
from guarded import Guarded, band_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -7.0
EPS = 1e-3


def product_grid(nx, ny, z=(-1.0, 1.0)):
    from pseudo_lidar import PillarGrid
    g = PillarGrid(x=(0.0, float(nx)), y=(0.0, float(ny)), z=z, size=(1.0, 1.0))
    assert (g.nx, g.ny) == (nx, ny)
    return g


def batch(a, fill=SENTINEL, nan_filled=False):
    """the case's pillars on the device in buffers of a["capacity"] rows; behind the pillars `fill` and counts of 1 << 20; nan_filled: NaNs
    in every slot the definition does not read"""
    from pseudo_lidar import PillarBatch
    vox, coords, num = SC.padded(a, fill)
    if nan_filled:
        vox = SC.nan_filled(a)
    pb = PillarBatch(len(a["offsets"]) - 1, a["capacity"], vox.shape[1], vox.shape[2], DEV)
    for t, v in ((pb.voxels, vox), (pb.coords, coords), (pb.num_points, num), (pb.offsets, a["offsets"])):
        t.copy_(torch.from_numpy(np.array(v)))
    pb.grid = product_grid(a["nx"], a["ny"])
    return pb


def moments_window(columns):
    """a float64 [2 + C + C C] window between sentinel bands -> the Guarded, the tensor"""
    g = Guarded((8 * SR.size(columns),), torch.uint8, band=64)
    return g, g.t.view(torch.float64)


def voxels_window(pb):
    g = Guarded(tuple(pb.voxels.shape), band=band_for(tuple(pb.voxels.shape)))
    return g, g.t


# ---------------------------------------------------------------------------------------------- 1. the moments
@pytest.mark.parametrize("name", SC.ALL)
def test_moments_against_fsum(name):
    """|err| <= n 2^-53 sum |terms| (float64 summation of n terms in any order); rows and used exact; M symmetric in its bits; a second run
    and a run with NaNs in every unused slot and behind P give the same bytes"""
    from pseudo_lidar import pillar_moments
    a = SC.build(name)
    Cc = a["voxels"].shape[2]
    runs = []
    for nan in (False, False, True):
        g, out = moments_window(Cc)
        assert pillar_moments(batch(a, nan_filled=nan), out=out) is out
        torch.cuda.synchronize()
        assert g.intact()
        runs.append(out.cpu().numpy())
    SR.check_moments(runs[0], SC.moments(name), name)
    assert runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()
    fresh = pillar_moments(batch(a))                                                       # a tensor of its own
    assert fresh.dtype == torch.float64 and fresh.cpu().numpy().tobytes() == runs[0].tobytes()
    if name == "special-o32":
        assert np.isnan(runs[0][2:]).any() and np.isfinite(runs[0][:2]).all()


# ---------------------------------------------------------------------------------------------- 2. the adjoint
@pytest.mark.parametrize("name", SC.ALL)
def test_moments_backward_against_float64(name):
    """|err| <= 2^-24 |ref| + (C + 1) 2^-53 sum |terms|; +0.0 by bits in unused slots and behind P (the capacity cut among the cases); two
    runs and a run on NaN-filled unused slots give the same bytes"""
    from pseudo_lidar import pillar_moments_backward
    a = SC.build(name)
    grad = torch.from_numpy(SC.gradient(name)).to(DEV)
    runs = []
    for nan in (False, False, True):
        pb = batch(a, nan_filled=nan)
        g, out = voxels_window(pb)
        assert pillar_moments_backward(pb, grad, out=out) is out
        torch.cuda.synchronize()
        assert g.intact()
        runs.append(out.cpu().numpy())
    SR.check_backward(runs[0], SC.backward(name), name)
    assert runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()
    fresh = pillar_moments_backward(batch(a), grad)
    assert fresh.cpu().numpy().tobytes() == runs[0].tobytes()


def test_rows_behind_the_pillars_in_wide_stores():
    """more rows behind the last pillar than pillars, at an odd start: the 16-byte stores and their unaligned ends"""
    from pseudo_lidar import pillar_moments_backward
    a = dict(SC.build("mixed-N5-c9-o64"))
    a["capacity"] = len(a["voxels"]) + 301
    pb = batch(a)
    g, out = voxels_window(pb)
    grad = SC.gradient("mixed-N5-c9-o64")
    pillar_moments_backward(pb, torch.from_numpy(grad).to(DEV), out=out)
    torch.cuda.synchronize()
    assert g.intact()
    SR.check_backward(out.cpu().numpy(), SR.moments_backward(a["voxels"], a["num_points"], a["offsets"], grad[2:11], grad[11:], a["capacity"]), "roomy")


# ---------------------------------------------------------------------------------------------- 3. the layer, stage by stage
def make_layer(columns, c_out, grid, seed):
    from pseudo_lidar import PillarFeatureLayer
    layer = PillarFeatureLayer(columns, c_out, eps=EPS, grid=grid if columns == 10 else None, batch_stats=True)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.linear.weight.copy_(torch.randn(layer.linear.weight.shape, generator=gen) * 0.4)
        layer.norm.weight.copy_(torch.randn(c_out, generator=gen).abs() + 0.5)
        layer.norm.bias.copy_(torch.randn(c_out, generator=gen) * 0.3)
        layer.norm.running_mean.copy_(torch.randn(c_out, generator=gen) * 0.2)
        layer.norm.running_var.copy_(torch.rand(c_out, generator=gen) + 0.1)
    return layer.to(DEV).train()


def within(got, ref, what, rel=2.0 ** -23, slack=2.0 ** -30):
    """one float32 rounding that may fall either way, plus the measured float64 slack"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, bound = np.abs(got - ref), rel * np.abs(ref) + slack * np.abs(ref).max()
    print("    %-18s max err / bound %.3g" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), (what, float((err - bound).max()))


def bits(t):
    return t.detach().cpu().contiguous().numpy()


LAYER_CASES = [("mixed-N5-c9-o64", 9, True), ("over-N64-c4-o64", 4, True), ("pair-N5-c9-o64", 10, True), ("cut-finite", 4, True), ("real-o64", 4, False)]


@pytest.mark.parametrize("name,columns,canvas", LAYER_CASES)
def test_layer_stage_by_stage(name, columns, canvas):
    from pseudo_lidar import PillarFeatureNet, fold_batch, pillar_moments
    a = SC.build(name)
    c_out, cap = a["weight"].shape[0], a["capacity"]
    pb = batch(a, fill=float("nan"))
    pb.grid = product_grid(a["nx"], a["ny"], z=(-3.0, 1.0))                                # zc = -1
    zc = -1.0 if columns == 10 else None
    layer = make_layer(columns, c_out, pb.grid, 60 + columns)
    before = {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}
    P = R.live_pillars(a["offsets"], min(cap, len(a["voxels"])))
    vox, coords, num = a["voxels"][:P], a["coords"][:P], a["num_points"][:P]
    assert np.isfinite(vox).all()

    # (a) the fold: folded(pillars) against fold_batch on the CPU, fed the GPU's moments read back
    moments = pillar_moments(pb).cpu()
    SR.check_moments(moments.numpy(), SC.moments(name), name)
    wf, bf, bp = layer.folded(pb)
    leaves = [before[k].clone().requires_grad_(True) for k in ("linear.weight", "norm.weight", "norm.bias")]
    ref = fold_batch(*leaves, moments, EPS, before["norm.running_mean"], before["norm.running_var"], layer.grid, dtype=torch.float64)
    assert (bp is None) == (ref[2] is None) == (columns != 10) and wf.dtype == bf.dtype == torch.float32
    for got, want, what in ((wf, ref[0], "weight"), (bf, ref[1], "bias")) + (((bp, ref[2], "bias_pad"),) if bp is not None else ()):
        within(bits(got), want.detach().numpy(), what)

    # (c) the buffers after this one step against float64 BatchNorm1d on the stock formulation
    w64, g64, b64 = (before[k].double() for k in ("linear.weight", "norm.weight", "norm.bias"))
    stock = SR.stock(torch.from_numpy(vox.astype(np.float64)), num, w64, g64, b64, EPS, before["norm.running_mean"].double(),
                     before["norm.running_var"].double(), 0.1, zc)
    assert int(layer.norm.num_batches_tracked) == 1
    within(bits(layer.norm.running_mean), stock["norm"].running_mean.numpy(), "running_mean", slack=0.0)
    within(bits(layer.norm.running_var), stock["norm"].running_var.numpy(), "running_var", slack=0.0)
    assert not torch.equal(layer.norm.running_mean.cpu(), before["norm.running_mean"])

    # (b) forward and features are pfn_ref's under the GPU's own folded layer, bit for bit
    wn, bn = bits(wf), bits(bf)
    bpn = bn if bp is None else bits(bp)
    want = R.pseudo_image(a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], wn, bn, bias_pad=bpn, capacity=cap)
    with torch.no_grad():
        C.same_bits(bits(layer.features(pb))[:P], want["features"])
        if canvas:
            for layout in ("nchw", "nhwc"):
                C.same_bits(bits(layer(pb, layout=layout)), want["canvas"])
    assert int(layer.norm.num_batches_tracked) == (4 if canvas else 2)                    # a step a call

    # (d), (e) the gradients: the canvas (or the feature rows) gets an upstream gradient
    rng = np.random.RandomState(70 + len(name))
    shape = want["canvas"].shape if canvas else (cap, c_out)
    up = rng.standard_normal(shape).astype(F)
    up_t = torch.from_numpy(up).to(DEV)
    pb.voxels.requires_grad_(True)
    m = pillar_moments(pb)
    assert m.requires_grad and m.grad_fn is not None
    m.retain_grad()
    folded = fold_batch(layer.linear.weight, layer.norm.weight, layer.norm.bias, m, EPS, layer.norm.running_mean, layer.norm.running_var, layer.grid)[:3]
    for t in folded:
        if t is not None:
            t.retain_grad()
    net = PillarFeatureNet(*folded)
    (net.pseudo_image(pb) if canvas else net.features(pb)).backward(up_t)
    torch.cuda.synchronize()
    by_hand = [bits(t.grad) for t in (layer.linear.weight, layer.norm.weight, layer.norm.bias, pb.voxels)]
    for got, want_bits in zip((wf, bf) + ((bp,) if bp is not None else ()), folded):
        assert np.array_equal(bits(got).view(np.uint32), bits(want_bits).view(np.uint32))       # the layer's fold is this fold
    # (d): a CPU float64 backward through fold_batch, fed the GPU's gradients of the folded layer
    moments_leaf = moments.clone().requires_grad_(True)
    ref = fold_batch(*leaves, moments_leaf, EPS, before["norm.running_mean"], before["norm.running_var"], layer.grid, dtype=torch.float64)
    outs = [t for t in ref[:3] if t is not None]
    grads = torch.autograd.grad(outs, leaves + [moments_leaf], [t.grad.cpu().double() for t in folded if t is not None])
    for got, want_grad, what in zip(by_hand[:3], grads[:3], ("linear.weight.grad", "norm.weight.grad", "norm.bias.grad")):
        within(got, want_grad.numpy(), what)
        assert float(np.abs(got).max()) > 0
    within(bits(m.grad)[2:], grads[3].numpy()[2:], "moments.grad", rel=2.0 ** -40)
    # (e): the float32 sum of pfn_bwd_ref's d_voxels and the adjoint's restatement, fed the GPU's g_s and H
    kw = dict(d_canvas=up) if canvas else dict(d_features=up)
    kernel = BR.gradients(a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], wn, bn, bpn, capacity=cap, **kw)
    Cc = vox.shape[2]
    mg = bits(m.grad)
    adjoint = SR.moments_backward(a["voxels"], a["num_points"], a["offsets"], mg[2:2 + Cc], mg[2 + Cc:], cap)
    dk = np.zeros(adjoint["d_voxels64"].shape)
    dk[:len(kernel["d_voxels"])] = kernel["d_voxels"]
    total = dk + adjoint["d_voxels64"]
    got = by_hand[3]
    assert got.dtype == F and (got[~adjoint["used"]].view(np.uint32) == 0).all()
    err, bound = np.abs(got.astype(np.float64) - total), SR.backward_bound(adjoint) + 2.0 ** -24 * np.abs(total)
    print("    %-18s max err / bound %.3g" % ("voxels.grad", float((err[adjoint["used"]] / bound[adjoint["used"]]).max())))
    assert (err <= bound).all(), float((err - bound).max())
    assert float(np.abs(adjoint["d_voxels64"]).max()) > 0 and float(np.abs(kernel["d_voxels"]).max()) > 0
    # the layer's own forward and backward give the same bytes
    for t in (layer.linear.weight, layer.norm.weight, layer.norm.bias, pb.voxels):
        t.grad = None
    (layer(pb) if canvas else layer.features(pb)).backward(up_t)
    for got, want_bits in zip((layer.linear.weight, layer.norm.weight, layer.norm.bias, pb.voxels), by_hand):
        assert np.array_equal(bits(got.grad).view(np.uint32), want_bits.view(np.uint32))
    pb.voxels.requires_grad_(False)

    # (f) eval(): the frozen path's bytes, the buffers left alone
    layer.eval()
    state = {k: v.clone() for k, v in layer.state_dict().items()}
    frozen = PillarFeatureNet.from_state_dict(layer.state_dict(), prefix="", eps=EPS, grid=layer.grid)
    with torch.no_grad():
        got = layer(pb) if canvas else layer.features(pb)
    want_eval = frozen.pseudo_image(pb) if canvas else frozen.features(pb)
    assert torch.equal(got[:P if not canvas else None].view(torch.int32), want_eval[:P if not canvas else None].view(torch.int32))
    assert all(torch.equal(v, layer.state_dict()[k]) for k, v in state.items())
    assert list(state.keys()) == list(before.keys())


@pytest.mark.parametrize("name", SC.FALLBACK)
def test_fewer_than_two_rows_fold_the_running_statistics(name):
    from pseudo_lidar import PillarFeatureNet
    a = SC.build(name)
    pb = batch(a, fill=float("nan"))
    layer = make_layer(4, 32, None, 9)
    state = {k: v.clone() for k, v in layer.state_dict().items()}
    out = layer(pb)
    frozen = PillarFeatureNet.from_state_dict(state, prefix="", eps=EPS).pseudo_image(pb)
    assert torch.equal(out.detach().view(torch.int32), frozen.view(torch.int32))
    assert all(torch.equal(v, layer.state_dict()[k]) for k, v in state.items()) and int(layer.norm.num_batches_tracked) == 0
    out.sum().backward()
    assert layer.norm.bias.grad is not None and bool(torch.isfinite(layer.linear.weight.grad).all())


def test_layer_trains_with_batch_statistics():
    """thirty Adam steps on mixed-N5-c9-o64 towards a fixed canvas, the voxels requiring a gradient too: the loss falls and every step
    counts"""
    a = SC.build("mixed-N5-c9-o64")
    pb = batch(a, fill=float("nan"))
    teacher = make_layer(9, 64, None, 31).eval()
    with torch.no_grad():
        target = teacher(pb)
    student = make_layer(9, 64, None, 32)
    opt = torch.optim.Adam(student.parameters(), lr=0.03)
    pb.voxels.requires_grad_(True)
    losses = []
    for step in range(31):
        loss = ((student(pb) - target) ** 2).sum() / (len(a["voxels"]) * 64)
        losses.append(loss.detach())
        opt.zero_grad()
        pb.voxels.grad = None
        loss.backward()
        opt.step()
    losses = [float(v) for v in losses]
    print("loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert int(student.norm.num_batches_tracked) == 31 and bool(torch.isfinite(pb.voxels.grad[:len(a["voxels"])]).all())


# ---------------------------------------------------------------------------------------------- 4. graph capture
def test_capture_and_replay_on_new_contents():
    """pillar_moments(out=) and pillar_moments_backward(out=) captured on one stream as one chain; replayed, and replayed after the
    voxels changed in place: the eager bytes"""
    from pseudo_lidar import pillar_moments, pillar_moments_backward
    a = SC.build("pair-N5-c9-o64")
    pb = batch(a)
    grad = torch.from_numpy(SC.gradient("pair-N5-c9-o64")).to(DEV)
    gm, m = moments_window(9)
    gv, dv = voxels_window(pb)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pillar_moments(pb, out=m)
        pillar_moments_backward(pb, grad, out=dv)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pillar_moments(pb, out=m)
        pillar_moments_backward(pb, grad, out=dv)
    for change in (False, True):
        if change:
            pb.voxels.mul_(-1.5).add_(0.25)
            grad.mul_(0.5)
        m.fill_(SENTINEL); dv.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert gm.intact() and gv.intact()
        eager_m, eager_dv = pillar_moments(pb), pillar_moments_backward(pb, grad)
        assert torch.equal(m.view(torch.int64), eager_m.view(torch.int64)) and torch.equal(dv.view(torch.int32), eager_dv.view(torch.int32))
        vox = pb.voxels.cpu().numpy()[:len(a["voxels"])]
        SR.check_moments(m.cpu().numpy(), SR.moments(vox, a["num_points"], a["offsets"], a["capacity"]), "replay")
    assert not np.array_equal(m.cpu().numpy(), SC.moments("pair-N5-c9-o64")["moments"])


# ---------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_refuses_bad_arguments_untouched():
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401  (registers the signatures)
    h = L.lib()
    a = SC.build("mixed-N5-c9-o64")
    pb = batch(a)
    cap = a["capacity"]
    nbytes = h.mcav_pillar_moments_workspace_bytes(cap, 5, 9)
    assert nbytes >= 8 * 55 and nbytes % 256 == 0
    for bad in ((-1, 5, 9), (cap, 0, 9), (cap, 65, 9), (cap, 5, 5), (cap, 5, 10)):
        assert h.mcav_pillar_moments_workspace_bytes(*bad) == 0, bad
    gm, m = moments_window(9)
    gv, dv = voxels_window(pb)
    ws = torch.full((nbytes + 8,), 0x55, dtype=torch.uint8, device=DEV)
    grad = torch.from_numpy(SC.gradient("mixed-N5-c9-o64")).to(DEV)
    good = dict(v=L.ptr(pb.voxels), n=L.ptr(pb.num_points), o=L.ptr(pb.offsets), B=len(pb), cap=cap, N=5, C=9)
    fwd = dict(good, m=L.ptr(m), ws=L.ptr(ws), bytes=nbytes)
    bwd = dict(good, g=L.c_p(grad.data_ptr() + 16), H=L.c_p(grad.data_ptr() + 88), dv=L.ptr(dv))
    call_f = lambda **kw: h.mcav_pillar_moments(*[dict(fwd, **kw)[k] for k in fwd], L.stream())
    call_b = lambda **kw: h.mcav_pillar_moments_bwd(*[dict(bwd, **kw)[k] for k in bwd], L.stream())
    shared = [dict(v=L.c_p(0)), dict(n=L.c_p(0)), dict(o=L.c_p(0)), dict(B=0), dict(B=-1), dict(B=65536), dict(cap=-1), dict(N=0), dict(N=65),
              dict(C=0), dict(C=5), dict(C=10), dict(v=L.c_p(pb.voxels.data_ptr() + 2))]
    for kw in shared + [dict(m=L.c_p(0)), dict(ws=L.c_p(0)), dict(m=L.c_p(m.data_ptr() + 4)), dict(ws=L.c_p(ws.data_ptr() + 4))]:
        assert call_f(**kw) == -1, kw
    for kw in shared + [dict(g=L.c_p(0)), dict(H=L.c_p(0)), dict(dv=L.c_p(0)), dict(g=L.c_p(grad.data_ptr() + 4)), dict(dv=L.c_p(dv.data_ptr() + 1))]:
        assert call_b(**kw) == -1, kw
    for short in (0, nbytes - 1):
        assert call_f(bytes=short) == -2, short
    torch.cuda.synchronize()
    assert gm.untouched() and gv.untouched() and bool((ws == 0x55).all())
    assert call_f() == 0 and call_b() == 0
    torch.cuda.synchronize()
    assert gm.intact() and gv.intact()
    SR.check_moments(m.cpu().numpy(), SC.moments("mixed-N5-c9-o64"), "abi")
    SR.check_backward(dv.cpu().numpy(), SC.backward("mixed-N5-c9-o64"), "abi")
    with pytest.raises(L.MCAVError):
        pseudo_lidar.pillar_moments(pb, out=m[:-1])
    with pytest.raises(L.MCAVError):
        pseudo_lidar.pillar_moments(pb, out=torch.zeros(92, device=DEV))                   # float32
    with pytest.raises(L.MCAVError):
        pseudo_lidar.pillar_moments_backward(pb, grad.float())
    with pytest.raises(L.MCAVError):
        pseudo_lidar.pillar_moments_backward(pb, grad, out=dv[:-1])
    with pytest.raises(L.MCAVError):
        pseudo_lidar.pillar_moments_backward(pb, grad.cpu())
