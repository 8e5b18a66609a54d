"""GPU: the gradient's way from pillar voxels back to the disparity (include/mcav_depth.h: mcav_pl_batch_project_indexed,
mcav_pillarize_indexed, mcav_pillarize_bwd, mcav_pl_batch_project_bwd; pseudo_lidar.project_batch / pillarize with provenance or a
gradient, project_batch_backward, pillarize_backward) against the restatement (tests/pl_bwd_ref.py), bit for bit, on the cases of
tests/pl_bwd_cases.py: the provenance, sentinels in and behind every buffer, the old entries beside the new ones; the whole chain
disparity -> cloud -> pillars -> canvas under autograd against the chained restatements; repeatability, graph capture and replay on new
contents of the raw calls and of the autograd path; what the graph nodes hold; the path without a gradient; the C ABI's refusals."""
import numpy as np
import pytest
import torch

import pfn_bwd_ref as FB
import pillar_ref as PR
import pl_bwd_cases as C
import pl_bwd_ref as BR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -7.0
PIXEL_SENTINEL = -12345


def dev(v, dtype=None):
    return torch.from_numpy(np.array(v, dtype or v.dtype)).to(DEV)


_TABLES = {}


def tables_of(beams):
    from pseudo_lidar import BeamTables
    key = (len(beams[0]), len(beams[1]))
    if key not in _TABLES:
        _TABLES[key] = BeamTables(*beams)
    return _TABLES[key]


def project(a, m, out=None, **kw):
    """pl_bwd_cases' arguments -> PseudoLiDAR.project_batch; a scale table goes in as the float32 products the restatement forms"""
    from pseudo_lidar import PseudoLiDAR
    pl = PseudoLiDAR.from_matrices(a["T"][0], a["P"][0], a["sparsity"])
    scale = a["scale"] if a["scales"] is None else dev((F(a["scale"]) * a["scales"]).astype(F))
    return pl.project_batch(m, sizes=a["sizes"], P=a["P"], T=a["T"], input=a["input"], scale=scale, max_height=a["max_height"],
                            max_depth=None if np.isinf(a["max_depth"]) else a["max_depth"],
                            beams=None if a["beams"] is None else tables_of(a["beams"]), out=out, padded=(a["Hg"], a["Wg"]), **kw)


def cloud_buffers(case):
    """a CloudBatch of the case's capacity, points and pixels full of sentinels"""
    from pseudo_lidar import CloudBatch
    cb = CloudBatch(C.project_build(case)["m"].shape[0], C.project_capacity(case), DEV)
    cb.points.fill_(SENTINEL)
    cb.pixels = torch.full((cb.points.shape[0],), PIXEL_SENTINEL, dtype=torch.int32, device=DEV)
    return cb


# ---------------------------------------------------------------------------------------------- the projection: provenance and backward
@pytest.mark.parametrize("case", C.PROJECT_CASES)
def test_projection_provenance_and_backward_match_restatement(case):
    from pseudo_lidar import project_batch_backward
    a, fwd, ref = C.project_build(case), C.project_forward(case), C.project_reference(case)
    C.project_non_trivial(case)
    n = len(fwd["pixels"])
    m = dev(a["m"])
    plain = cloud_buffers(case)
    plain.pixels = None
    project(a, m, out=plain)                                       # the old entry
    cb = cloud_buffers(case)
    pixels = cb.pixels
    assert project(a, m, out=cb, provenance=True) is cb and cb.pixels is pixels and cb.points.grad_fn is None and plain.pixels is None
    assert np.array_equal(cb.offsets.cpu().numpy(), fwd["offsets"])
    C.same_bits(cb.points[:n].cpu().numpy(), fwd["cloud"])
    assert torch.equal(cb.points.view(torch.int32), plain.points.view(torch.int32)) and torch.equal(cb.offsets, plain.offsets)
    assert bool((cb.points[n:] == SENTINEL).all())
    assert np.array_equal(cb.pixels[:n].cpu().numpy(), fwd["pixels"]) and bool((cb.pixels[n:] == PIXEL_SENTINEL).all())

    B, h, w = a["m"].shape
    out = torch.full((B, h, w), SENTINEL, device=DEV)
    got = project_batch_backward(cb, dev(C.project_upstream(case)), out=out)       # NaN behind the rows that exist
    assert got is out
    G = cb._bwd_ws[0][:4 * B * a["Hg"] * a["Wg"]].view(torch.float32).reshape(B, a["Hg"], a["Wg"])
    C.same_bits(G.cpu().numpy(), ref["G"])
    C.same_bits(out.cpu().numpy(), ref["d_m"])
    again = project_batch_backward(cb, dev(C.project_upstream(case)))
    assert again.data_ptr() != out.data_ptr() and torch.equal(again.view(torch.int32), out.view(torch.int32))


# ---------------------------------------------------------------------------------------------- the pillars: provenance and backward
def pillar_grid(g=C.GRID):
    from pseudo_lidar import PillarGrid
    pg = PillarGrid(x=(float(g.x0), float(g.x0) + g.nx * float(g.vx)), y=(float(g.y0), float(g.y0) + g.ny * float(g.vy)),
                    z=(float(g.z0), float(g.z1)), size=(float(g.vx), float(g.vy)))
    assert (pg.nx, pg.ny) == (g.nx, g.ny)
    return pg


def pillar_buffers(case):
    from pseudo_lidar import PillarBatch
    a = C.pillar_build(case)
    cap = C.pillar_capacity(case)
    pb = PillarBatch(3, cap, a["max_points"], 9 if a["decorate"] else 4, DEV)
    pb.voxels.fill_(SENTINEL); pb.coords.fill_(1 << 20); pb.num_points.fill_(1 << 20)
    pb.slot_points = torch.full((cap, a["max_points"]), PIXEL_SENTINEL, dtype=torch.int32, device=DEV)
    return pb


@pytest.mark.parametrize("case", C.PILLAR_CASES)
def test_pillar_provenance_and_backward_match_restatement(case):
    from pseudo_lidar import pillarize, pillarize_backward
    a, fwd, ref = C.pillar_build(case), C.pillar_forward(case), C.pillar_reference(case)
    C.pillar_non_trivial(case)
    P = len(fwd["coords"])
    pts, off = dev(a["points"]), dev(a["offsets"])
    kw = dict(grid=pillar_grid(), max_points=a["max_points"], decorate=a["decorate"])
    plain = pillar_buffers(case)
    plain.slot_points = None
    pillarize(pts, off, out=plain, **kw)                           # the old entry
    pb = pillar_buffers(case)
    slots = pb.slot_points
    assert pillarize(pts, off, out=pb, provenance=True, **kw) is pb and pb.slot_points is slots and pb.voxels.grad_fn is None
    assert plain.slot_points is None
    for name in ("voxels", "coords", "num_points", "offsets"):
        x, y = getattr(pb, name), getattr(plain, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert np.array_equal(pb.offsets.cpu().numpy(), fwd["offsets"])
    C.same_bits(pb.voxels[:P].cpu().numpy(), fwd["voxels"])
    assert bool((pb.voxels[P:] == SENTINEL).all())
    assert np.array_equal(pb.slot_points[:P].cpu().numpy(), fwd["slot_points"]) and bool((pb.slot_points[P:] == PIXEL_SENTINEL).all())

    out = torch.full((len(a["points"]), 4), SENTINEL, device=DEV)
    got = pillarize_backward(pb, dev(C.pillar_upstream(case)), out=out)             # NaN behind the pillars that exist
    assert got is out
    C.same_bits(out.cpu().numpy(), ref["d_points"])
    again = pillarize_backward(pb, dev(C.pillar_upstream(case)))
    assert again.data_ptr() != out.data_ptr() and torch.equal(again.view(torch.int32), out.view(torch.int32))


# ---------------------------------------------------------------------------------------------- disparity -> canvas under autograd
BEV = PR.make_grid(x=(0.0, 48.0), y=(-16.0, 16.0), z=(-3.0, 1.0), size=(2.0, 2.0))        # 24 x 16 cells over the scene
BEV_SLOTS = 4


def make_layer(seed):
    from pseudo_lidar import PillarFeatureLayer
    torch.manual_seed(seed)
    layer = PillarFeatureLayer(9, 32)
    with torch.no_grad():
        layer.linear.weight.mul_(0.5)
        layer.norm.running_mean.copy_(torch.randn(32) * 0.1)
        layer.norm.running_var.copy_(torch.rand(32) + 0.5)
        layer.norm.bias.copy_(torch.randn(32) * 0.2)
    return layer.to(DEV)


def chained_reference(a, fixed, weight, bias):
    """disparity -> d_disparity through the restatements: the forwards with their provenance, then pfn_bwd_ref -> pillars -> projection"""
    fwd = BR.project_forward(**a)
    B = a["m"].shape[0]
    cap = B * a["Hg"] * a["Wg"] if a["beams"] is None else B * (len(a["beams"][0]) - 1) * (len(a["beams"][1]) - 1)
    pil = PR.pillarize(fwd["cloud"], fwd["offsets"], BEV, BEV_SLOTS, decorate=True)
    slots = BR.pillar_slots(fwd["cloud"], fwd["offsets"], BEV, BEV_SLOTS)
    g = FB.gradients(pil["voxels"], pil["coords"], pil["num_points"], pil["offsets"], BEV.nx, BEV.ny, weight, bias, d_canvas=fixed)
    d_points = BR.pillarize_bwd(g["d_voxels"], slots, pil["num_points"], cap)["d_points"]
    out = BR.project_bwd(d_points, fwd, **a)
    return fwd, pil, d_points, out["d_m"]


@pytest.mark.parametrize("case", ["odd-dense", "odd-beams8x16"])
def test_disparity_gradient_through_the_whole_chain(case):
    """a leaf disparity -> project_batch -> .pillars(decorate=True) -> PillarFeatureLayer(9, 32) -> (canvas * fixed).sum().backward():
    disp.grad is the chained restatements' gradient, bit for bit"""
    a = C.project_build(case)
    B, h, w = a["m"].shape
    layer = make_layer(3)
    disp = dev(a["m"])[:, None].clone().requires_grad_(True)      # [B, 1, h, w], as the network hands it over
    cloud = project(a, disp)
    assert cloud.points.requires_grad and cloud.points.grad_fn is not None and cloud.pixels is not None
    pillars = cloud.pillars(grid=pillar_grid(BEV), max_points=BEV_SLOTS, decorate=True)
    assert pillars.voxels.grad_fn is not None and pillars.slot_points is not None
    canvas = layer(pillars)
    fixed = np.random.RandomState(77).standard_normal(tuple(canvas.shape)).astype(F)
    (canvas * dev(fixed)).sum().backward()
    assert disp.grad is not None and tuple(disp.grad.shape) == (B, 1, h, w)
    weight, bias, _ = (None if t is None else t.detach().cpu().numpy() for t in layer.folded())
    fwd, pil, d_points, want = chained_reference(a, fixed, weight, bias)
    n, P = len(fwd["pixels"]), len(pil["coords"])
    C.same_bits(cloud.points[:n].detach().cpu().numpy(), fwd["cloud"])
    C.same_bits(pillars.voxels[:P].detach().cpu().numpy(), pil["voxels"])
    assert P >= 20 and (d_points[:n, :3] != 0).any() and (want != 0).reshape(B, -1).any(axis=1).all()
    C.same_bits(disp.grad[:, 0].cpu().numpy(), want)
    assert layer.linear.weight.grad is not None and bool((layer.linear.weight.grad != 0).any())      # the layer still learns beside it


def test_two_runs_give_the_same_bytes_and_objects_are_reusable():
    """the chain twice into the same CloudBatch and PillarBatch (out=): identical gradients; a stale backward is refused"""
    from mcav import lib as L
    a = C.project_build("odd-dense")
    layer = make_layer(4)
    fixed = None
    grads, cloud, pillars = [], None, None
    for _ in range(2):
        disp = dev(a["m"]).requires_grad_(True)
        cloud = project(a, disp, out=cloud)
        pillars = cloud.pillars(grid=pillar_grid(BEV), max_points=BEV_SLOTS, decorate=True, out=pillars)
        canvas = layer(pillars)
        fixed = torch.randn(canvas.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) if fixed is None else fixed
        (canvas * fixed).sum().backward()
        grads.append(disp.grad)
    assert grads[0].data_ptr() != grads[1].data_ptr() and torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    assert bool((grads[0] != 0).any())
    disp = dev(a["m"]).requires_grad_(True)
    stale = project(a, disp, out=cloud).points.sum()
    project(a, disp, out=cloud)
    with pytest.raises(L.MCAVError, match="again"):
        stale.backward()


def test_capture_and_replay_on_new_contents():
    """both forwards with provenance and both backwards, captured as plain calls into fixed buffers, replayed after the plane and the
    upstream gradient changed in place: the bytes of an eager run"""
    import pl_batch_cases as PC
    from pseudo_lidar import CloudBatch, PillarBatch, pillarize, pillarize_backward, project_batch_backward
    a = C.project_build("odd-dense")
    B, h, w = a["m"].shape
    cap = B * a["Hg"] * a["Wg"]
    grid = pillar_grid(BEV)
    pcap = min(cap, B * grid.nx * grid.ny)

    def chain(m, up, cloud, pillars, d_points, d_m):
        project(a, m, out=cloud, provenance=True)
        pillarize(cloud.points, cloud.offsets, grid=grid, max_points=BEV_SLOTS, decorate=True, out=pillars, provenance=True)
        pillarize_backward(pillars, up, out=d_points)
        project_batch_backward(cloud, d_points, out=d_m)

    def buffers():
        return (CloudBatch(B, cap, DEV), PillarBatch(B, pcap, BEV_SLOTS, 9, DEV), torch.empty(cap, 4, device=DEV), torch.empty(B, h, w, device=DEV))

    m, up = dev(a["m"]), torch.randn(pcap, BEV_SLOTS, 9, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    held = buffers()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain(m, up, *held)                                        # warm-up: tables, workspaces and provenance buffers exist
    torch.cuda.current_stream().wait_stream(s)
    first = held[3].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(m, up, *held)
    other = np.stack([PC.network_map(h, w, 900 + b, "disparity") for b in range(B)])
    other[~np.isfinite(other)] = F(0.03)
    m.copy_(dev(other))
    up.copy_(torch.randn(up.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(7)))
    held[2].fill_(SENTINEL); held[3].fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    eager = buffers()
    chain(m, up, *eager)
    assert torch.equal(held[0].offsets, eager[0].offsets) and not torch.equal(held[3], first)
    assert torch.equal(held[2].view(torch.int32), eager[2].view(torch.int32)) and torch.equal(held[3].view(torch.int32), eager[3].view(torch.int32))
    fwd = BR.project_forward(**dict(a, m=other))
    slots = BR.pillar_slots(fwd["cloud"], fwd["offsets"], BEV, BEV_SLOTS)
    num = PR.pillarize(fwd["cloud"], fwd["offsets"], BEV, BEV_SLOTS, decorate=True)["num_points"]
    d_points = BR.pillarize_bwd(up.cpu().numpy(), slots, num, cap)["d_points"]
    C.same_bits(held[2].cpu().numpy(), d_points)
    C.same_bits(held[3].cpu().numpy(), BR.project_bwd(d_points, fwd, **dict(a, m=other))["d_m"])


def test_autograd_chain_captures_and_replays():
    """the autograd path itself under capture: a disparity that requires a gradient -> project_batch(out=) -> pillars(out=) ->
    (voxels * fixed).sum().backward(), captured once and replayed after the disparity changed in place: disp.grad holds the bytes of an
    eager run on the new contents (both nodes, their saved tensors, the stamp and the reused buffers are part of what is captured)"""
    import pl_batch_cases as PC
    from pseudo_lidar import CloudBatch, PillarBatch
    a = C.project_build("odd-dense")
    B, h, w = a["m"].shape
    cap = B * a["Hg"] * a["Wg"]
    grid = pillar_grid(BEV)
    pcap = min(cap, B * grid.nx * grid.ny)
    fixed = torch.randn(pcap, BEV_SLOTS, 9, device=DEV, generator=torch.Generator(DEV).manual_seed(8))

    def step(disp, cloud, pillars):
        project(a, disp, out=cloud)
        cloud.pillars(grid=grid, max_points=BEV_SLOTS, decorate=True, out=pillars)
        (pillars.voxels * fixed).sum().backward()

    disp = dev(a["m"]).requires_grad_(True)
    cloud, pillars = CloudBatch(B, cap, DEV), PillarBatch(B, pcap, BEV_SLOTS, 9, DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    warm = disp.detach().clone().requires_grad_(True)             # a leaf of its own: the captured leaf's accumulation node is made
    with torch.cuda.stream(s):                                     # on the capturing stream
        step(warm, cloud, pillars)                                 # warm-up: tables, workspaces and provenance buffers exist
    torch.cuda.current_stream().wait_stream(s)
    first = warm.grad
    assert disp.grad is None                                       # the captured backward allocates it from the capture's pool
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(disp, cloud, pillars)
    other = np.stack([PC.network_map(h, w, 900 + b, "disparity") for b in range(B)])
    other[~np.isfinite(other) | (other < 0)] = F(0.03)
    with torch.no_grad():
        disp.copy_(dev(other))
    disp.grad.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    eager = dev(other).requires_grad_(True)
    step(eager, CloudBatch(B, cap, DEV), PillarBatch(B, pcap, BEV_SLOTS, 9, DEV))
    assert bool((eager.grad != 0).any()) and not torch.equal(eager.grad, first)
    assert torch.equal(disp.grad.view(torch.int32), eager.grad.view(torch.int32))


def test_nodes_hold_tensors_not_objects():
    """the graph keeps what backward needs alive without the CloudBatch / PillarBatch (no reference cycle through them), and an in-place
    change of the disparity between forward and backward is refused by autograd's version check"""
    import gc
    import weakref
    a = C.project_build("odd-dense")
    fixed = None
    grads = []
    for drop in (False, True):
        disp = dev(a["m"]).requires_grad_(True)
        cloud = project(a, disp)
        pillars = cloud.pillars(grid=pillar_grid(BEV), max_points=BEV_SLOTS, decorate=True)
        voxels = pillars.voxels
        fixed = torch.randn(voxels.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(9)) if fixed is None else fixed
        if drop:
            refs = weakref.ref(cloud), weakref.ref(pillars)
            gc.disable()
            try:
                del cloud, pillars
                assert refs[0]() is None and refs[1]() is None     # freed by reference counting alone
            finally:
                gc.enable()
        (voxels * fixed).sum().backward()
        grads.append(disp.grad)
    assert bool((grads[0] != 0).any()) and torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    disp = dev(a["m"]).requires_grad_(True)
    plane = disp * 1.0
    loss = project(a, plane).points.sum()
    plane.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


# ---------------------------------------------------------------------------------------------- without a gradient
def test_without_a_gradient_nothing_changes():
    a = C.project_build("odd-dense")
    fwd = C.project_forward("odd-dense")
    n = len(fwd["pixels"])
    m = dev(a["m"])
    cloud = project(a, m)
    assert cloud.points.grad_fn is None and not cloud.points.requires_grad and cloud.pixels is None
    C.same_bits(cloud.points[:n].cpu().numpy(), fwd["cloud"])
    pillars = cloud.pillars(grid=pillar_grid(BEV), max_points=BEV_SLOTS, decorate=True)
    assert pillars.voxels.grad_fn is None and not pillars.voxels.requires_grad and pillars.slot_points is None
    want = PR.pillarize(fwd["cloud"], fwd["offsets"], BEV, BEV_SLOTS, decorate=True)
    C.same_bits(pillars.voxels[:len(want["coords"])].cpu().numpy(), want["voxels"])
    with torch.no_grad():                                          # grad mode off: a plane that requires a gradient changes nothing
        quiet = project(a, m.clone().requires_grad_(True))
    assert quiet.points.grad_fn is None and quiet.pixels is None and torch.equal(quiet.points[:n].view(torch.int32), cloud.points[:n].view(torch.int32))
    # an object that carried a graph goes back to its plain buffer
    live = project(a, m.clone().requires_grad_(True))
    assert live.points.grad_fn is not None
    ptr = live.points.data_ptr()
    project(a, m, out=live)
    assert live.points.grad_fn is None and live.pixels is None and live.points.data_ptr() == ptr


# ---------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_refuses_bad_arguments():
    """return codes only: nothing is launched with a bad pointer"""
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401
    hl = L.lib()
    B, h, w, Hg, Wg, cap = 2, 8, 13, 23, 37, 64
    t = dict(d_points=torch.zeros(cap + 1, 4, device=DEV), pixels=torch.zeros(cap, dtype=torch.int32, device=DEV),
             offsets=torch.zeros(B + 1, dtype=torch.int32, device=DEV), m=torch.zeros(B, h, w, device=DEV),
             sizes=torch.tensor([[Hg, Wg]] * B, dtype=torch.int32, device=DEV), calib=torch.zeros(B, 28, dtype=torch.float64, device=DEV),
             d_m=torch.full((B, h, w), SENTINEL, device=DEV))
    nbytes = hl.mcav_pl_batch_project_bwd_workspace_bytes(B, Hg, Wg)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)

    def plane(**kw):
        arg = dict({k: L.ptr(v) for k, v in t.items()}, capacity=cap, B=B, h=h, w=w, Hg=Hg, Wg=Wg, scale=1.0, scales=L.c_p(0), flags=0,
                   ws=L.ptr(ws), nbytes=nbytes)
        arg.update(kw)
        return hl.mcav_pl_batch_project_bwd(*[arg[k] for k in ("d_points", "capacity", "pixels", "offsets", "m", "B", "h", "w", "Hg", "Wg", "sizes",
                                                               "calib", "scale", "scales", "flags", "d_m", "ws", "nbytes")], L.stream())

    for kw in (dict(d_points=L.c_p(0)), dict(pixels=L.c_p(0)), dict(offsets=L.c_p(0)), dict(m=L.c_p(0)), dict(sizes=L.c_p(0)), dict(calib=L.c_p(0)),
               dict(d_m=L.c_p(0)), dict(ws=L.c_p(0)), dict(B=0), dict(h=0), dict(w=0), dict(Hg=0), dict(Wg=-1), dict(flags=2),
               dict(scale=float("nan")), dict(d_points=L.c_p(t["d_points"].data_ptr() + 4)), dict(ws=L.c_p(ws.data_ptr() + 1)),
               dict(Hg=1 << 16, Wg=1 << 16)):
        assert plane(**kw) == -1, kw
    assert plane(nbytes=nbytes - 1) == -2
    torch.cuda.synchronize()
    assert bool((t["d_m"] == SENTINEL).all())
    assert plane() == 0                                            # an empty cloud: every element written, +0.0
    torch.cuda.synchronize()
    assert bool((t["d_m"].view(torch.int32) == 0).all())

    N, pcap, n_max = 3, 5, 11
    p = dict(d_voxels=torch.zeros(pcap * N * 9 + 1, device=DEV), slots=torch.zeros(pcap, N, dtype=torch.int32, device=DEV),
             num=torch.zeros(pcap, dtype=torch.int32, device=DEV), poff=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
             d_points=torch.full((n_max + 1, 4), SENTINEL, device=DEV))

    def pillars(**kw):
        arg = dict({k: L.ptr(v) for k, v in p.items()}, B=B, capacity=pcap, N=N, flags=1, n_max=n_max)
        arg.update(kw)
        return hl.mcav_pillarize_bwd(*[arg[k] for k in ("d_voxels", "slots", "num", "poff", "B", "capacity", "N", "flags", "d_points", "n_max")],
                                     L.stream())

    for kw in (dict(d_voxels=L.c_p(0)), dict(slots=L.c_p(0)), dict(num=L.c_p(0)), dict(poff=L.c_p(0)), dict(d_points=L.c_p(0)), dict(B=0),
               dict(B=65536), dict(capacity=-1), dict(N=0), dict(N=65), dict(flags=2), dict(n_max=-1), dict(n_max=1 << 31),
               dict(d_points=L.c_p(p["d_points"].data_ptr() + 4)), dict(d_voxels=L.c_p(p["d_voxels"].data_ptr() + 2))):
        assert pillars(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((p["d_points"] == SENTINEL).all())
    assert pillars() == 0                                          # no pillars: every row +0.0, nothing behind n_max touched
    torch.cuda.synchronize()
    assert bool((p["d_points"][:n_max].view(torch.int32) == 0).all()) and bool((p["d_points"][n_max:] == SENTINEL).all())
    # the indexed forwards refuse a null provenance buffer before anything else
    assert hl.mcav_pl_batch_project_indexed(None, B, h, w, Hg, Wg, None, None, None, None, None, 0, 0, 1.0, None, 1.0, 1.0, 0, 0, None, 0, None,
                                            None, None, 0, None) == -1
    assert hl.mcav_pillarize_indexed(None, None, B, 0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1, 1, 1, 0, None, None, None, 0, None, None, None, 0,
                                     None) == -1
