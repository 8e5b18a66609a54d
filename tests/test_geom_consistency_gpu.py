"""GPU: the depth geometry-consistency kernels (include/mcav_depth.h: mcav_geom_consistency_fwd / _bwd) against the float64 definition
(tests/geom_consistency_ref.py) on the inputs of tests/test_geom_consistency_cpu.py, their determinism contracts, and the term inside
Losses, a captured graph and the trainer.

Tolerances are not chosen here: test_geom_consistency_cpu.HOST_DEV records, per case and per tensor, the measured deviation of the
header's arithmetic on the host (fp32, no FMA) from float64; the kernels get 4x that (FMA contraction, v_rcp + Newton) plus 1e-7 of the
tensor's maximum.  Pixels the definition itself flags as ties (within 1e-3 of a validity border, a cell edge or D_proj = D_samp; at most
0.5 % by the choice of seeds, capped at 1 % here) and, for the gradients, the texels their taps reach are left out of the per-pixel
comparison.  Only a pixel at a validity BORDER can change n_d; the loss gets the worst such pixels can do on top of the kernel
tolerance, 0.5 * #border-flagged / n_d per direction (test_geom_consistency_cpu.scalar_allowance) -- the seeds in use have none, so that
is zero -- and d_poses the kernel tolerance alone."""
import numpy as np
import pytest
import torch

import geom_consistency_ref as R
import test_geom_consistency_cpu as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def hip_run(dt, dr, poses, K, min_valid, weight=1.0, upstream=None, inputs_are_depth=False, want_diff=True, grads=None, accumulate=0,
            backward=True, loss0=0.0, lds_tile=False):
    """The C ABI, directly.  Inputs: CPU tensors (any float dtype; K stays float64).  -> dict of CPU tensors."""
    import losses  # noqa: F401  (registers the signatures)
    import mcav.lib as L
    h = L.lib()
    a, b, p = (t.to(DEV, torch.float32).contiguous() for t in (dt, dr, poses))
    k = K.to(DEV).contiguous()
    B, _, H, W = a.shape
    flags = (L.WL_K_F64 if k.dtype == torch.float64 else 0) | (L.WL_INPUT_DEPTH if inputs_are_depth else 0)
    ws = L.workspace(h.mcav_geom_consistency_workspace_bytes(B, H, W), a.device, "geom_consistency")
    saved = torch.empty(4 + 24 * B, dtype=torch.float64, device=DEV)
    loss = torch.full((1,), loss0, dtype=torch.float32, device=DEV)
    diff = torch.empty(B, 2, H, W, dtype=torch.float32, device=DEV) if want_diff else None
    flags |= L.GC_LDS_TILE if lds_tile else 0                          # (the backward's scatter form; the forward ignores it)
    args = [L.ptr(a), L.ptr(b), L.ptr(p), L.ptr(k), B, H, W, flags, min_valid, weight, L.ptr(saved)]
    L.check(h.mcav_geom_consistency_fwd(*args, L.ptr(loss), L.ptr(diff), L.ptr(ws), ws.numel(), L.stream()), "fwd")
    out = dict(saved=saved)
    if backward:
        g = grads if grads is not None else [torch.empty_like(a), torch.empty_like(b), torch.empty_like(p)]
        up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
        L.check(h.mcav_geom_consistency_bwd(*args, L.ptr(up), L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), accumulate, L.ptr(ws), ws.numel(),
                                            L.stream()), "bwd")
        out.update(d_disp_t=g[0].cpu(), d_disp_r=g[1].cpu(), d_poses=g[2].cpu())
    torch.cuda.synchronize()
    sv = saved.cpu()
    out.update(loss=float(loss.cpu()[0]), n=[int(sv[0]), int(sv[1])], diff=diff.cpu() if want_diff else None, saved=sv)
    return out


@pytest.mark.parametrize("name", list(C.CASES))
def test_parity_with_the_definition(name):
    dt, dr, poses, K, mv = C.case_inputs(name)
    ref = C.reference(name)
    C.check_case_ties(name, ref)                                       # the seeds' share of ties, by the definition itself
    got = hip_run(dt, dr, poses, K, mv)
    assert float(ref["flagged"].double().mean()) <= 0.01               # the share left out of the per-pixel comparison
    assert got["n"] == ref["n"]                                        # no pixel sits at a validity border
    assert bool(((got["diff"] >= 0) == (ref["diff"] >= 0)).all())      # the same pixels are valid
    dev = C.deviations(got, ref)
    allow = {k: 4 * C.HOST_DEV[name][k] + 1e-7 + (C.scalar_allowance(ref) if k == "loss" else 0.0) for k in dev}
    print(name, "n", got["n"], "deviation / allowance:", {k: "%.3g / %.3g" % (dev[k], allow[k]) for k in dev})
    for k in dev:
        assert dev[k] <= allow[k], (k, dev[k], allow[k])
    assert float(got["d_poses"][:, 1].abs().max()) == 0.0              # pose[:,1] takes no part


def test_two_runs_and_a_permuted_batch_are_bit_identical():
    dt, dr, poses, K, mv = C.case_inputs("23x37")
    a = hip_run(dt, dr, poses, K, mv)
    b = hip_run(dt, dr, poses, K, mv)
    perm = [1, 0]
    c = hip_run(dt[perm], dr[perm], poses[perm], K[perm], mv)
    assert a["loss"] == b["loss"] == c["loss"] and a["n"] == b["n"] == c["n"]
    for k in ("diff", "d_disp_t", "d_disp_r", "d_poses"):
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k][perm], c[k]), k
    assert torch.equal(a["saved"][:4], c["saved"][:4])


def test_many_to_one_is_bit_identical_from_run_to_run():
    """Every pixel of direction 0 adds into a few dozen texels: contended integer adds, arrival order changes from run to run."""
    dt, dr, poses, K, mv = C.case_inputs("many_to_one")
    a = hip_run(dt, dr, poses, K, mv)
    b = hip_run(dt, dr, poses, K, mv)
    assert int((a["d_disp_r"] != 0).sum()) < 100 and float(a["d_disp_r"].abs().max()) > 0
    for k in ("d_disp_t", "d_disp_r", "d_poses"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["23x37", "many_to_one", "24x40"])
def test_lds_tile_scatter_gives_the_same_bits(name):
    """MCAV_GC_LDS_TILE: the same integer sums through an LDS tile.  23x37: ragged tiles, most taps inside the halo; many-to-one:
    every tile but the central ones overflows its halo into global adds, all on a few dozen texels."""
    dt, dr, poses, K, mv = C.case_inputs(name)
    a = hip_run(dt, dr, poses, K, mv)
    b = hip_run(dt, dr, poses, K, mv, lds_tile=True)
    assert a["loss"] == b["loss"] and float(a["d_disp_r"].abs().max()) > 0
    for k in ("diff", "d_disp_t", "d_disp_r", "d_poses"):
        assert torch.equal(a[k], b[k]), k


def test_forward_without_backward_leaves_nothing_behind():
    dt, dr, poses, K, mv = C.case_inputs("24x40")
    a = hip_run(dt, dr, poses, K, mv)
    dt2, dr2, poses2, K2, _ = C.case_inputs("many_to_one")
    hip_run(dt2, dr2, poses2, K2, mv, backward=False)                  # another forward in the same workspace, no backward
    hip_run(dt, dr, poses, K, mv, backward=False)
    b = hip_run(dt, dr, poses, K, mv)
    assert a["loss"] == b["loss"] and a["n"] == b["n"]
    for k in ("diff", "d_disp_t", "d_disp_r", "d_poses"):
        assert torch.equal(a[k], b[k]), k


def test_loss_accumulates_and_accumulate_adds():
    dt, dr, poses, K, mv = C.case_inputs("8x16")
    a = hip_run(dt, dr, poses, K, mv, weight=0.5, upstream=3.0)
    assert a["loss"] > 0
    base = [torch.full_like(a[k], v).to(DEV) for k, v in (("d_disp_t", 0.25), ("d_disp_r", -0.5), ("d_poses", 2.0))]
    want = [b.cpu() + a[k] for b, k in zip(base, ("d_disp_t", "d_disp_r", "d_poses"))]
    c = hip_run(dt, dr, poses, K, mv, weight=0.5, upstream=3.0, grads=base, accumulate=1, loss0=1.5)
    assert c["loss"] == float(np.float32(1.5) + np.float32(a["loss"]))
    for w, k in zip(want, ("d_disp_t", "d_disp_r", "d_poses")):
        assert torch.equal(c[k], w), k
    one = hip_run(dt, dr, poses, K, mv)                                # weight and upstream scale the gradients: 0.5 * 3
    for k in ("d_disp_t", "d_disp_r", "d_poses"):
        assert float((a[k] - 1.5 * one[k]).abs().max()) <= 2e-6 * float(one[k].abs().max()), k


def test_closed_forms():
    C.check_closed_forms(lambda Dt, Dr, p, K, mv: hip_run(Dt, Dr, p, K, mv, inputs_are_depth=True))


def test_float32_intrinsics_are_the_same_call():
    dt, dr, poses, K, mv = C.case_inputs("23x37")
    a = hip_run(dt, dr, poses, K, mv)
    b = hip_run(dt, dr, poses, K.float(), mv)
    for k in ("diff", "d_disp_t", "d_disp_r", "d_poses"):
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- inside Losses
def loss_inputs(B=2, H=24, W=40, seed=3):
    dt, dr, poses, K = R.inputs(B, H, W, seed)
    g = torch.Generator().manual_seed(seed + 100)
    imgs = [torch.rand(B, 3, H, W, generator=g) for _ in range(3)]
    return imgs, dt.float(), dr.float(), poses.float(), K


def losses_run(crit, imgs, dt, dr, poses, K):
    x, y, z = (t.to(DEV).clone().requires_grad_() for t in (dt, dr, poses))
    out = crit.forward(imgs[0].to(DEV), [imgs[1].to(DEV), imgs[2].to(DEV)], [[x], [y]], z, K.to(DEV), None)
    sum(out).backward()
    torch.cuda.synchronize()
    return [o.detach().cpu() for o in out], [t.grad.cpu() for t in (x, y, z)]


def test_losses_off_is_todays_losses():
    from losses import Losses
    inp = loss_inputs()
    a = losses_run(Losses(), *inp)
    b = losses_run(Losses(geometry_consistency=False), *inp)
    assert len(a[0]) == len(b[0]) == 2
    for p, q in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(p, q)
    crit = Losses()
    assert (crit.geometry_consistency, crit.geometry_consistency_weight, crit.geometry_min_valid, crit.keep_consistency) == (False, 0.5, 100, False)
    assert crit.consistency is None


def test_losses_on_adds_the_term_and_its_gradients():
    from losses import Losses
    imgs, dt, dr, poses, K = loss_inputs()
    base = losses_run(Losses(), imgs, dt, dr, poses, K)
    crit = Losses(geometry_consistency=True, keep_consistency=True)
    on = losses_run(crit, imgs, dt, dr, poses, K)
    term = hip_run(dt, dr, poses, K, 100, weight=0.5)
    assert len(on[0]) == 3
    assert torch.equal(on[0][0], base[0][0]) and torch.equal(on[0][1], base[0][1])
    assert float(on[0][2]) == term["loss"] > 0
    for g_on, g_base, k in zip(on[1], base[1], ("d_disp_t", "d_disp_r", "d_poses")):
        want = g_base + term[k]                                        # autograd adds the two nodes' gradients in fp32
        assert float((g_on - want).abs().max()) <= 1e-6 * float(want.abs().max()), k
        assert float(term[k].abs().max()) > 0
    assert tuple(crit.consistency.shape) == (2, 2, 24, 40) and torch.equal(crit.consistency.cpu(), term["diff"])
    crit2 = Losses(geometry_consistency=True, geometry_consistency_weight=0.25, geometry_min_valid=10 ** 6)
    off = losses_run(crit2, imgs, dt, dr, poses, K)                    # n_d <= min_valid: the term and its gradients vanish
    assert float(off[0][2]) == 0.0
    for p, q in zip(off[1], base[1]):
        assert torch.equal(p, q)


def test_multiscale_path_takes_scale_0():
    """Two scales per pass: the third loss is the single-scale term on scale 0, its gradient reaches scale 0 and the poses, and the
    coarse maps get none from it."""
    from losses import Losses
    imgs, dt, dr, poses, K = loss_inputs()
    T = [i.to(DEV) for i in imgs]
    coarse = lambda t: torch.nn.functional.avg_pool2d(t, 2).contiguous()
    leaves = [t.to(DEV).clone().requires_grad_() for t in (dt, dr, coarse(dt), coarse(dr), poses)]
    x, y, xc, yc, z = leaves
    out = Losses(geometry_consistency=True).forward(T[0], [T[1], T[2]], [[x, xc], [y, yc]], z, K.to(DEV), None)
    assert len(out) == 3
    grads = torch.autograd.grad(out[2], leaves, allow_unused=True)
    torch.cuda.synchronize()
    term = hip_run(dt, dr, poses, K, 100, weight=0.5)
    assert float(out[2].detach()) == term["loss"]
    assert torch.equal(grads[0].cpu(), term["d_disp_t"]) and torch.equal(grads[1].cpu(), term["d_disp_r"])
    assert torch.equal(grads[4].cpu(), term["d_poses"])
    assert all(g is None or float(g.abs().max()) == 0.0 for g in grads[2:4])


def test_graph_replay_matches_eager():
    """The node's forward + backward captured in a hipGraph (two memset nodes, three launches, no host sync) and replayed on new poses
    and disparities: bit-equal to the eager run."""
    from losses import Losses
    _, dt, dr, poses, K = loss_inputs()
    _, dt2, dr2, poses2, _ = loss_inputs(seed=4)
    crit = Losses(geometry_consistency=True)
    Kd = K.to(DEV)
    x, y, z = (t.to(DEV).clone().requires_grad_() for t in (dt, dr, poses))

    def step():
        for p in (x, y, z):
            p.grad = None
        out = crit.geometry_consistency_loss(x, y, z, Kd)
        out.backward()
        return out.detach()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g = step()
        grads_g = [x.grad, y.grad, z.grad]
    with torch.no_grad():
        x.copy_(dt2.to(DEV)); y.copy_(dr2.to(DEV)); z.copy_(poses2.to(DEV))
    g.replay()
    torch.cuda.synchronize()
    want = hip_run(dt2, dr2, poses2, K, 100, weight=0.5, upstream=1.0)
    first = hip_run(dt, dr, poses, K, 100, weight=0.5, upstream=1.0)
    assert float(out_g) == want["loss"] != first["loss"]
    for a, k in zip(grads_g, ("d_disp_t", "d_disp_r", "d_poses")):
        assert torch.equal(a.detach().cpu(), want[k]), k


def test_trainer_config_key_eager_and_hipgraph():
    """`loss: {geometry_consistency: true, ...}` in the trainer config: one step at 2 x 64 x 128, issued eagerly and as a captured
    hipGraph, gives the same three losses and parameters."""
    import dp_worker as WK
    from oracle.step import synthetic_batch
    from trainer import Trainer
    results = []
    for graph in (0, 1):
        cfg = WK.build_config(64, 128, 2, graph)
        cfg["loss"] = dict(cfg.get("loss") or {}, geometry_consistency=True, geometry_consistency_weight=0.5, geometry_min_valid=100)
        t = Trainer(cfg)
        assert t.criterion.geometry_consistency and t.criterion.geometry_consistency_weight == 0.5 and t.criterion.geometry_min_valid == 100
        WK.seed_models(t)
        t.set_train()
        _, loss = t.train_step(synthetic_batch(2, 64, 128, seed=70))
        torch.cuda.synchronize()
        results.append(([float(x.detach()) for x in loss], t.model_optimizer.arena().flat.detach().clone()))
    (le, fe), (lg, fg) = results
    assert len(le) == len(lg) == 3 and le[2] > 0
    assert all(abs(x - y) <= 1e-6 * abs(y) for x, y in zip(le, lg)), (le, lg)
    assert all(np.isfinite(x) for x in le)
    assert float((fe - fg).abs().max()) <= 1e-6 * float(fe.abs().max())
