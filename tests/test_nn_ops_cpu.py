"""CPU: the float64 references of tests/nn_ops_ref.py against torch's own float64 operators, on the case lists the GPU file uses
(tests/nn_ops_cases.py).  What tests/test_nn_ops_gpu.py measures the HIP kernels against is only as good as this file says."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_ops_cases as K
import nn_ops_ref as R

F64 = torch.float64
TIGHT = 1e-12          # float64 against float64: a few hundred roundings of 1.1e-16


def close(a, b, tol=TIGHT):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol * scale, (float((a - b).abs().max()), scale)


def nchw(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ BatchNorm
def slab64(x, groups):
    """the slab of float64 sums, one row pair per tile"""
    G, m, rows, C = x.shape
    return torch.stack([x.sum(2), (x * x).sum(2)], 2).reshape(G * m, 2, C)


@pytest.mark.parametrize("case", [c for c in K.FIN_CASES if c[0] * c[1] <= 71 * 2048], ids=str)
def test_bn_finalize_ref_against_batchnorm2d(case):
    """bn_finalize_ref on the float64 sums of x, one group at a time, against nn.BatchNorm2d(double) run on the groups in order: the saved
    statistics through the output it implies, and the running statistics after all groups."""
    mtiles, C, groups, running = case
    a = K.fin_build(mtiles, C, groups)
    x = a["x"].double()
    bn = torch.nn.BatchNorm2d(C, eps=K.EPS, momentum=K.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(a["gamma"]); bn.bias.copy_(a["beta"]); bn.running_mean.copy_(a["running_mean"]); bn.running_var.copy_(a["running_var"])
    got = R.bn_finalize_ref(slab64(x, groups), a["count"], a["gamma"], a["beta"], K.EPS, K.MOMENTUM, a["running_mean"], a["running_var"], groups)
    for g in range(groups):
        xg = x[g].reshape(-1, C)
        want = bn(xg.reshape(-1, C, 1, 1)).reshape(-1, C)          # N = pixels, 1 x 1 maps
        y = R.bn_apply_ref(xg, got["scale"][g:g + 1], got["shift"][g:g + 1], None, False, 1)
        # E[x^2] - mean^2 in float64 loses (mean / std)^2 * 1.1e-16: 1e-10 on the mean / std = 1e3 channel
        cols = torch.ones(C, dtype=torch.bool)
        cols[2 if C > 2 else 0] = False
        close(y[:, cols], want[:, cols], 1e-11)
        close(y, want, 1e-7)
    close(got["running_mean"], bn.running_mean, 1e-12)
    close(got["running_var"], bn.running_var, 1e-9)
    assert int(bn.num_batches_tracked) == groups


def test_bn_finalize_ref_edges():
    """count = 1 keeps the biased variance for the running one; the constant channels clamp to variance 0 and invstd = 1 / sqrt(eps), one of
    them from a NEGATIVE raw variance; a single group leaves running statistics that two calls of one group each would."""
    a = K.fin_build(1, 16, 1, rows=1)
    r = R.bn_finalize_ref(a["slab"], 1.0, a["gamma"], a["beta"], K.EPS, K.MOMENTUM, a["running_mean"], a["running_var"], 1)
    # one sample: the variance is the float32 rounding of x^2 at most
    assert (r["var"] <= 2.0 ** -23 * r["mean"] ** 2).all() and torch.isfinite(r["running_var"]).all()
    close(r["running_var"], (1 - K.MOMENTUM) * a["running_var"].double() + K.MOMENTUM * r["var"][0])
    for mtiles in K.FIN_MTILES:
        a = K.fin_build(mtiles, 16, 2)
        r = R.bn_finalize_ref(a["slab"], a["count"], a["gamma"], a["beta"], K.EPS, K.MOMENTUM, None, None, 2)
        assert r["running_mean"] is None and r["running_var"] is None
        assert (r["var_raw"][:, 0] == 0).all() and (r["var_raw"][:, 1] < 0).all(), r["var_raw"][:, :2]
        assert (r["invstd"][:, :2] == 1.0 / np.sqrt(K.EPS)).all()
        ratio = r["mean"][:, 2].abs() * r["invstd"][:, 2]
        assert ((ratio > 500) & (ratio < 2000)).all()
    a = K.fin_build(33, 16, 2)
    both = R.bn_finalize_ref(a["slab"], a["count"], a["gamma"], a["beta"], K.EPS, K.MOMENTUM, a["running_mean"], a["running_var"], 2)
    rm, rv = a["running_mean"], a["running_var"]
    for g in range(2):
        one = R.bn_finalize_ref(a["slab"][g * 33:(g + 1) * 33], a["count"], a["gamma"], a["beta"], K.EPS, K.MOMENTUM, rm, rv, 1)
        rm, rv = one["running_mean"], one["running_var"]
    close(both["running_mean"], rm); close(both["running_var"], rv)


@pytest.mark.parametrize("case", K.BN_CASES + [K.BN_WRAP + (True, True, False, False)], ids=str)
def test_bn_apply_and_bwd_ref_against_autograd(case):
    """relu(bn(x) + residual) per group through nn.BatchNorm2d(double) and autograd against bn_apply_ref / bn_bwd_ref fed the exact float64
    statistics of x.  (One pixel per group: nn.BatchNorm2d refuses to train on it; the references are checked by their own algebra.)"""
    C, pix, groups, relu, _, _, _ = case
    a = K.bn_build(C, pix, groups)
    x, dy, res = a["x"].double(), a["dy"].double(), a["res"].double()
    xg = x.reshape(groups, pix, C)
    mean = xg.mean(1)
    invstd = 1.0 / torch.sqrt((xg * xg).mean(1) - mean * mean + K.EPS)
    gamma, beta = a["gamma"].double(), a["beta"].double()
    y = R.bn_apply_ref(x, gamma * invstd, beta - mean * gamma * invstd, res, relu, groups)
    r = R.bn_bwd_ref(dy, y, x, gamma, mean, invstd, relu, groups)
    if pix == 1:
        close(r["sums"][:, 0], (dy * ((y > 0) if relu else 1)).reshape(groups, C)); assert float(r["sums"][:, 1].abs().max()) < 1e-9
        assert float(r["dx"].abs().max()) < 1e-9
        return
    bn = torch.nn.BatchNorm2d(C, eps=K.EPS).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    xs = [xg[g].clone().requires_grad_() for g in range(groups)]
    rs = res.reshape(groups, pix, C).clone().requires_grad_()
    ys = []
    for g in range(groups):
        o = bn(xs[g].reshape(pix, C, 1, 1)).reshape(pix, C) + rs[g]          # N = pixels, 1 x 1 maps
        ys.append(torch.relu(o) if relu else o)
    want = torch.cat(ys)
    close(y, want, 1e-9)
    want.backward(dy)
    # 1e-9: the mask is taken from y, and a y within 1e-13 of 0 does not occur in these inputs; float64 BatchNorm differs by summation order
    close(r["dx"], torch.cat([t.grad for t in xs]), 1e-9)
    close(r["dres"], rs.grad.reshape(-1, C))
    close(r["dgamma"], bn.weight.grad, 1e-9)
    close(r["dbeta"], bn.bias.grad, 1e-10)
    assert r["sums"].shape == (groups, 2, C)
    close(r["sums"].sum(0), torch.stack([r["dbeta"], r["dgamma"]]))


# ------------------------------------------------------------------------------------------------ BatchNorm, eval mode
@pytest.mark.parametrize("case", K.EVAL_CASES, ids=str)
def test_bn_eval_coeffs_ref_against_batchnorm2d(case):
    """x * scale + shift of bn_eval_coeffs_ref equals nn.BatchNorm2d(C).double().eval() holding the case's parameters and buffers, on a random
    map whose channels sit around their running mean (so the two terms of the output are of one size: the cancelling case for shift)."""
    C, kind, eps = case
    a = K.eval_build(C, kind, eps)
    bn = torch.nn.BatchNorm2d(C, eps=eps).double().eval()
    with torch.no_grad():
        bn.weight.copy_(a["gamma"]); bn.bias.copy_(a["beta"]); bn.running_mean.copy_(a["running_mean"]); bn.running_var.copy_(a["running_var"])
    g = K.gen(C, 31)
    x = a["running_mean"].double().view(1, C, 1, 1) + torch.sqrt(a["running_var"].double() + eps).view(1, C, 1, 1) * torch.randn(2, C, 3, 5, generator=g, dtype=F64)
    scale, shift = R.bn_eval_coeffs_ref(a["gamma"].double(), a["beta"].double(), a["running_mean"].double(), a["running_var"].double(), eps)
    with torch.no_grad():
        want = bn(x)
    got = x * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1)
    # per element against the size of the TERMS (x * scale and shift are up to 3e5 where the output is O(1))
    mag = (x * scale.view(1, C, 1, 1)).abs() + shift.abs().view(1, C, 1, 1) + 1e-300
    assert float(((got - want).abs() / mag).max()) <= 1e-13
    # and on a plain random map, against the largest output.  Not where the case plants a beta that cancels mean * scale (3e5) down to O(10):
    # there float64 itself keeps 3e5 * 1.1e-16 = 3e-11 of the terms, 8e-12 measured against an output of 70, and the rule above is the one that holds
    if kind not in ("cancel", "mixed"):
        x = torch.randn(2, C, 3, 5, generator=g, dtype=F64)
        with torch.no_grad():
            close(x * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1), bn(x), 1e-13)
    assert int(bn.num_batches_tracked) == 0


def test_bn_eval_cases_cover_what_they_name():
    """Block edge, every variance and eps, gamma zeros and negatives, |running_mean| towards 1e3 against a small beta and against a cancelling one."""
    assert {1, 63, 64, 65, 2048} <= set(K.EVAL_C) and set(K.EVAL_EPS) == {float(np.float32(1e-5)), float(np.float32(1e-3))}
    for C in (65, 2048):
        for eps in K.EVAL_EPS:
            m = K.eval_build(C, "mixed", eps)
            assert {float(v) for v in m["running_var"]} == {float(np.float32(v)) for v in K.EVAL_VARS}
            assert (m["gamma"] == 0).any() and (m["gamma"] < 0).any() and (m["gamma"] > 0).any()
            for kind in ("mixed", "cancel"):
                a = K.eval_build(C, kind, eps)
                sc, sh = R.bn_eval_coeffs_ref(a["gamma"].double(), a["beta"].double(), a["running_mean"].double(), a["running_var"].double(), eps)
                terms = a["beta"].double().abs() + (a["running_mean"].double() * sc).abs()
                live = terms > 0
                assert float(a["running_mean"].abs().max()) > 900 and float((sh.abs() / terms)[live].min()) < 1e-3      # shift cancels to 1e-4 of its terms
                assert bool(((a["running_mean"].abs() > 250) & (a["beta"].abs() < 1e-2)).any())
    for v in K.EVAL_VARS:
        assert bool((K.eval_build(64, "var=%g" % v, K.EVAL_EPS[0])["running_var"] == float(np.float32(v))).all())


def test_bn_eval_cases_have_teeth():
    """The bound the GPU test applies (test_nn_ops_gpu.check_eval_coeffs) passes for the float32 restatement and for one that contracts
    beta - mean * scale into a single rounding, and FAILS on at least one case for each wrong definition: eps dropped, running_var read as a
    standard deviation, the sign of mean * scale flipped.  Checked here so that it is known without a GPU."""
    from test_nn_ops_gpu import check_eval_coeffs

    def right(g, b, m, v, eps):
        return R.bn_eval_coeffs_ref(g, b, m, v, eps)

    def contracted(g, b, m, v, eps):
        sc = g / torch.sqrt(v + eps)
        return sc, (b.double() - m.double() * sc.double()).float()          # one rounding for the product and the difference together

    def no_eps(g, b, m, v, eps):
        return R.bn_eval_coeffs_ref(g, b, m, v, 0.0)

    def var_as_std(g, b, m, v, eps):
        sc = g / (v + eps)
        return sc, b - m * sc

    def sign_flipped(g, b, m, v, eps):
        sc = g / torch.sqrt(v + eps)
        return sc, b + m * sc

    def failures(f):
        bad = []
        for C, kind, eps in K.EVAL_CASES:
            if C > 512:
                continue
            a = K.eval_build(C, kind, eps)
            sc, sh = f(a["gamma"], a["beta"], a["running_mean"], a["running_var"], eps)
            try:
                check_eval_coeffs(a, eps, sc, sh)
            except AssertionError:
                bad.append((C, kind, eps))
        return bad

    assert failures(right) == [] and failures(contracted) == []
    for wrong in (no_eps, var_as_std, sign_flipped):
        bad = failures(wrong)
        assert bad, wrong.__name__
        print("%-12s fails %d of the cases, e.g. %s" % (wrong.__name__, len(bad), bad[0]))


# ------------------------------------------------------------------------------------------------ max-pool
def taps_from_flat(idx, H, W):
    """torch's flat input index (iy * W + ix, NCHW) -> tap ky * 3 + kx of the window of its output position"""
    B, C, Ho, Wo = idx.shape
    oy = torch.arange(Ho)[None, None, :, None]
    ox = torch.arange(Wo)[None, None, None, :]
    return ((idx // W - (2 * oy - 1)) * 3 + (idx % W - (2 * ox - 1))).permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", K.POOL_CASES + [(1, 65, 67, 4)], ids=str)
def test_maxpool_ref_against_torch(case):
    B, H, W, C = case
    x, dy, dx0 = K.pool_build(B, H, W, C)
    assert C == 4 or (torch.isnan(x).any() and torch.isinf(x).any())
    xd = x.double()
    want, idx = F.max_pool2d(xd.permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    got, tap = R.maxpool_ref(xd)
    want = want.permute(0, 2, 3, 1)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, 7.0), torch.nan_to_num(want, 7.0))
    assert torch.equal(tap.long(), taps_from_flat(idx, H, W))
    assert (got[..., 1] == float("-inf")).all() and (tap[..., 1].long() == taps_from_flat(idx, H, W)[..., 1]).all()
    # the float32 evaluation selects the same elements
    got32, tap32 = R.maxpool_ref(x)
    assert torch.equal(tap32, tap) and torch.equal(got32.view(torch.int32), got.float().view(torch.int32))
    # adjoint: <P x, y> = <x, P^T y> for the linear map the taps define (on a finite x of its own), plain and accumulating
    xf = torch.randn(x.shape, dtype=F64, generator=K.gen(B, H, W, C))
    sel = R.maxpool_bwd_ref(torch.ones_like(dy.double()), tap, x.shape)          # how often each input was selected
    back = R.maxpool_bwd_ref(dy.double(), tap, x.shape)
    b, oy, ox, c = torch.meshgrid(torch.arange(B), torch.arange(got.shape[1]), torch.arange(got.shape[2]), torch.arange(C), indexing="ij")
    picked = xf[b, 2 * oy - 1 + tap.long() // 3, 2 * ox - 1 + tap.long() % 3, c]
    assert abs(float((picked * dy).sum() - (xf * back).sum())) <= 1e-12 * float((xf * back).abs().sum() + 1)
    assert float(sel.sum()) == dy.numel()
    close(R.maxpool_bwd_ref(dy.double(), tap, x.shape, dx0.double()), back + dx0.double())
    # and against autograd where the input is finite
    xr = torch.relu(xf).requires_grad_()
    yr = F.max_pool2d(xr.permute(0, 3, 1, 2), 3, 2, 1)
    yr.backward(dy.double().permute(0, 3, 1, 2))
    close(R.maxpool_bwd_ref(dy.double(), R.maxpool_ref(xr.detach())[1], x.shape), xr.grad)


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("case", [c for c in K.ADAM_CASES if c[0] <= K.ADAM_GRID + 1], ids=str)
def test_adam_ref_against_torch(case):
    n, first, scale = case
    p, grads, m, v = K.adam_build(n, first)
    ref = torch.nn.Parameter(p.double())
    opt = torch.optim.Adam([ref], lr=K.ADAM_LR, betas=(K.ADAM_B1, K.ADAM_B2), eps=K.ADAM_EPS, foreach=False)
    opt.state[ref] = {"step": torch.tensor(float(first - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    pp, mm, vv = p.double(), m.double(), v.double()
    for k in range(K.ADAM_STEPS):
        ref.grad = grads[k].double() * scale
        opt.step()
        pp, mm, vv = R.adam_ref(pp, grads[k].double(), mm, vv, K.ADAM_LR, K.ADAM_B1, K.ADAM_B2, K.ADAM_EPS, first + k, scale)
    close(pp, ref.detach(), 1e-13)
    close(mm, opt.state[ref]["exp_avg"]); close(vv, opt.state[ref]["exp_avg_sq"])
    z = K.adam_zero_block(n)
    assert torch.equal(pp[z], p.double()[z]) and torch.isfinite(pp).all()
    assert int(opt.state[ref]["step"]) == first - 1 + K.ADAM_STEPS


# ------------------------------------------------------------------------------------------------ layout, elementwise, helpers
@pytest.mark.parametrize("bhw", K.LAYOUT_BHW, ids=str)
def test_layout_refs(bhw):
    B, H, W = bhw
    for C, Cp, choff in K.NCHW_TO_NHWC:
        src, dst = K.randn((B, C, H, W), B, C, 1).double(), K.randn((B, H, W, Cp), B, Cp, 2).double()
        out = R.nchw_to_nhwc_ref(src, dst, choff)
        keep = torch.ones(Cp, dtype=torch.bool); keep[choff:choff + C] = False
        assert torch.equal(out[..., keep], dst[..., keep])
        assert torch.equal(R.nhwc_to_nchw_ref(out, C, choff), src)
    for C, Cp in K.NCHW3:
        s = [K.randn((B, C, H, W), B, C, i).double() for i in range(3)]
        out = R.nchw3_to_nhwc_ref(s[0], s[1], s[2], Cp)
        assert torch.equal(out.permute(0, 3, 1, 2)[:, :3 * C], torch.cat(s, 1)) and float(out[..., 3 * C:].abs().sum()) == 0


@pytest.mark.parametrize("act", K.ACTS)
def test_act_bwd_ref_against_autograd(act):
    z = torch.randn(257, dtype=F64, generator=K.gen(act)).requires_grad_()
    y = [lambda t: t, torch.relu, F.elu, torch.sigmoid][act](z)
    dy = torch.randn(257, dtype=F64, generator=K.gen(act, 1))
    y.backward(dy)
    close(R.act_bwd_ref(dy, y.detach(), act), z.grad)
    dx0 = torch.randn(257, dtype=F64, generator=K.gen(act, 2))
    close(R.act_bwd_ref(dy, y.detach(), act, dx0), z.grad + dx0)
    dst = torch.full((257, 4), 3.0, dtype=F64)
    out = R.act_bwd_strided_ref(dy, y.detach(), act, dst, 4)
    close(out[:, 0], z.grad); assert (out[:, 1:] == 3.0).all()


def inner(a, b):
    return float((a.double() * b.double()).sum())


def test_adjoint_refs():
    """<A x, y> = <x, A^T y> in float64 for each forward / adjoint pair, and the forwards against torch."""
    for B, H, W, C in K.SPATIAL_MEAN:
        x, y = K.randn((B, H, W, C), B, H, 1).double(), K.randn((B, C), B, C, 2).double()
        close(R.spatial_mean_ref(x, 0.06), 0.06 * x.mean((1, 2)))
        assert abs(inner(R.spatial_mean_ref(x, 0.06), y) - inner(x, R.spatial_mean_bwd_ref(y, x.shape, 0.06))) < 1e-12 * (1 + x.abs().sum())
    for P, h, w in K.UPSAMPLE:
        x, y = K.randn((P, h, w), P, h, 3).double(), K.randn((P, 2 * h, 2 * w), P, w, 4).double()
        assert torch.equal(R.upsample_nearest2x_ref(x), F.interpolate(x[None], scale_factor=2, mode="nearest")[0])
        assert abs(inner(R.upsample_nearest2x_ref(x), y) - inner(x, R.upsample_nearest2x_bwd_ref(y))) < 1e-12 * (1 + y.abs().sum())
    for B, Hl, Wl, C in K.ADJ_FOLD:
        x, t = K.randn((B, Hl, Wl, C), B, Hl, 5).double(), K.randn((B, Hl + 2, Wl + 2, C), B, Wl, 6).double()
        rep = R.replicate_ring_ref(x)
        assert torch.equal(rep, F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1))
        assert abs(inner(rep, t) - inner(x, R.upsample_adj_fold_ref(t, None, 0, None))) < 1e-12 * (1 + t.abs().sum())
        for act in K.ACTS:
            aux, add = K.act_output((B, Hl, Wl, C), act, B, C, act).double(), K.randn((B, Hl, Wl, C), B, C, 8).double()
            close(R.upsample_adj_fold_ref(t, aux, act, add), R.upsample_adj_fold_ref(t, None, 0, None) * R.dact_ref(aux, act) + add)
    for n, Cs, soff, Cd, doff, C in K.COPY_CHANNELS:
        src, dst = K.randn((n, Cs), n, Cs, 1).double(), K.randn((n, Cd), n, Cd, 2).double()
        out = R.copy_channels_ref(src, soff, dst, doff, C, False)
        assert torch.equal(out[:, doff:doff + C], src[:, soff:soff + C])
        acc = R.copy_channels_ref(src, soff, dst, doff, C, True)
        close(acc - dst, out - R.copy_channels_ref(torch.zeros_like(src), soff, dst, doff, C, False))
        # slice and concat are each other's adjoint
        y = K.randn((n, C), n, C, 3).double()
        back = R.copy_channels_ref(y, 0, torch.zeros_like(src), soff, C, False)
        assert abs(inner(src[:, soff:soff + C], y) - inner(src, back)) < 1e-12 * (1 + src.abs().sum())
    x = K.randn((129, 96), 1).double()
    close(R.colsum_ref(x), x.t() @ torch.ones(129, dtype=F64)); close(R.colsum_ref(x, x[0]), x.sum(0) + x[0])


def test_case_lists_reach_the_paths_they_name():
    assert [K.fin_slices(m) for m in K.FIN_MTILES if m > 64] == [9, 9, 33, 128, 114]
    for C, pix, groups, *_ in K.BN_CASES:
        assert C % 4 == 0 and (256 % (C // 4) == 0 or (C // 4) % 256 == 0)
    blocks = lambda pix: min(-(-pix // 32), 1024)
    per = lambda pix: -(-pix // blocks(pix))
    assert per(70) > 3 * (256 // 64) and per(51300) > 3 * (256 // 16) and blocks(32769) == 1024 and per(32769) == 33
    C, pix, groups = K.BN_WRAP
    n4, trip = groups * pix * C // 4, 4096 * 256
    assert trip < (groups - 1) * pix * C // 4 < n4
    B, H, W, C = K.POOL_WRAP
    assert B * R.pool_out(H) * R.pool_out(W) * C // 4 > trip
    assert K.LAYOUT_WRAP[0] * K.LAYOUT_WRAP[1] * K.LAYOUT_WRAP[2] > trip and K.ELEMENTWISE_N[-1] > trip
    assert {s for _, f, s in K.ADAM_CASES if f == 1} == set(K.ADAM_SCALES) == {s for _, f, s in K.ADAM_CASES if f == 1000}
    a, b = torch.tensor([1.0, -0.0, 1.0]), torch.tensor([np.float32(1.0) + np.float32(2 ** -23), 0.0, 1.0])
    assert K.ulp_distance(a, b).tolist() == [1, 0, 0]
