"""GPU: the kernels of csrc/nn_ops.hip (BatchNorm finalize / eval coefficients / apply / backward, max-pool, activation backward, layout, fused Adam) and the
helpers of csrc/aux_ops.hip, each on its own through the C ABI, against the float64 definitions of tests/nn_ops_ref.py on the cases of
tests/nn_ops_cases.py (tests/test_nn_ops_cpu.py checks those definitions against torch).

Rules of this file.
  * Every buffer a kernel WRITES is a window of a larger allocation whose bands before and after hold a sentinel bit pattern (Guarded);
    call() asserts the bands after every launch, so a ragged-tail store shows without faulting.  The window itself starts as sentinels
    (a NaN pattern) too: an element the kernel skipped fails the comparison.
  * Pure copies and selections are compared bit for bit.
  * Everything else obeys the three-column rule (tests/arbiter.py) element by element, and for reductions entry by entry (one row per
    channel): with err(v) = |v - float64| / mag, mag the SUM OF THE ABSOLUTE TERMS of the output (not the possibly cancelling result),
        err(HIP)  <=  2 * max(err(the same formula in plain float32 torch on the CPU), ops * 2^-24).
    2^-24 is one float32 rounding (half a step) relative to mag; `ops` is the number of roundings on the longest path of the KERNEL'S
    evaluation, counted in the docstring of each test, so the floor alone is a bound a correct kernel always meets: nothing here was fitted
    to what the kernels return.
"""
import copy
import math

import numpy as np
import pytest
import torch

import nn_ops_cases as K
import nn_ops_ref as R
from guarded import SENT8, SENT32, Guarded, P, bits, same_bits  # noqa: F401  (the window helpers, shared with the conv modules)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
E_INVALID, E_WORKSPACE = -1, -2
F32 = torch.float32


def call(name, *args, outs=(), expect=0):
    """launch on the current stream, wait, check the return code and the guard bands of every output"""
    from mcav import lib as L
    from mcav import nn, tape  # noqa: F401  (register the signatures)
    rc = getattr(L.lib(), name)(*args, L.stream())
    torch.cuda.synchronize()
    assert rc == expect, "%s returned %d, expected %d" % (name, rc, expect)
    for o in outs:
        assert o.intact(), "%s wrote outside its output" % name
    return rc


def dev(t):
    return t.contiguous().to(DEV)


def three_col(name, hip, cpu32, ref64, mag, ops):
    """the rule of the module docstring, entry by entry; prints the three columns before it asserts"""
    hip, cpu32, ref64 = hip.detach().cpu().double(), cpu32.detach().double(), ref64.detach().double()
    assert hip.shape == ref64.shape == cpu32.shape, (name, hip.shape, cpu32.shape, ref64.shape)
    mag = mag.detach().double().expand_as(ref64).clamp_min(1e-300)
    e_hip, e_cpu = (hip - ref64).abs() / mag, (cpu32 - ref64).abs() / mag
    allow = 2.0 * e_cpu.clamp_min(ops * U)
    print("  %-22s worst |HIP-fp64| %.3e  |CPUfp32-fp64| %.3e  floor %.3e (%d ops)" % (name, float(e_hip.max()) if e_hip.numel() else 0.0,
                                                                                   float(e_cpu.max()) if e_cpu.numel() else 0.0, ops * U, ops))
    bad = ~(e_hip <= allow)                       # (a NaN fails)
    assert not bool(bad.any()), "%s: %d entries beyond 2 x max(CPU fp32, %d roundings); first %s: HIP %.9g fp64 %.9g err %.3e allowed %.3e" % (
        name, int(bad.sum()), ops, tuple(int(v) for v in bad.nonzero()[0]), float(hip[bad][0]), float(ref64[bad][0]), float(e_hip[bad][0]),
        float(allow[bad][0]))


def within_one_ulp(name, hip, want64):
    """hip is the float32 rounding of the float64 value, give or take one step (another summation order in double moves the last bit)"""
    d = K.ulp_distance(hip.detach().cpu(), want64.float())
    assert int(d.max()) <= 1, "%s: %d entries more than one float32 step from the float64 value (worst %d steps)" % (name, int((d > 1).sum()), int(d.max()))


# ================================================================================================ 3.2 mcav_bn_finalize
def finalize_workspace(mtiles, C, groups):
    from mcav import lib as L
    from mcav import nn  # noqa: F401
    nbytes = L.lib().mcav_bn_finalize_workspace_bytes(mtiles, C, groups)
    assert (nbytes > 0) == (mtiles > 64)
    return L.workspace(nbytes, torch.device(DEV, torch.cuda.current_device()), "bn_fin", zero=True) if nbytes else None      # the product's own cached one


def run_finalize(a, mtiles, C, groups, running):
    o = dict(scale=Guarded((groups, C)), shift=Guarded((groups, C)), mean=Guarded((groups, C)), invstd=Guarded((groups, C)))
    o["running_mean"] = Guarded((C,), init=a["running_mean"]) if running else None
    o["running_var"] = Guarded((C,), init=a["running_var"]) if running else None
    ws = finalize_workspace(mtiles, C, groups)
    slab, gamma, beta = dev(a["slab"]), dev(a["gamma"]), dev(a["beta"])
    call("mcav_bn_finalize", P(slab), mtiles, C, a["count"], P(gamma), P(beta), K.EPS, K.MOMENTUM, P(o["running_mean"]), P(o["running_var"]),
         P(o["scale"]), P(o["shift"]), P(o["mean"]), P(o["invstd"]), groups, P(ws), ws.numel() if ws is not None else 0,
         outs=[v for v in o.values() if v is not None])
    if ws is not None:          # the tickets (1 KB at the head of the workspace) are back at zero for the next launch
        assert bool((ws[:1024].view(torch.int32) == 0).all()), "completion tickets left non-zero"
    return o


def check_finalize(a, o, groups, running):
    """mean, invstd: the float32 rounding of the float64 value of the SAME slab, +- 1 step.
    scale = gamma * invstd: invstd within one step (2 roundings) + the product = 3.
    shift = beta - mean * scale, mag |beta| + |mean * scale|: mean (2) + scale (3) + product (1) on the second term, + the subtraction = 7.
    running = (1 - m) * running + m * stat per group, mag the same expression on absolute values: per group (1 - m) and its product (2) on
    one term, the statistic within one step and its product (3) on the other, + the addition: 4 per group at most."""
    gamma, beta = a["gamma"], a["beta"]
    r = R.bn_finalize_ref(a["slab"], a["count"], gamma, beta, K.EPS, K.MOMENTUM, a["running_mean"] if running else None,
                          a["running_var"] if running else None, groups)
    within_one_ulp("mean", o["mean"].t, r["mean"])
    within_one_ulp("invstd", o["invstd"].t, r["invstd"])
    mean32, inv32 = r["mean"].float(), r["invstd"].float()
    sc32 = gamma[None] * inv32
    three_col("scale", o["scale"].t, sc32, r["scale"], r["scale"].abs(), 3)
    three_col("shift", o["shift"].t, beta[None] - mean32 * sc32, r["shift"], beta.double().abs()[None] + (r["mean"] * r["scale"]).abs(), 7)
    if running:
        count = a["count"]
        unb = r["var"] * count / (count - 1.0) if count > 1 else r["var"]
        m32, one_m = torch.tensor(K.MOMENTUM, dtype=F32), torch.tensor(1.0, dtype=F32) - torch.tensor(K.MOMENTUM, dtype=F32)
        rm32, rv32 = a["running_mean"].clone(), a["running_var"].clone()
        am, av = a["running_mean"].double().abs(), a["running_var"].double().abs()
        for g in range(groups):
            rm32, rv32 = one_m * rm32 + m32 * mean32[g], one_m * rv32 + m32 * unb[g].float()
            am, av = (1 - K.MOMENTUM) * am + K.MOMENTUM * r["mean"][g].abs(), (1 - K.MOMENTUM) * av + K.MOMENTUM * unb[g].abs()
        three_col("running_mean", o["running_mean"].t, rm32, r["running_mean"], am, 4 * groups)
        three_col("running_var", o["running_var"].t, rv32, r["running_var"], av, 4 * groups)
    return r


@pytest.mark.parametrize("case", K.FIN_CASES, ids=str)
def test_bn_finalize(case):
    mtiles, C, groups, running = case
    a = K.fin_build(mtiles, C, groups)
    r = check_finalize(a, run_finalize(a, mtiles, C, groups, running), groups, running)
    # the edges every slab carries: a constant channel (variance exactly 0), one whose raw variance is NEGATIVE (the clamp), mean / std = 1e3
    if C > 2:
        assert (r["var_raw"][:, 0] == 0).all() and (r["var_raw"][:, 1] < 0).all()
        assert (r["invstd"][:, :2] == 1.0 / math.sqrt(K.EPS)).all()


def test_bn_finalize_workspace_reuse_on_one_stream():
    """One cached workspace, one stream, layers of different widths in turn: a ticket word that another layer's partial sums had covered, or
    that a launch left non-zero, makes the next launch finish early or never (the failure the comment in mcav_bn_finalize_workspace_bytes
    records).  Every call is checked against the reference, twice round."""
    seq = [(257, 2048, 1), (1025, 64, 2), (257, 2048, 2), (71, 128, 3)]
    for _ in range(2):
        for i, (mtiles, C, groups) in enumerate(seq):
            a = K.fin_build(mtiles, C, groups, seed=i)
            check_finalize(a, run_finalize(a, mtiles, C, groups, True), groups, True)


@pytest.mark.parametrize("groups", (1, 2))
def test_bn_finalize_count_one(groups):
    a = K.fin_build(1, 64, groups, rows=1)
    assert a["count"] == 1.0
    r = check_finalize(a, run_finalize(a, 1, 64, groups, True), groups, True)
    assert torch.isfinite(r["running_var"]).all()


def test_bn_finalize_refuses_half_a_pair_of_running_statistics():
    a = K.fin_build(33, 64, 1)
    slab, gamma, beta = dev(a["slab"]), dev(a["gamma"]), dev(a["beta"])
    for which in (0, 1):
        outs = [Guarded((1, 64)) for _ in range(4)]
        run = Guarded((64,))
        call("mcav_bn_finalize", P(slab), 33, 64, a["count"], P(gamma), P(beta), K.EPS, K.MOMENTUM, P(run) if which == 0 else None,
             P(run) if which == 1 else None, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), 1, None, 0, outs=outs + [run], expect=E_INVALID)
        assert all(o.untouched() for o in outs + [run])
    outs = [Guarded((1, 64)) for _ in range(4)]        # and a many-tile call without its workspace
    call("mcav_bn_finalize", P(dev(K.fin_build(65, 64, 1)["slab"])), 65, 64, 130.0, P(gamma), P(beta), K.EPS, K.MOMENTUM, None, None,
         P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), 1, None, 0, outs=outs, expect=E_WORKSPACE)
    assert all(o.untouched() for o in outs)


def test_bn_train_coeffs_wrapper_and_counter():
    """mcav.nn.bn_train_coeffs (the call the networks make) gives what the ABI gives, updates the holder's running statistics, and
    num_batches_tracked advances by `groups` once flush_bn_counters() has run."""
    from mcav import nn as N
    from mcav.holders import BNParams
    mtiles, C, groups = 71, 96, 3
    a = K.fin_build(mtiles, C, groups)
    bn = BNParams(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(a["gamma"]); bn.bias.copy_(a["beta"]); bn.running_mean.copy_(a["running_mean"]); bn.running_var.copy_(a["running_var"])
    N.flush_bn_counters()
    st = N.bn_train_coeffs(bn, dev(a["slab"]), a["count"], groups)
    torch.cuda.synchronize()
    o = run_finalize(a, mtiles, C, groups, True)
    for name, t in (("scale", st.scale), ("shift", st.shift), ("mean", st.mean), ("invstd", st.invstd),
                    ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
        assert same_bits(t, o[name].t), name
    assert st.groups == groups and int(bn.num_batches_tracked) == 0
    N.flush_bn_counters()
    assert int(bn.num_batches_tracked) == groups


# ================================================================================================ mcav_bn_eval_coeffs (eval mode: scale / shift from the running statistics)
def check_eval_coeffs(a, eps, scale, shift):
    """scale = gamma / sqrt(running_var + eps), mag |scale|: the addition, the root, the division = 3 roundings.
    shift = beta - running_mean * scale, mag |beta| + |running_mean * scale| (NOT the possibly cancelling difference): scale's 3, the product,
    the subtraction and one to spare for a contracted multiply-add's other rounding = 6.  No bit equality: the device may contract.
    (Also called by tests/test_nn_ops_cpu.py on deliberately wrong restatements: the cases must make this raise for each of them.)"""
    gamma, beta, rm, rv = a["gamma"], a["beta"], a["running_mean"], a["running_var"]
    sc64, sh64 = R.bn_eval_coeffs_ref(gamma.double(), beta.double(), rm.double(), rv.double(), eps)
    sc32, sh32 = R.bn_eval_coeffs_ref(gamma, beta, rm, rv, eps)
    three_col("eval scale", scale, sc32, sc64, sc64.abs(), 3)
    three_col("eval shift", shift, sh32, sh64, beta.double().abs() + (rm.double() * sc64).abs(), 6)


@pytest.mark.parametrize("case", K.EVAL_CASES, ids=str)
def test_bn_eval_coeffs(case):
    """Every channel written (the windows start as sentinels: a skipped one fails as NaN), nothing outside them, on both sides of the 64-thread
    block edge and at ResNet-50's widest layer; values under the three-column rule of check_eval_coeffs."""
    C, kind, eps = case
    a = K.eval_build(C, kind, eps)
    scale, shift = Guarded((C,)), Guarded((C,))
    gamma, beta, rm, rv = (dev(a[k]) for k in ("gamma", "beta", "running_mean", "running_var"))       # (named: alive until the launch is done)
    call("mcav_bn_eval_coeffs", P(gamma), P(beta), P(rm), P(rv), eps, C, P(scale), P(shift), outs=[scale, shift])
    assert bool(torch.isfinite(scale.t).all()) and bool(torch.isfinite(shift.t).all())
    check_eval_coeffs(a, eps, scale.t, shift.t)


def test_bn_eval_coeffs_wrapper():
    """mcav.nn.bn_eval_coeffs (the call conv_bn / tape.batchnorm make in eval mode) reads the holder's buffers as they are NOW (loaded ones too),
    gives what the ABI gives, keeps no batch statistics (mean / invstd None: what the backward's refusal looks at) and touches no counter."""
    from mcav import nn as N
    from mcav.holders import BNParams
    C, eps = 96, K.EVAL_EPS[0]
    a = K.eval_build(C, "mixed", eps)
    bn = BNParams(C).to(DEV)
    assert float(np.float32(bn.eps)) == eps
    bn.load_state_dict(dict(weight=a["gamma"], bias=a["beta"], running_mean=a["running_mean"], running_var=a["running_var"],
                            num_batches_tracked=torch.tensor(7)))
    N.flush_bn_counters()
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    st = N.bn_eval_coeffs(bn)
    torch.cuda.synchronize()
    check_eval_coeffs(a, eps, st.scale, st.shift)
    assert st.mean is None and st.invstd is None and st.groups == 1 and not N._NBT_PENDING
    assert all(torch.equal(v, before[k]) for k, v in bn.state_dict().items()) and int(bn.num_batches_tracked) == 7


def test_bn_eval_coeffs_refusals():
    """A NULL for any of the six pointers, or C <= 0: MCAV_E_INVALID before any launch, both windows still all sentinels."""
    C, eps = 65, K.EVAL_EPS[0]
    a = K.eval_build(C, "mixed", eps)
    ins = [dev(a[k]) for k in ("gamma", "beta", "running_mean", "running_var")]
    for null in range(6):
        scale, shift = Guarded((C,)), Guarded((C,))
        ptrs = [P(t) for t in ins] + [P(scale), P(shift)]
        ptrs[null] = None
        call("mcav_bn_eval_coeffs", *ptrs[:4], eps, C, *ptrs[4:], outs=[scale, shift], expect=E_INVALID)
        assert scale.untouched() and shift.untouched(), null
    for bad_c in (0, -1, -64):
        scale, shift = Guarded((C,)), Guarded((C,))
        call("mcav_bn_eval_coeffs", *[P(t) for t in ins], eps, bad_c, P(scale), P(shift), outs=[scale, shift], expect=E_INVALID)
        assert scale.untouched() and shift.untouched(), bad_c


# ================================================================================================ 3.3 apply, backward reduce + finalize, backward apply
def reduce_adds(C, pix):
    """float32 additions on the longest path of one partial sum of bn_bwd_reduce_kernel: a lane adds ceil(per / PL) pixels, lane 0 then adds
    the PL lanes; the blocks are summed in float64"""
    blocks = min(-(-pix // 32), 1024)
    per = -(-pix // blocks)
    PL = max(1, 256 // min(C // 4, 256))
    return -(-per // PL) + PL


def run_bn_case(case, repeat=False):
    """apply: y = x * scale + shift (+ residual), ReLU; mag |x scale| + |shift| + |residual|; product, two additions: 3 roundings.
    reduce: sums[g][0][c] = sum g, mag sum |g|: reduce_adds() additions + the cast of the float64 total = adds + 1.
            sums[g][1][c] = sum g * xhat, mag sum |g xhat|: xhat is a subtraction and a product, g * xhat one more: adds + 4.
            dbeta / dgamma: the float64 sum over groups cast once (the same count), + 1 when accumulated into a non-zero gradient.
    backward apply, given the KERNEL'S sums (the second pass on its own): dx = (gamma invstd) * (g - s1/n - xhat * (s2/n)),
            mag |gamma invstd| (|g| + |s1|/n + |xhat s2|/n): 1/n, gamma * invstd, s2 * (1/n), x - mean, * invstd, the two fused
            multiply-adds, the final product, and s1 * (1/n) inside the first of them: 9.
    dres is the masked gradient itself (+0.0 where y_act <= 0, both signed zeros masked): bit for bit, also when accumulated (one IEEE addition)."""
    C, pix, groups, relu, want_dres, dres_acc, acc = case
    a = K.bn_build(C, pix, groups)
    n = groups * pix
    sc32 = a["gamma"][None] * a["invstd"]
    sh32 = a["beta"][None] - a["mean"] * sc32
    x, dy, res = a["x"], a["dy"], a["res"]
    xd, dyd, resd, gam = dev(x), dev(dy), dev(res), dev(a["gamma"])
    scd, shd, meand, invd = dev(sc32), dev(sh32), dev(a["mean"]), dev(a["invstd"])
    # ---- apply
    y = Guarded((n, C))
    call("mcav_bn_apply", P(xd), P(scd), P(shd), P(resd), 1 if relu else 0, n, C, P(y), pix, outs=[y])
    y64 = R.bn_apply_ref(x.double(), sc32.double(), sh32.double(), res.double(), relu, groups)
    y32 = R.bn_apply_ref(x, sc32, sh32, res, relu, groups)
    mag = (x.double().reshape(groups, pix, C) * sc32.double()[:, None]).abs().reshape(n, C) + sh32.double().abs().repeat_interleave(pix, 0) + res.double().abs()
    three_col("bn_apply y", y.t, y32, y64, mag, 3)
    if relu:
        assert bool((y.t >= 0).all())
    # ---- reduce + finalize
    y_act = K.plant_zeros(y.cpu().clone()) if relu else None
    yad = dev(y_act) if relu else None
    from mcav import lib as L
    wsb = L.lib().mcav_bn_bwd_workspace_bytes(n, C, groups)
    got = []
    for _ in range(2 if repeat else 1):
        ws = Guarded((wsb,), torch.uint8)
        sums = Guarded((groups, 2, C))
        dg, db = Guarded((C,), init=a["dgamma0"] if acc else None), Guarded((C,), init=a["dbeta0"] if acc else None)
        call("mcav_bn_bwd_reduce", P(dyd), P(yad), P(xd), P(meand), P(invd), int(relu), n, C, P(dg), P(db), int(acc), P(sums), groups, P(ws), wsb,
             outs=[ws, sums, dg, db])
        got.append((sums, dg, db))
    sums, dg, db = got[0]
    if repeat:
        assert all(same_bits(p.t, q.t) for p, q in zip(got[0], got[1])), "two runs of the reduction differ"
    mean64, inv64, g64 = a["mean"].double(), a["invstd"].double(), a["gamma"].double()
    r64 = R.bn_bwd_ref(dy.double(), y_act.double() if relu else None, x.double(), g64, mean64, inv64, relu, groups)
    r32 = R.bn_bwd_ref(dy, y_act, x, a["gamma"], a["mean"], a["invstd"], relu, groups)
    adds = reduce_adds(C, pix)
    three_col("sums[.,0] (sum g)", sums.t[:, 0], r32["sums"][:, 0], r64["sums"][:, 0], r64["abs1"], adds + 1)
    three_col("sums[.,1] (sum g xhat)", sums.t[:, 1], r32["sums"][:, 1], r64["sums"][:, 1], r64["abs2"], adds + 4)
    b0, g0 = (a["dbeta0"], a["dgamma0"]) if acc else (torch.zeros(C), torch.zeros(C))
    three_col("dbeta", db.t, b0 + r32["dbeta"], b0.double() + r64["dbeta"], b0.double().abs() + r64["abs1"].sum(0), adds + 1 + int(acc))
    three_col("dgamma", dg.t, g0 + r32["dgamma"], g0.double() + r64["dgamma"], g0.double().abs() + r64["abs2"].sum(0), adds + 4 + int(acc))
    # ---- backward apply, from the kernel's sums
    dx = Guarded((n, C))
    dres = Guarded((n, C), init=a["dres0"] if dres_acc else None) if want_dres else None
    call("mcav_bn_bwd_apply", P(dyd), P(yad), P(xd), P(gam), P(meand), P(invd), P(sums), int(relu), n, C, P(dx), P(dres), int(dres_acc), groups,
         outs=[dx] + ([dres] if want_dres else []))
    ks = sums.cpu()
    s64 = R.bn_bwd_ref(dy.double(), y_act.double() if relu else None, x.double(), g64, mean64, inv64, relu, groups, sums=ks.double())
    s32 = R.bn_bwd_ref(dy, y_act, x, a["gamma"], a["mean"], a["invstd"], relu, groups, sums=ks)
    gi = (g64[None] * inv64).repeat_interleave(pix, 0).abs()
    s1n, s2n = (ks[:, 0].double() / pix).repeat_interleave(pix, 0).abs(), (ks[:, 1].double() / pix).repeat_interleave(pix, 0).abs()
    three_col("bn_bwd_apply dx", dx.t, s32["dx"], s64["dx"], gi * (s64["dres"].abs() + s1n + s64["xhat"].abs() * s2n), 9)
    if want_dres:
        want = s32["dres"] if not dres_acc else a["dres0"] + s32["dres"]
        assert same_bits(dres.t, want), "dres is not the masked gradient"
        if relu:
            assert bool((s32["dres"][y_act == 0] == 0).all()) and (y_act.numel() < 4096 or bool((bits(y_act) == -2 ** 31).any()))      # +0.0 / -0.0 are masked


@pytest.mark.parametrize("case", K.BN_CASES, ids=str)
def test_bn_apply_and_backward(case):
    run_bn_case(case, repeat=case[1] in (33, 1057, 51300))


def test_bn_apply_and_backward_second_trip_of_the_grid():
    """n4 above 4096 x 256 work items with three groups: the elementwise kernels' grid-stride loops wrap, and the boundary between groups 1
    and 2 lies inside the second trip"""
    run_bn_case(K.BN_WRAP + (True, True, False, False))


@pytest.mark.parametrize("nblk", (1, 31, 33, 225, 300, 1024))
@pytest.mark.parametrize("C,groups", ((96, 1), (64, 3)))
def test_bn_bwd_finalize_on_a_given_slab(nblk, C, groups):
    """mcav_bn_bwd_finalize on its own (the entry a data gradient's statistics slab goes through): partial sums [groups][nblk][2][C] ->
    sums, dgamma, dbeta.  32 slice lanes, eight partials in flight while k + 224 < nblk (225, 300, 1024 reach that loop, with and without
    a tail).  The sums are float64 and cast once: 1 rounding on mag sum |partial|, + 1 when accumulated; any width (96: a ragged block)."""
    part = K.randn((groups, nblk, 2, C), nblk, C, groups) + 0.1
    g0, b0 = K.randn((C,), nblk, C, 1), K.randn((C,), nblk, C, 2)
    partd = dev(part)
    s64, a64 = part.double().sum(1), part.double().abs().sum(1)
    for acc in (0, 1):
        sums, dg, db = Guarded((groups, 2, C)), Guarded((C,), init=g0 if acc else None), Guarded((C,), init=b0 if acc else None)
        call("mcav_bn_bwd_finalize", P(partd), nblk, C, P(dg), P(db), acc, P(sums), groups, outs=[sums, dg, db])
        three_col("sums", sums.t, part.sum(1), s64, a64, 1)
        zero = torch.zeros(C)
        three_col("dbeta", db.t, (b0 if acc else zero) + part.sum(1)[:, 0].sum(0), (b0.double() if acc else 0) + s64[:, 0].sum(0),
                  (b0.double().abs() if acc else 0) + a64[:, 0].sum(0), 1 + acc)
        three_col("dgamma", dg.t, (g0 if acc else zero) + part.sum(1)[:, 1].sum(0), (g0.double() if acc else 0) + s64[:, 1].sum(0),
                  (g0.double().abs() if acc else 0) + a64[:, 1].sum(0), 1 + acc)


def test_bn_entries_refuse_bad_arguments():
    """MCAV_E_INVALID for C = 6 at every entry with a width, for C = 96 at the reduction (its lane split needs C/4 to divide 256), for
    n_pix % groups != 0, for relu without y_act; MCAV_E_WORKSPACE for a short workspace; outputs untouched every time."""
    from mcav import lib as L
    t = torch.ones(4096, device=DEV)
    ws = Guarded((L.lib().mcav_bn_bwd_workspace_bytes(12, 96, 2),), torch.uint8)

    def fresh():
        return [Guarded((1024,)) for _ in range(4)]
    o = fresh()
    call("mcav_bn_apply", P(t), P(t), P(t), None, 0, 12, 6, P(o[0]), 12, outs=o, expect=E_INVALID)
    for C, n, groups, relu, ya in ((6, 12, 1, 0, t), (96, 12, 1, 0, t), (64, 13, 2, 0, t), (64, 12, 1, 1, None)):
        call("mcav_bn_bwd_reduce", P(t), P(ya), P(t), P(t), P(t), relu, n, C, P(o[0]), P(o[1]), 0, P(o[2]), groups, P(ws), ws.t.numel(),
             outs=o + [ws], expect=E_INVALID)
    call("mcav_bn_bwd_reduce", P(t), P(t), P(t), P(t), P(t), 0, 12, 64, P(o[0]), P(o[1]), 0, P(o[2]), 1, P(ws), 1024, outs=o + [ws], expect=E_WORKSPACE)
    for C, n, groups, relu, ya in ((6, 12, 1, 0, t), (64, 13, 2, 0, t), (64, 12, 1, 1, None)):
        call("mcav_bn_bwd_apply", P(t), P(ya), P(t), P(t), P(t), P(t), P(t), relu, n, C, P(o[0]), P(o[1]), 0, groups, outs=o, expect=E_INVALID)
    assert all(v.untouched() for v in o + [ws])


# ================================================================================================ 3.4 statistics end to end
STAT_OFFSETS = (0.0, 1.3, 13.0)          # -> mean / std of the convolution's output of about 0, 10, 100


@pytest.mark.parametrize("offset", STAT_OFFSETS)
def test_statistics_chain_keeps_its_digits(offset):
    """conv_fwd(stats=True) -> bn_train_coeffs on a 1x1 convolution (64 -> 64, positive weights) of x = offset + noise: the chain forms
    E[y^2] - mean^2 from float32 tile sums, which loses (mean / std)^2 of its digits.  Columns, per channel, relative error of invstd against
    float64 BatchNorm of the float64 convolution: the chain; a float32 CPU evaluation of the same two-moment formula (float32 convolution,
    float32 sums over tiles of the slab's own height, float64 across tiles and after).  The CPU column is its worst channel (the two
    columns are independent rounding draws per channel).  Floor per channel: var = E[y^2] - mean^2 carries (1 + ratio^2) roundings of size
    2^-24 per rounding of E[y^2], invstd half of that; the roundings no float32 evaluation avoids are y, y^2 and a pairwise tile sum of depth
    log2(tile): ops = 2 + log2(tile)."""
    from mcav import nn as N
    from mcav.holders import BNParams
    B, H, W, C = 2, 32, 64, 64
    g = K.gen(int(offset * 10), 34)
    x = (offset + torch.randn(B, H, W, C, generator=g)).float()
    w = ((0.5 + torch.rand(C, C, 1, 1, generator=g)) / C).float()
    y64 = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double()).permute(0, 2, 3, 1).reshape(-1, C)
    mean64 = y64.mean(0)
    var64 = ((y64 - mean64) ** 2).mean(0)
    inv64 = 1.0 / torch.sqrt(var64 + K.EPS)
    ratio = mean64.abs() / var64.sqrt()
    spec = N.ConvSpec(torch.nn.Parameter(dev(w)), None, 1, 0, N.PAD_ZERO)
    y, slab = N.conv_fwd(spec, dev(x), stats=True)
    bn = BNParams(C).to(DEV)
    st = N.bn_train_coeffs(bn, slab, B * H * W)
    N.flush_bn_counters()
    torch.cuda.synchronize()
    M, mt = B * H * W, slab.shape[0]
    assert M % mt == 0
    tile = M // mt
    y32 = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w).permute(0, 2, 3, 1).reshape(mt, tile, C)
    s1 = y32.sum(1).double().sum(0)
    s2 = (y32 * y32).sum(1).double().sum(0)
    m = s1 / M
    inv_cpu = 1.0 / torch.sqrt((s2 / M - m * m).clamp_min(0) + K.EPS)
    e_hip = ((st.invstd[0].cpu().double() - inv64) / inv64).abs()
    e_cpu = ((inv_cpu - inv64) / inv64).abs()
    floor = 0.5 * (1 + ratio ** 2) * (2 + math.log2(tile)) * U
    print("  statistics chain: mean/std %.1f (tile %d): invstd error  chain %.3e (worst channel)  fp32 two-moment CPU %.3e  floor %.3e" % (
        float(ratio.mean()), tile, float(e_hip.max()), float(e_cpu.max()), float(floor.max())))
    bad = ~(e_hip <= 2.0 * torch.maximum(e_cpu.max(), floor))
    assert not bool(bad.any()), "invstd of %d channels beyond 2 x max(fp32 two-moment evaluation, floor): chain %.3e cpu %.3e floor %.3e" % (
        int(bad.sum()), float(e_hip.max()), float(e_cpu.max()), float(floor.max()))


# ================================================================================================ 3.5 max-pool
def run_pool(case):
    """forward: values and taps bit for bit (NaN payloads included).  backward: up to four windows select an input element (3 additions),
    + 1 when accumulated into dx: mag is the same scatter of |dy| (+ |dx|), 4 roundings."""
    B, H, W, C = case
    x, dy, dx0 = K.pool_build(B, H, W, C)
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    want, tap = R.maxpool_ref(x)
    y, idx = Guarded((B, Ho, Wo, C)), Guarded((B, Ho, Wo, C), torch.uint8)
    xd, dyd = dev(x), dev(dy)
    call("mcav_maxpool3s2_fwd", P(xd), B, H, W, C, P(y), P(idx), outs=[y, idx])
    assert torch.equal(idx.cpu(), tap), "%d winning taps differ" % int((idx.cpu() != tap).sum())
    assert same_bits(y.t, want)
    mag = R.maxpool_bwd_ref(dy.double().abs(), tap, x.shape)
    for acc in (False, True):
        dx = Guarded((B, H, W, C), init=dx0 if acc else None)
        call("mcav_maxpool3s2_bwd", P(dyd), P(idx), B, H, W, C, P(dx), int(acc), outs=[dx])
        three_col("maxpool_bwd acc=%d" % acc, dx.t, R.maxpool_bwd_ref(dy, tap, x.shape, dx0 if acc else None),
                  R.maxpool_bwd_ref(dy.double(), tap, x.shape, dx0.double() if acc else None), mag + (dx0.double().abs() if acc else 0), 4)


@pytest.mark.parametrize("case", K.POOL_CASES, ids=str)
def test_maxpool(case):
    run_pool(case)


def test_maxpool_second_trip_of_the_grid():
    run_pool(K.POOL_WRAP)


# ================================================================================================ 3.6 Adam
def adam_columns(p0, g, m0, v0, step, scale, lr=K.ADAM_LR):
    """-> (float64 reference, torch.optim.Adam(foreach=False) in float32, mags) of ONE update from the given float32 state"""
    r64 = R.adam_ref(p0.double(), g.double(), m0.double(), v0.double(), lr, K.ADAM_B1, K.ADAM_B2, K.ADAM_EPS, step, scale)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([par], lr=lr, betas=(K.ADAM_B1, K.ADAM_B2), eps=K.ADAM_EPS, foreach=False)
    opt.state[par] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    par.grad = g * scale                     # (exact: the scales are powers of two)
    opt.step()
    gr = (g.double() * scale).abs()
    mag_m = m0.double().abs() + (gr + m0.double().abs()) * (1 - K.ADAM_B1)
    mag_v = K.ADAM_B2 * v0.double() + (1 - K.ADAM_B2) * gr * gr
    denom = torch.sqrt(r64[2]) / math.sqrt(1 - K.ADAM_B2 ** step) + K.ADAM_EPS
    mag_p = p0.double().abs() + lr / (1 - K.ADAM_B1 ** step) * mag_m / denom
    return r64, (par.detach(), opt.state[par]["exp_avg"], opt.state[par]["exp_avg_sq"]), (mag_p, mag_m, mag_v)


@pytest.mark.parametrize("case", K.ADAM_CASES, ids=str)
def test_adam_step(case):
    """mcav_adam_step, ADAM_STEPS updates; every update is measured on its own, from the state the kernel itself left (so no bound has to
    cover the drift of two float32 trajectories), against float64 Adam on the float32 scalars the ABI receives.
    m = m + (g s - m)(1 - b1), mag |m| + (|g s| + |m|)(1 - b1): g s, the subtraction, the product, the addition: 4.
    v = b2 v + (1 - b2)(g s)^2, all terms positive: g s twice, its square, two products, the addition: 6.
    p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)), mag |p| + (lr / bc1) mag_m / denom: m (4), the denominator (v 6/2, sqrt, the cast of
    sqrt(bc2), the division, + eps: 7), m / denom (1), the cast of bc1 and lr / bc1 (2), the product (1), the subtraction (1): 16, say 17."""
    n, first, scale = case
    p, grads, m, v = K.adam_build(n, first)
    pd, md, vd = Guarded((n,), init=p), Guarded((n,), init=m), Guarded((n,), init=v)
    for k in range(K.ADAM_STEPS):
        step = first + k
        p0, m0, v0 = pd.cpu().clone(), md.cpu().clone(), vd.cpu().clone()
        call("mcav_adam_step", P(pd), P(dev(grads[k])), P(md), P(vd), n, K.ADAM_LR, K.ADAM_B1, K.ADAM_B2, K.ADAM_EPS, step, scale, outs=[pd, md, vd])
        r64, c32, mags = adam_columns(p0, grads[k], m0, v0, step, scale)
        three_col("step %d exp_avg" % step, md.t, c32[1], r64[1], mags[1], 4)
        three_col("step %d exp_avg_sq" % step, vd.t, c32[2], r64[2], mags[2], 6)
        three_col("step %d param" % step, pd.t, c32[0], r64[0], mags[0], 17)
    z = K.adam_zero_block(n)
    assert same_bits(pd.t[z], p[z]), "g = m = v = 0 moved the parameter"
    assert bool(torch.isfinite(pd.t).all()) and bool(torch.isfinite(md.t).all()) and bool(torch.isfinite(vd.t).all())
    assert bool((vd.t[z] == 0).all()) and bool((md.t[z] == 0).all())


@pytest.mark.parametrize("n,first", [(1000, 1), (257, 1000), (K.ADAM_GRID + 1, 1)])
def test_adam_device_state_entry_against_host_scalar_entry(n, first):
    """mcav_adam_step_dev from state8 = [step - 1, lr, grad_scale, ...] against mcav_adam_step at the same step, from the same state: the
    moments identical in bits; the parameters within one float32 step (the bias corrections come from the host's and the device's pow());
    state8[0] advances by one per call; an lr written into state8[1] takes effect on the next call."""
    scale = 0.5
    p, grads, m, v = K.adam_build(n, first)
    A = [Guarded((n,), init=t) for t in (p, m, v)]
    Bv = [Guarded((n,), init=t) for t in (p, m, v)]
    st = Guarded((8,), init=torch.tensor([first - 1, K.ADAM_LR, scale, 0, 0, 0, 0, 0], dtype=F32))
    lr = K.ADAM_LR
    for k in range(K.ADAM_STEPS):
        step = first + k
        if k == 3:
            lr = float(np.float32(2.5e-3))
            st.t[1] = lr
        Bv[0].t.copy_(A[0].t)
        gd = dev(grads[k])
        call("mcav_adam_step", P(A[0]), P(gd), P(A[1]), P(A[2]), n, lr, K.ADAM_B1, K.ADAM_B2, K.ADAM_EPS, step, scale, outs=A)
        call("mcav_adam_step_dev", P(Bv[0]), P(gd), P(Bv[1]), P(Bv[2]), n, K.ADAM_B1, K.ADAM_B2, K.ADAM_EPS, P(st), outs=Bv + [st])
        s8 = st.cpu()
        assert float(s8[0]) == step and float(s8[1]) == lr and float(s8[2]) == scale and (s8[5:] == 0).all()
        assert same_bits(A[1].t, Bv[1].t) and same_bits(A[2].t, Bv[2].t), "moments differ between the two entries at step %d" % step
        d = K.ulp_distance(A[0].cpu(), Bv[0].cpu())
        assert int(d.max()) <= 1, "parameters %d float32 steps apart at step %d" % (int(d.max()), step)
    # and the lr of the record against the reference (the agreement above is between two entries of one library)
    q = Guarded((n,), init=p)
    mm, vv = Guarded((n,), init=m), Guarded((n,), init=v)
    st2 = Guarded((8,), init=torch.tensor([first - 1, 2 * K.ADAM_LR, scale, 0, 0, 0, 0, 0], dtype=F32))
    call("mcav_adam_step_dev", P(q), P(dev(grads[0])), P(mm), P(vv), n, K.ADAM_B1, K.ADAM_B2, K.ADAM_EPS, P(st2), outs=[q, mm, vv, st2])
    r64, c32, mags = adam_columns(p, grads[0], m, v, first, scale, lr=2 * K.ADAM_LR)
    three_col("dev entry, lr x 2", q.t, c32[0], r64[0], mags[0], 17)


def test_fused_adam_capturable_continues_after_load_state_dict():
    """FusedAdam: two step()s, state_dict() into a second optimiser over copies of the parameters, then step_capturable() there against
    step() on the first: the step count continues at 3 on the host and in the device record, moments identical, parameters within one step."""
    from mcav.optim import FusedAdam
    g = K.gen(99)
    shapes = [(5, 3), (7,), (2, 2, 3, 3)]
    ps = [torch.nn.Parameter(dev(torch.randn(s, generator=g))) for s in shapes]
    grads = [[dev(torch.randn(s, generator=g)) for s in shapes] for _ in range(3)]
    A = FusedAdam(ps, 1e-3)
    A.grad_scale = 0.5
    A.zero_grad()
    for k in range(2):
        for p, gr in zip(ps, grads[k]):
            p.grad.copy_(gr)
        A.step()
    sd = copy.deepcopy(A.state_dict())
    assert all(float(s["step"]) == 2 for s in sd["state"].values())
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    Bo = FusedAdam(qs, 1e-3)
    Bo.grad_scale = 0.5
    Bo.zero_grad()
    Bo.load_state_dict(sd)
    assert Bo._step == 2
    for p, q, gr in zip(ps, qs, grads[2]):
        p.grad.copy_(gr); q.grad.copy_(gr)
    A.step()
    Bo.step_capturable()
    torch.cuda.synchronize()
    assert Bo._step == 3 and float(Bo.device_state()[0]) == 3.0
    assert all(float(s["step"]) == 3 for s in Bo.state_dict()["state"].values())
    assert same_bits(A._m, Bo._m) and same_bits(A._v, Bo._v)
    assert int(K.ulp_distance(A.arena().flat.cpu(), Bo.arena().flat.cpu()).max()) <= 1


# ================================================================================================ 3.7 layout, elementwise, helpers
@pytest.mark.parametrize("bhw", K.LAYOUT_BHW + (K.LAYOUT_WRAP,), ids=str)
def test_layout_kernels(bhw):
    """pure permutations, bit for bit; the channels of a pixel that a call does not own keep what the buffer held (the sentinel)"""
    B, H, W = bhw
    wrap = bhw == K.LAYOUT_WRAP
    for C, Cp, choff in (K.NCHW_TO_NHWC[:2] if wrap else K.NCHW_TO_NHWC):
        src = K.randn((B, C, H, W), B, C, H, 1)
        held = K.randn((B, H, W, Cp), B, Cp, H, 2)
        dst = Guarded((B, H, W, Cp), init=held)
        call("mcav_nchw_to_nhwc", P(dev(src)), B, C, H, W, P(dst), Cp, choff, outs=[dst])
        assert same_bits(dst.t, R.nchw_to_nhwc_ref(src, held, choff)), (C, Cp, choff)
    for C, Cp, choff in (K.NHWC_TO_NCHW[:2] if wrap else K.NHWC_TO_NCHW):
        src = K.randn((B, H, W, Cp), B, Cp, H, 3)
        dst = Guarded((B, C, H, W))
        call("mcav_nhwc_to_nchw", P(dev(src)), B, C, H, W, Cp, choff, P(dst), outs=[dst])
        assert same_bits(dst.t, R.nhwc_to_nchw_ref(src, C, choff)), (C, Cp, choff)
    for C, Cp in (K.NCHW3[:1] if wrap else K.NCHW3):
        s = [K.randn((B, C, H, W), B, C, H, 4 + i) for i in range(3)]
        dst = Guarded((B, H, W, Cp))
        sd = [dev(t) for t in s]
        call("mcav_nchw3_to_nhwc", P(sd[0]), P(sd[1]), P(sd[2]), B, C, H, W, P(dst), Cp, outs=[dst])
        assert same_bits(dst.t, R.nchw3_to_nhwc_ref(s[0], s[1], s[2], Cp)), (C, Cp)


def test_layout_kernels_refuse_bad_arguments():
    t = torch.ones(4096, device=DEV)
    o = Guarded((4096,))
    call("mcav_nchw3_to_nhwc", P(t), P(t), P(t), 1, 6, 2, 2, P(o), 16, outs=[o], expect=E_INVALID)          # 3 C > Cp
    call("mcav_nchw3_to_nhwc", P(t), P(t), P(t), 1, 1, 2, 2, P(o), 6, outs=[o], expect=E_INVALID)           # Cp not a multiple of 4
    call("mcav_nchw_to_nhwc", P(t), 1, 3, 2, 2, P(o), 4, 2, outs=[o], expect=E_INVALID)                     # choff + C > Cp
    call("mcav_nhwc_to_nchw", P(t), 1, 3, 2, 2, 4, 2, P(o), outs=[o], expect=E_INVALID)
    assert o.untouched()


@pytest.mark.parametrize("n", K.ELEMENTWISE_N)
def test_elementwise_kernels(n):
    """act_bwd: dy * act'(y): ReLU a selection (1 rounding allowed for the product by 1), ELU y + 1 and the product (2), sigmoid 1 - y and two
    products (3), + 1 when accumulated; mag |dy act'(y)| + |dx|.  add, mul: one IEEE operation, bit for bit.  affine a x + b: 2 roundings
    (1 when fused), mag |a x| + |b|."""
    for act in K.ACTS:
        y, dy, dx0 = K.act_output((n,), act, n, act), K.randn((n,), n, act, 1), K.randn((n,), n, act, 2)
        dyd, yd = dev(dy), dev(y)
        for acc in (False, True):
            dx = Guarded((n,), init=dx0 if acc else None)
            call("mcav_act_bwd", P(dyd), P(yd), act, n, P(dx), int(acc), outs=[dx])
            r64 = R.act_bwd_ref(dy.double(), y.double(), act, dx0.double() if acc else None)
            mag = (dy.double() * R.dact_ref(y.double(), act)).abs() + (dx0.double().abs() if acc else 0)
            three_col("act_bwd act=%d acc=%d" % (act, acc), dx.t, R.act_bwd_ref(dy, y, act, dx0 if acc else None), r64, mag, (1, 1, 2, 3)[act] + int(acc))
        if n <= 257:
            for stride in (1, 4, 16):
                dst = Guarded((n, stride))
                call("mcav_act_bwd_strided", P(dyd), P(yd), act, n, P(dst), stride, outs=[dst])
                got = dst.cpu()
                three_col("act_bwd_strided act=%d" % act, got[:, 0], R.act_bwd_ref(dy, y, act), R.act_bwd_ref(dy.double(), y.double(), act),
                          (dy.double() * R.dact_ref(y.double(), act)).abs(), (1, 1, 2, 3)[act])
                assert bool((bits(got[:, 1:]) == SENT32).all())                    # the other channels keep what the buffer held
    a, b = K.randn((n,), n, 7), K.randn((n,), n, 8)
    ad, bd = dev(a), dev(b)
    out = Guarded((n,))
    call("mcav_add", P(ad), P(bd), n, P(out), outs=[out])
    assert same_bits(out.t, a + b)
    out = Guarded((n,))
    call("mcav_mul", P(ad), P(bd), n, P(out), outs=[out])
    assert same_bits(out.t, a * b)
    for ca, cb in ((float(np.float32(10.0)), float(np.float32(0.01))), (float(np.float32(-0.3)), 0.0)):
        out = Guarded((n,))
        call("mcav_affine", P(ad), ca, cb, n, P(out), outs=[out])
        three_col("affine", out.t, ca * a + cb, ca * a.double() + cb, (ca * a.double()).abs() + abs(cb), 2)


@pytest.mark.parametrize("shape", K.SPATIAL_MEAN, ids=str)
def test_spatial_mean_and_its_adjoint(shape):
    """forward: n_pix sequential float32 additions, the division and the product by scale: n_pix + 1 roundings on mag scale * mean |x|.
    backward: scale / n_pix and one product: 2."""
    B, H, W, C = shape
    x, dout = K.randn(shape, B, H, W, C), K.randn((B, C), B, C, 3)
    scale = float(np.float32(0.06))
    out = Guarded((B, C))
    call("mcav_spatial_mean", P(dev(x)), B, H * W, C, scale, P(out), outs=[out])
    three_col("spatial_mean", out.t, R.spatial_mean_ref(x, scale), R.spatial_mean_ref(x.double(), scale), R.spatial_mean_ref(x.double().abs(), scale), H * W + 1)
    dx = Guarded(shape)
    call("mcav_spatial_mean_bwd", P(dev(dout)), B, H * W, C, scale, P(dx), outs=[dx])
    r64 = R.spatial_mean_bwd_ref(dout.double(), shape, scale)
    three_col("spatial_mean_bwd", dx.t, R.spatial_mean_bwd_ref(dout, shape, scale), r64, r64.abs(), 2)
    # <A x, y> = <x, A^T y> with the kernels' own outputs, in float64: 1e-5 of the sum of |terms| (n_pix + 3 roundings of 6e-8 at most)
    lhs, rhs = float((out.cpu().double() * dout.double()).sum()), float((x.double() * dx.cpu().double()).sum())
    assert abs(lhs - rhs) <= (H * W + 3) * U * float((x.double().abs() * r64.abs()).sum())


@pytest.mark.parametrize("case", K.COPY_CHANNELS, ids=str)
def test_copy_channels(case):
    n, Cs, soff, Cd, doff, C = case
    src, held = K.randn((n, Cs), n, Cs, 1), K.randn((n, Cd), n, Cd, 2)
    for acc in (0, 1):
        dst = Guarded((n, Cd), init=held)
        call("mcav_copy_channels", P(dev(src)), n, Cs, soff, P(dst), Cd, doff, C, acc, outs=[dst])
        assert same_bits(dst.t, R.copy_channels_ref(src, soff, held, doff, C, bool(acc)))          # (accumulate: one IEEE addition)
    o = Guarded((n, Cd))
    call("mcav_copy_channels", P(dev(src)), n, Cs, Cs - C + 1, P(o), Cd, doff, C, 0, outs=[o], expect=E_INVALID)
    call("mcav_copy_channels", P(dev(src)), n, Cs, soff, P(o), Cd, Cd - C + 1, C, 0, outs=[o], expect=E_INVALID)
    assert o.untouched()


@pytest.mark.parametrize("C", K.COLSUM_C)
@pytest.mark.parametrize("pix", K.COLSUM_PIX)
def test_colsum(C, pix):
    """Per channel.  A block owns per = ceil(pix / min(pix, 128)) pixels, PL = 256 / min(C, 256) lanes: a lane adds ceil(per / PL) values, lane 0
    the PL lane sums (from 0: PL additions); the blocks are added in float64 and cast once, + 1 when accumulated: ceil(per / PL) + PL + 1 (+ 1)
    roundings on mag sum |x| (+ |out|)."""
    from mcav import lib as L
    x, out0 = K.randn((pix, C), pix, C, 1) + 0.25, K.randn((C,), pix, C, 2)
    wsb = L.lib().mcav_colsum_workspace_bytes(C)
    per, PL = -(-pix // min(pix, 128)), 256 // min(C, 256)
    for acc in (0, 1):
        ws, out = Guarded((wsb,), torch.uint8), Guarded((C,), init=out0 if acc else None)
        call("mcav_colsum", P(dev(x)), pix, C, P(out), acc, P(ws), wsb, outs=[ws, out])
        three_col("colsum acc=%d" % acc, out.t, R.colsum_ref(x, out0 if acc else None), R.colsum_ref(x.double(), out0.double() if acc else None),
                  x.double().abs().sum(0) + (out0.double().abs() if acc else 0), -(-per // PL) + PL + 1 + acc)
    o, ws = Guarded((C,)), Guarded((wsb,), torch.uint8)
    call("mcav_colsum", P(dev(x)), pix, C, P(o), 0, P(ws), wsb - 1, outs=[o, ws], expect=E_WORKSPACE)
    assert o.untouched() and ws.untouched()


@pytest.mark.parametrize("case", K.UPSAMPLE, ids=str)
def test_upsample_nearest2x_and_its_adjoint(case):
    """forward a pure copy: bit for bit.  adjoint (a + b) + (c + d): 2 roundings on mag the same sum of |g|; and <A x, y> = <x, A^T y> holds
    between the two kernels to those roundings."""
    planes, h, w = case
    x, gout = K.randn((planes, h, w), planes, h, w), K.randn((planes, 2 * h, 2 * w), planes, h, w, 1)
    up = Guarded((planes, 2 * h, 2 * w))
    call("mcav_upsample_nearest2x", P(dev(x)), planes, h, w, P(up), outs=[up])
    assert same_bits(up.t, R.upsample_nearest2x_ref(x))
    gin = Guarded((planes, h, w))
    call("mcav_upsample_nearest2x_bwd", P(dev(gout)), planes, h, w, P(gin), outs=[gin])
    mag = R.upsample_nearest2x_bwd_ref(gout.double().abs())
    three_col("upsample_nearest2x_bwd", gin.t, R.upsample_nearest2x_bwd_ref(gout), R.upsample_nearest2x_bwd_ref(gout.double()), mag, 2)
    lhs, rhs = float((up.cpu().double() * gout.double()).sum()), float((x.double() * gin.cpu().double()).sum())
    assert abs(lhs - rhs) <= 2 * U * float((x.double().abs() * mag).sum())


@pytest.mark.parametrize("case", K.ADJ_FOLD, ids=str)
def test_upsample_adj_fold(case):
    """Up to nine ring / interior values fold onto a pixel (8 additions from zero: 9), the activation factor (ReLU 0, ELU 2, sigmoid 3: the
    factor and its product), the addend (1): mag (fold of |tmp|) * |act'| + |addend|."""
    B, Hl, Wl, C = case
    tmp = K.randn((B, Hl + 2, Wl + 2, C), B, Hl, Wl, C)
    addend = K.randn((B, Hl, Wl, C), B, Hl, Wl, C, 1)
    tmpd, addd = dev(tmp), dev(addend)
    for act in K.ACTS:
        aux = K.act_output((B, Hl, Wl, C), act, B, Hl, C, act)
        auxd = dev(aux)
        for use_aux, use_add in ((True, True), (True, False), (False, True), (False, False)):
            out = Guarded((B, Hl, Wl, C))
            call("mcav_upsample_adj_fold", P(tmpd), B, Hl, Wl, C, P(auxd) if use_aux else None, act, P(addd) if use_add else None, P(out), outs=[out])
            args = lambda t: (t(tmp), t(aux) if use_aux else None, act, t(addend) if use_add else None)
            mag = R.upsample_adj_fold_ref(tmp.double().abs(), None, 0, None) * (R.dact_ref(aux.double(), act).abs() if use_aux else 1) \
                + (addend.double().abs() if use_add else 0)
            three_col("adj_fold act=%d aux=%d add=%d" % (act, use_aux, use_add), out.t, R.upsample_adj_fold_ref(*args(lambda t: t)),
                      R.upsample_adj_fold_ref(*args(lambda t: t.double())), mag, 9 + ((0, 0, 2, 3)[act] if use_aux else 0) + int(use_add))
    o = Guarded((B, Hl, Wl, 6))
    call("mcav_upsample_adj_fold", P(tmpd), B, Hl, Wl, 6, None, 0, None, P(o), outs=[o], expect=E_INVALID)
    assert o.untouched()
