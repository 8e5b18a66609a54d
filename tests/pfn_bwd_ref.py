"""TEST INFRASTRUCTURE: the definition of the pillar feature net's backward (include/mcav_depth.h: mcav_pillar_pseudo_image_bwd,
pseudo_lidar.PillarFeatureNet.gradients) in numpy on pfn_ref's fma32 / act, and the stock formulation in float64 torch differentiated by
autograd, which the restatement is held against (tests/test_pfn_bwd_cpu.py).

    g        g[p, o] for p < P: d_canvas[b, o, iy, ix] when the row's (b, iy, ix) lies inside the canvas, +0.0 otherwise or without a
             d_canvas; d_features[p, o] is added in float32 when given
    winner   pre, act and m = feat[p, o] as pfn_ref has them.  Gradient flows iff m > 0 (a NaN fails; relu'(0) = 0) and goes to the lowest
             slot k < n with act(pre[p, k, o]) == m; if no used slot attains m the padding term act(bias_pad[o]) won; a tie between a
             slot and the padding goes to the slot.  slot[p, o] = k, PADDING or NO_FLOW
    sums     d_weight[o, c] = sum_p g[p, o] voxels[p, k, c] and d_bias[o] = sum_p g[p, o] over the (p, o) won by a slot, d_bias_pad[o] =
             sum_p g[p, o] over those won by the padding: float64 terms (exact), float64 sums, rounded once
    d_voxels [capacity, N, C]: acc = +0.0, then for o ascending acc = fma32(g[p, o], weight[o, c], acc) whenever slot[p, o] == k; +0.0 in
             rows at and beyond P
"""
import functools

import numpy as np

import pfn_cases as C
import pfn_ref as R

F = np.float32
NO_FLOW, PADDING = -2, -1


def winners(voxels, num_points, P, weight, bias, bias_pad):
    """-> feat [P, C_out] float32 (pfn_ref.features' bits), slot [P, C_out] int64"""
    vox = np.asarray(voxels, F)[:P]
    weight, bias, bias_pad = np.asarray(weight, F), np.asarray(bias, F), np.asarray(bias_pad, F)
    N, Cc = vox.shape[1:]
    C_out = weight.shape[0]
    acc = np.broadcast_to(bias, (P, N, C_out)).astype(F)
    for c in range(Cc):
        acc = R.fma32(vox[:, :, c, None], weight[None, None, :, c], acc)
    a = R.act(acc)
    n = np.clip(np.asarray(num_points[:P], np.int64), 0, N)
    used = np.arange(N)[None, :] < n[:, None]
    feat = R.features(voxels, num_points, P, weight, bias, bias_pad)
    with np.errstate(invalid="ignore"):
        flows = feat > 0
        attains = (a == feat[:, None, :]) & used[:, :, None]
    slot = np.where(attains.any(axis=1), attains.argmax(axis=1), PADDING)
    slot = np.where(flows, slot, NO_FLOW).astype(np.int64)
    assert not ((slot == PADDING) & (n == N)[:, None]).any()
    return feat, slot


def upstream(coords, P, B, ny, nx, C_out, d_canvas=None, d_features=None):
    """-> g [P, C_out] float32; d_canvas [B, C_out, ny, nx]"""
    g = np.zeros((P, C_out), F)
    c = np.asarray(coords[:P], np.int64)
    if d_canvas is not None:
        ok = R.inside(c, B, ny, nx)
        g[ok] = np.asarray(d_canvas, F)[c[ok, 0], :, c[ok, 2], c[ok, 3]]
    if d_features is not None:
        g = (g + np.asarray(d_features, F)[:P]).astype(F)
    return g


def gradients(voxels, coords, num_points, offsets, nx, ny, weight, bias, bias_pad=None, d_canvas=None, d_features=None, capacity=None):
    """-> dict(d_weight, d_bias, d_bias_pad float32; d_voxels [capacity, N, C] float32; the float64 sums d_weight64, ... before their
    rounding and the sums of their terms' magnitudes abs_weight, abs_bias, abs_bias_pad; slot [P, C_out]; g [P, C_out])"""
    bias_pad = bias if bias_pad is None else bias_pad
    assert d_canvas is not None or d_features is not None
    vox, weight = np.asarray(voxels, F), np.asarray(weight, F)
    cap = len(vox) if capacity is None else min(capacity, len(vox))
    B, P = len(offsets) - 1, R.live_pillars(offsets, cap)
    N, Cc = vox.shape[1:]
    C_out = weight.shape[0]
    feat, slot = winners(vox, num_points, P, weight, bias, bias_pad)
    g = upstream(coords, P, B, ny, nx, C_out, d_canvas, d_features)
    g64 = g.astype(np.float64)
    to_slot, to_pad = slot >= 0, slot == PADDING
    x = vox[:P][np.arange(P)[:, None], np.clip(slot, 0, N - 1)].astype(np.float64)            # [P, C_out, C]: the winning slot's row
    with np.errstate(invalid="ignore", over="ignore"):
        tw = np.where(to_slot[:, :, None], g64[:, :, None] * x, 0.0)
        tb, tp = np.where(to_slot, g64, 0.0), np.where(to_pad, g64, 0.0)
        out = dict(d_weight64=tw.sum(axis=0), d_bias64=tb.sum(axis=0), d_bias_pad64=tp.sum(axis=0),
                   abs_weight=np.abs(tw).sum(axis=0), abs_bias=np.abs(tb).sum(axis=0), abs_bias_pad=np.abs(tp).sum(axis=0))
        for k in ("d_weight", "d_bias", "d_bias_pad"):
            out[k] = out[k + "64"].astype(F)
    dv = np.zeros((cap, N, Cc), F)
    acc = np.zeros((P, N, Cc), F)
    ks = np.arange(N)[None, :, None]
    for o in range(C_out):
        hit = slot[:, o, None, None] == ks                                                    # [P, N, 1]
        acc = np.where(hit, R.fma32(g[:, o, None, None], weight[o][None, None, :], acc), acc)
    dv[:P] = acc
    out.update(d_voxels=dv, slot=slot, g=g, features=feat)
    return out


def upstream_canvas(case, seed=0):
    """seeded normals over the WHOLE canvas [B, C_out, ny, nx] (a kernel that reads cells without a pillar is noticed: the restatement
    does not) and over the feature rows [P, C_out]; shared, read-only"""
    return _upstream(case, seed)


@functools.lru_cache(maxsize=None)
def _upstream(case, seed):
    a = C.build(case)
    rng = np.random.RandomState(7000 + seed + len(case))
    B, C_out = len(a["offsets"]) - 1, a["weight"].shape[0]
    dc = rng.standard_normal((B, C_out, a["ny"], a["nx"])).astype(F)
    df = rng.standard_normal((len(a["voxels"]), C_out)).astype(F)
    dc.setflags(write=False)
    df.setflags(write=False)
    return dc, df


@functools.lru_cache(maxsize=None)
def reference(case, pad="bias", source="canvas", capacity=None):
    """the restatement's gradients of a case of pfn_cases under upstream_canvas(case); source: "canvas", "features" or "both"; shared"""
    a = C.build(case)
    dc, df = upstream_canvas(case)
    out = gradients(a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"], C.bias_pad(a, pad),
                    d_canvas=dc if source in ("canvas", "both") else None, d_features=df if source in ("features", "both") else None,
                    capacity=capacity)
    for v in out.values():
        v.setflags(write=False)
    return out


def sum_bound(ref64, abs_terms):
    """one float32 rounding plus a float64 sum of at most 2^20 terms in any order"""
    return 2.0 ** -24 * np.abs(ref64) + 2.0 ** -32 * abs_terms


def check_sums(got, want, what=""):
    """got: dict or triple of float32 arrays (d_weight, d_bias, d_bias_pad) against the restatement's float64 sums within sum_bound;
    non-finite entries by class"""
    if not isinstance(got, dict):
        got = dict(zip(("d_weight", "d_bias", "d_bias_pad"), got))
    for k, t in (("d_weight", "abs_weight"), ("d_bias", "abs_bias"), ("d_bias_pad", "abs_bias_pad")):
        v, ref, mag = np.asarray(got[k]), want[k + "64"], want[t]
        assert v.dtype == F and v.shape == ref.shape, (k, v.dtype, v.shape)
        fin = np.isfinite(ref) & np.isfinite(mag)
        assert np.array_equal(np.isnan(v), np.isnan(ref)), (what, k, "NaNs elsewhere")
        inf = np.isinf(ref)
        assert np.array_equal(v[inf].astype(np.float64), ref[inf]), (what, k, "infinities")
        fin &= ~np.isnan(ref) & ~inf
        err = np.abs(v[fin].astype(np.float64) - ref[fin])
        bound = sum_bound(ref[fin], mag[fin])
        assert (err <= bound).all(), "%s %s: off by %g where %g is allowed" % (what, k, (err - bound).max(), bound[np.argmax(err - bound)])


# ---------------------------------------------------------------------------------------------- float64 autograd through the stock formulation
NEAR = 1e-5


def torch_autograd(a, bias_pad, d_canvas, keep=None):
    """F.linear over [P, N, C] with the zero-masked padding rows going through the layer as second.pytorch has them, relu, max(dim=1),
    indexed scatter into a zeros canvas, all float64, differentiated by autograd under the upstream gradient d_canvas * keep.
    -> dict(d_weight, d_bias, d_bias_pad, d_voxels (float64), slot [P, C_out] (the float64 winner), near [P, C_out] (the two best
    competitors -- the used slots and the padding term once -- lie within NEAR relative, the best being positive))
    keep [P, C_out] of 0 / 1 or None: the (p, o) whose upstream gradient counts"""
    import torch
    vox = torch.from_numpy(a["voxels"].astype(np.float64)).requires_grad_(True)
    w, b, bp = (torch.from_numpy(np.asarray(v, np.float64)).clone().requires_grad_(True) for v in (a["weight"], a["bias"], bias_pad))
    P, N, _ = vox.shape
    n = torch.from_numpy(a["num_points"].astype(np.int64)).clamp(0, N)
    used = torch.arange(N)[None, :] < n[:, None]
    masked = vox * used[:, :, None]
    pre = torch.nn.functional.linear(masked, w) + torch.where(used[:, :, None], b[None, None, :], bp[None, None, :])
    act = torch.relu(pre)
    feat, idx = act.max(dim=1)
    B = len(a["offsets"]) - 1
    c = torch.from_numpy(a["coords"].astype(np.int64))
    canvas = torch.zeros((B, w.shape[0], a["ny"], a["nx"]), dtype=torch.float64)
    canvas[c[:, 0], :, c[:, 2], c[:, 3]] = feat
    up = torch.from_numpy(np.asarray(d_canvas, np.float64))
    if keep is not None:
        mask = torch.zeros_like(canvas)
        mask[c[:, 0], :, c[:, 2], c[:, 3]] = torch.from_numpy(np.asarray(keep, np.float64))
        up = up * mask
    dv, dw, db, dbp = torch.autograd.grad((canvas * up).sum(), (vox, w, b, bp), allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    with torch.no_grad():
        # competitors: the used slots, and the padding term once (its copies in the unused slots are one value)
        comp = torch.where(used[:, :, None], act, torch.full_like(act, -1.0))
        comp = torch.cat([comp, torch.where((n < N)[:, None, None], torch.relu(bp)[None, None, :], torch.full((1, 1, 1), -1.0, dtype=torch.float64)).expand(P, 1, -1)], dim=1)
        top = torch.topk(comp, min(2, comp.shape[1]), dim=1).values
        best = top[:, 0]
        second = top[:, 1] if top.shape[1] > 1 else torch.full_like(best, -1.0)
        near = (best > 0) & (best - second <= NEAR * best)
        first = comp.argmax(dim=1)
        slot = torch.where(first < N, first, torch.full_like(first, PADDING))
        slot = torch.where(best > 0, slot, torch.full_like(slot, NO_FLOW))
    return dict(d_voxels=zero(dv, vox).numpy(), d_weight=zero(dw, w).numpy(), d_bias=zero(db, b).numpy(), d_bias_pad=zero(dbp, bp).numpy(),
                slot=slot.numpy(), near=near.numpy(), features=feat.detach().numpy())
