"""TEST INFRASTRUCTURE: the definition of the two backwards that carry a gradient from pillar voxels back to the network's plane
(include/mcav_depth.h: mcav_pillarize_bwd, mcav_pl_batch_project_bwd; pseudo_lidar.pillarize_backward, project_batch_backward) in numpy,
one operation per rounding, the forwards' provenance (mcav_pillarize_indexed's slot_points, mcav_pl_batch_project_indexed's pixels)
restated from pillar_ref / pl_batch_ref, and the stock formulations in float64 torch differentiated by autograd, which the restatement
is held against (tests/test_pl_bwd_cpu.py).

Selection is piecewise constant: which pixel became which cloud row and which row which slot is taken from the forward, and only the
arithmetic behind it is differentiated.

pillars   slot k < count of pillar p holding row i, g = d_voxels[p]:
            C = 4   d_points[i][c] = g[k][c]
            C = 9   d_points[i][0] = float32((((double)g[k][0] + g[k][4]) + g[k][7]) - S4 / count), S4 = float64 sum of g[j][4], j < count, in
                    slot order from +0; y: columns 1, 5, 8; z: columns 2, 6 (no centre column); column 3 passes through
          every other row of d_points [n_max, 4] is +0.0
plane     a) row o of image b at (r, c) = pixels[o]: v = the plane resampled as the forward does, s_b the image's float32 scale,
             a_j = (((c - cu) / fu) ti[j][0] + ((r - cv) / fv) ti[j][1]) + ti[j][2], g_d = (g0 a_0 + g1 a_1) + g2 a_2, all float64;
             slope = ((-10 s_b) u) u with u = 1 / (10 v + 0.01), or s_b for a depth input; G[b][r][c] = float32(g_d slope), +0.0 elsewhere
          b) d_m[b][y][x] = float32 of the float64 sum over (r, c) ascending of (wy[r, y] wx[c, x]) G[b][r][c], w the forward's float32
             tap weights (1 - l at the lower tap, l at the upper, added in float32 where they coincide); G itself at equal sizes

ERROR BOUNDS against the float64 stock formulation (exact selection, float32 taps and weights promoted, everything else float64):
  pillars : the terms are float32 values promoted (exact); the float64 sums err by 2^-53 per operation; one rounding to float32 at the
            store: |err| <= 2^-24 |ref| + 2^-32 sum |terms| (pfn_bwd_ref.sum_bound).
  plane   : a term of d_m[y, x] is t = wy wx G[r, c].  Counting the float32 roundings behind it:
            (1) G is rounded once at its store: 2^-24 |t|.
            (2) v in the slope is the forward's float32 sample where the stock formulation has the exact blend: three float32 roundings
                on the way (the inner product or its fused sum, the outer product, the outer sum), each at most 2^-24 of the sum of the
                blend's magnitudes A = sum |w_i m_i|, so |dv| <= 3 2^-24 A.  slope = -10 s u^2 has d slope / slope = -20 u dv, so the
                term errs by 6 2^-24 kappa |t| with kappa = 10 u A; kappa < 1 when all four taps are positive (10 v u < 1).  A direct
                read or a depth input has no such error (kappa = 0).
            (3) the final store rounds the sum once: 2^-24 |ref|.
            float64 operations add 2^-53 each: 2^-40 sum |t| covers them.
            |err| <= 2^-24 (|ref| + sum |t| (1 + 6 kappa)) + 2^-40 sum |t|.  With kappa <= 1 this is the constant bound
                2^-24 (|ref| + 7 sum |t|) + 2^-40 sum |t|  <=  8 2^-24 sum |t| (1 + 2^-20)      (plane_bound),
            half of 2^-20 sum |t|.  The cases' planes are positive, so it is asserted on every element of every case.
            kappa > 1 needs a blend across a sign change that still lands in front of the camera, where 10 v + 0.01 nearly cancels and
            the slope is ill-conditioned in v itself.  One labelled case (`odd-negatives`) keeps the scene's negative disparities to show
            it; there, and only there, the tests use the kappa-weighted form (plane_bound_conditioned).
"""
import numpy as np

import pillar_ref as PR
import pl_batch_ref as R

F32, F64 = np.float32, np.float64
F32_MAX = np.finfo(F32).max


# ---------------------------------------------------------------------------------------------- pillars
def pillar_slots(points, offsets, grid, max_points, capacity=None):
    """-> slot_points int32 [P', N]: the row of `points` in every slot (-1: padding), P' = min(P, capacity); pillar_ref.pillarize's
    selection with the rows kept instead of their values"""
    points = np.asarray(points, F32)
    offsets = np.asarray(offsets, np.int32)
    N = int(max_points)
    n = PR.live_rows(points, offsets)
    idx = np.arange(n, dtype=np.int64)
    b = PR.image_of(offsets, idx)
    ix, iy, keep = PR.cells_of(points[:n], grid)
    cell = ((b * grid.ny + iy) * grid.nx + ix)[keep]
    rows = idx[keep]
    order = np.argsort(cell, kind="stable")
    cell, rows = cell[order], rows[order]
    ucell, start, count = np.unique(cell, return_index=True, return_counts=True)
    P = len(ucell)
    out = np.full((P, N), -1, np.int32)
    for p in range(P):
        k = min(int(count[p]), N)
        out[p, :k] = rows[start[p]:start[p] + k]
    return out[:P if capacity is None else min(int(capacity), P)]


def pillarize_bwd(d_voxels, slot_points, num_points, n_max):
    """d_voxels [>= P', N, C], slot_points [P', N], num_points [P'] -> dict(d_points float32 [n_max, 4], d_points64 and abs_terms
    float64 [n_max, 4]: the sums before their rounding and the sums of their terms' magnitudes)"""
    g = np.asarray(d_voxels, F32)
    P, N = slot_points.shape
    C = g.shape[2]
    out64, mag = np.zeros((n_max, 4), F64), np.zeros((n_max, 4), F64)
    out = np.zeros((n_max, 4), F32)
    for p in range(P):
        count = min(max(int(num_points[p]), 0), N)
        S, A = np.zeros(3, F64), np.zeros(3, F64)
        if C == 9:
            for j in range(count):                                  # slot order from +0
                S = S + g[p, j, 4:7].astype(F64)
                A = A + np.abs(g[p, j, 4:7].astype(F64))
        for k in range(count):
            i = int(slot_points[p, k])
            assert 0 <= i < n_max
            row = g[p, k].astype(F64)
            for c in range(4):
                if C == 4 or c == 3:
                    out[i, c], out64[i, c], mag[i, c] = g[p, k, c], row[c], abs(row[c])
                    continue
                own = row[c] + row[4 + c]
                m_ = abs(row[c]) + abs(row[4 + c])
                if c < 2:
                    own = own + row[7 + c]
                    m_ += abs(row[7 + c])
                out64[i, c] = own - S[c] / F64(count)
                mag[i, c] = m_ + A[c] / count
                out[i, c] = F32(out64[i, c])
    return dict(d_points=out, d_points64=out64, abs_terms=mag)


def pillar_autograd(points, slot_points, num_points, centres, d_voxels, C):
    """The stock formulation in float64 torch: gather the rows by index, mask the padding, PointPillars' decoration (mean over the used
    slots, the cell's centre a constant), autograd under d_voxels.  centres [P', 2] float64 -> d_points float64 [n_max, 4]"""
    import torch
    pts = torch.from_numpy(np.asarray(points, F64)).requires_grad_(True)
    sp = torch.from_numpy(slot_points.astype(np.int64))
    P, N = sp.shape
    n = torch.from_numpy(np.asarray(num_points, np.int64)).clamp(0, N)
    used = (torch.arange(N)[None, :] < n[:, None]).to(torch.float64)
    vox = pts[sp.clamp(min=0)] * used[:, :, None]
    if C == 9:
        mean = vox[:, :, :3].sum(dim=1) / n[:, None].to(torch.float64)
        cen = torch.from_numpy(np.asarray(centres, F64))
        vox = torch.cat([vox, (vox[:, :, :3] - mean[:, None, :]) * used[:, :, None], (vox[:, :, :2] - cen[:, None, :]) * used[:, :, None]], dim=2)
    up = torch.from_numpy(np.asarray(d_voxels, F64)[:P])
    (grad,) = torch.autograd.grad((vox * up).sum(), (pts,))
    return grad.numpy()


# ---------------------------------------------------------------------------------------------- the projection's provenance
def image_scales(B, scale, scales):
    """-> float32 [B] as the kernels form them, ok [B]: finite and positive (every image without a table)"""
    if scales is None:
        return np.full(B, F32(scale), F32), np.ones(B, bool)
    with np.errstate(all="ignore"):
        s = (F32(scale) * np.asarray(scales, F32)).astype(F32)
        return s, (s > 0) & (s <= F32_MAX)


def project_forward(m, sizes=None, P=None, T=None, Hg=None, Wg=None, input="disparity", scale=1.0, scales=None, intensity=None,
                    max_height=1.0, max_depth=np.inf, sparsity=0, beams=None, capacity=None):
    """pl_batch_ref.project_batch with per-image scales, a capacity, and the selection kept.
    -> dict(cloud float32 [n', 4], offsets int32 [B + 1] (exact), pixels int32 [n'] = r * Wg + c, image int64 [n'], n' = min(n, capacity))"""
    m = np.asarray(m, F32)
    B, h, w = m.shape
    sizes = [(h, w)] * B if sizes is None else [tuple(int(v) for v in s) for s in sizes]
    P = np.broadcast_to(np.asarray(P, F64), (B, 3, 4))
    T = np.broadcast_to(np.asarray(T, F64), (B, 4, 4))
    s, ok = image_scales(B, scale, scales)
    rows, pixels, image, offsets = [np.zeros((0, 4), F32)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [0]
    for b in range(B):
        Hb, Wb = sizes[b]
        idx = np.zeros(0, np.int64)
        if ok[b]:
            d = R.depth_image(m[b], Hb, Wb, input, s[b])
            q = R.points(d, P[b], T[b])
            keep = R.kept(q, d, max_height, max_depth)
            if beams is None:
                idx = np.flatnonzero(keep.reshape(-1))
                if sparsity:
                    idx = idx[0::int(sparsity)]
            else:
                idx = R.beam_winners(q, keep, beams[0], beams[1])
            with np.errstate(all="ignore"):
                xyz = q.reshape(-1, 3)[idx].astype(F32)
            i = np.zeros(len(idx), F32) if intensity is None else R.resize(intensity[b], Hb, Wb).reshape(-1)[idx]
            rows.append(np.concatenate([xyz, i[:, None]], axis=1).astype(F32))
        r, c = idx // Wb, idx % Wb
        pixels.append(r * Wg + c)
        image.append(np.full(len(idx), b, np.int64))
        offsets.append(offsets[-1] + len(idx))
    cap = offsets[-1] if capacity is None else min(int(capacity), offsets[-1])
    return dict(cloud=np.concatenate(rows).reshape(-1, 4)[:cap], offsets=np.asarray(offsets, np.int32),
                pixels=np.concatenate(pixels).astype(np.int32)[:cap], image=np.concatenate(image)[:cap])


def tap_weights(n_in, n_out):
    """-> float32 [n_out, n_in]: the forward's weight of every source in every output of one axis (1 - l at the lower tap, l at the upper,
    the two added in float32 where they coincide); the identity at equal sizes (the direct read)"""
    if n_in == n_out:
        return np.eye(n_in, dtype=F32)
    i0, i1, l = R.axis_taps(n_in, n_out)
    W = np.zeros((n_out, n_in), F32)
    o = np.arange(n_out)
    W[o, i0] = (F32(1) - l).astype(F32)
    W[o, i1] = (W[o, i1] + l).astype(F32)
    return W


def sample_rows(m_b, Hb, Wb, r, c):
    """the forward's float32 sample at pixels (r, c) and the sum of its blend's magnitudes (float64; 0 for the direct read)"""
    h, w = m_b.shape
    v = R.resize(m_b, Hb, Wb)[r, c]
    if (h, w) == (Hb, Wb):
        return v, np.zeros(len(r), F64)
    Wy, Wx = tap_weights(h, Hb).astype(F64), tap_weights(w, Wb).astype(F64)
    A = Wy @ np.abs(m_b.astype(F64)) @ Wx.T
    return v, A[r, c]


def project_bwd(d_points, fwd, m, sizes=None, P=None, T=None, Hg=None, Wg=None, input="disparity", scale=1.0, scales=None, **_):
    """d_points [>= n', 4]; fwd: project_forward's dict -> dict(d_m float32 [B, h, w], G float32 [B, Hg, Wg]; d_m64 the sums before their
    rounding, abs_terms sum |t| and weighted_terms sum |t| (1 + 6 kappa) per element of d_m, kappa [B, Hg, Wg] per pixel -- see the
    module's bound)"""
    m = np.asarray(m, F32)
    B, h, w = m.shape
    sizes = [(h, w)] * B if sizes is None else [tuple(int(v) for v in s) for s in sizes]
    P = np.broadcast_to(np.asarray(P, F64), (B, 3, 4))
    T = np.broadcast_to(np.asarray(T, F64), (B, 4, 4))
    s, ok = image_scales(B, scale, scales)
    g = np.asarray(d_points, F32)
    G = np.zeros((B, Hg, Wg), F32)
    Kap = np.zeros((B, Hg, Wg), F64)
    d_m, d_m64 = np.zeros((B, h, w), F32), np.zeros((B, h, w), F64)
    mag, wmag = np.zeros((B, h, w), F64), np.zeros((B, h, w), F64)
    for b in range(B):
        Hb, Wb = sizes[b]
        rows = np.flatnonzero(fwd["image"] == b)
        if not ok[b]:
            assert len(rows) == 0
            continue
        px = fwd["pixels"][rows].astype(np.int64)
        r, c = px // Wg, px % Wg
        assert (r < Hb).all() and (c < Wb).all()
        v, A = sample_rows(m[b], Hb, Wb, r, c)
        cu, cv, fu, fv, bx, by, ti = R.calib(P[b], T[b])
        xn, yn = (c.astype(F64) - cu) / fu, (r.astype(F64) - cv) / fv
        a = [(xn * ti[j, 0] + yn * ti[j, 1]) + ti[j, 2] for j in range(3)]
        g64 = g[rows].astype(F64)
        gd = (g64[:, 0] * a[0] + g64[:, 1] * a[1]) + g64[:, 2] * a[2]
        if input == "disparity":
            u = F64(1.0) / (F64(10.0) * v.astype(F64) + F64(0.01))
            slope = ((F64(-10.0) * F64(s[b])) * u) * u
            Kap[b, r, c] = 10.0 * np.abs(u) * A
        else:
            slope = np.full(len(rows), F64(s[b]))
        G[b, r, c] = (gd * slope).astype(F32)
        if (h, w) == (Hb, Wb):
            d_m[b] = G[b, :h, :w]
            d_m64[b] = G[b, :h, :w].astype(F64)
            mag[b] = wmag[b] = np.abs(d_m64[b])
            continue
        Wy, Wx = tap_weights(h, Hb).astype(F64), tap_weights(w, Wb).astype(F64)
        acc = np.zeros((h, w), F64)
        for rr in range(Hb):                                        # ascending (r, c); a pixel outside the window adds (+-0) to a sum
            for cc in range(Wb):                                    # that started at +0: no bit changes
                t = (Wy[rr][:, None] * Wx[cc][None, :]) * F64(G[b, rr, cc])
                acc = acc + t
                mag[b] += np.abs(t)
                wmag[b] += np.abs(t) * (1.0 + 6.0 * Kap[b, rr, cc])
        d_m64[b] = acc
        d_m[b] = acc.astype(F32)
    return dict(d_m=d_m, G=G, d_m64=d_m64, abs_terms=mag, weighted_terms=wmag, kappa=Kap)


def plane_bound(ref64, out):
    """the module's constant bound per element of d_m: kappa <= 1 on every contributing pixel (asserted by the caller)"""
    return 2.0 ** -24 * (np.abs(ref64) + 7.0 * out["abs_terms"]) + 2.0 ** -40 * out["abs_terms"]


def plane_bound_conditioned(ref64, out):
    """the kappa-weighted form, for the ill-conditioned demonstration alone"""
    return 2.0 ** -24 * (np.abs(ref64) + out["weighted_terms"]) + 2.0 ** -40 * out["abs_terms"]


def project_autograd(d_points, fwd, m, sizes=None, P=None, T=None, Hg=None, Wg=None, input="disparity", scale=1.0, scales=None, **_):
    """The stock formulation in float64 torch: the resize as two matrix products with the forward's float32 weights, the depth, the
    un-projection, the rows gathered by index, autograd under d_points.  -> d_m float64 [B, h, w]"""
    import torch
    m = np.asarray(m, F32)
    B, h, w = m.shape
    sizes = [(h, w)] * B if sizes is None else [tuple(int(v) for v in s) for s in sizes]
    P = np.broadcast_to(np.asarray(P, F64), (B, 3, 4))
    T = np.broadcast_to(np.asarray(T, F64), (B, 4, 4))
    s, ok = image_scales(B, scale, scales)
    mt = torch.from_numpy(m.astype(F64)).requires_grad_(True)
    up = torch.from_numpy(np.asarray(d_points, F64))
    loss = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        rows = np.flatnonzero(fwd["image"] == b)
        if not ok[b] or len(rows) == 0:
            continue
        Hb, Wb = sizes[b]
        Wy, Wx = (torch.from_numpy(tap_weights(n, N).astype(F64)) for n, N in ((h, Hb), (w, Wb)))
        v = Wy @ mt[b] @ Wx.T
        d = float(s[b]) / (10.0 * v + 0.01) if input == "disparity" else v * float(s[b])
        cu, cv, fu, fv, bx, by, ti = R.calib(P[b], T[b])
        rr, cc = torch.meshgrid(torch.arange(Hb, dtype=torch.float64), torch.arange(Wb, dtype=torch.float64), indexing="ij")
        x = ((cc - cu) * d) / fu + bx
        y = ((rr - cv) * d) / fv + by
        q = torch.stack([((x * ti[j, 0] + y * ti[j, 1]) + d * ti[j, 2]) + ti[j, 3] for j in range(3)], dim=-1)
        px = torch.from_numpy(fwd["pixels"][rows].astype(np.int64))
        cloud = q[px // Wg, px % Wg]                                # indexing by the recorded selection
        loss = loss + (cloud * up[torch.from_numpy(rows), :3]).sum()
    (grad,) = torch.autograd.grad(loss, (mt,), allow_unused=True)
    return np.zeros((B, h, w), F64) if grad is None else grad.numpy()
