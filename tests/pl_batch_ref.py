"""TEST INFRASTRUCTURE: the batched pseudo-LiDAR projection (include/mcav_depth.h: mcav_pl_batch_project, PseudoLiDAR.project_batch)
restated in numpy -- its definition.  float64, element-wise, no matmul, every operation rounded on its own; the float32 steps (the
evaluation protocol's resize and depth conversion) in float32 with each operation rounded, the fused multiply-adds of
csrc/eval_math.h's bilinear_sample rounded once.

For image b with true size (Hb, Wb) inside the padded (Hg, Wg), P = P[b] (3x4), T = T[b] (4x4 velodyne -> camera), at pixel (r, c):
  v     = m[b] ([h, w] float32) resized to (Hb, Wb) as csrc/eval_math.h bilinear_sample does (the resize of tests/eval_protocol_ref.py
          `upsample`, which torch evaluates to within 2 float32 ulps of it); m[b][r, c] itself when (h, w) == (Hb, Wb)
  d     = eval_protocol_ref.depth_of(v, scale) = 1 / (10 v + 0.01) * scale in float32; input="depth": v * scale
  point = x = ((c - cu) d) / fu + bx, y likewise, q_j = ((x ti[j][0] + y ti[j][1]) + d ti[j][2]) + ti[j][3]  (csrc/pl_math.h)
  keep  = q0 >= 0 and q2 < max_height and d <= max_depth
  row   = float32(q0), float32(q1), float32(q2), i        i = 0 or an intensity plane [B, h, w] resized as m
dense: kept pixels in (image, row-major pixel) order, every sparsity-th of each image; beams: per (image, beam, azimuth) cell of the
tables the kept pixel (q0 > 0) with the smallest float32((q0 q0 + q1 q1) + q2 q2), ties to the lowest pixel, in cell order.
-> (cloud float32 [n, 4], offsets int32 [B + 1])
"""
import numpy as np

from eval_protocol_ref import depth_of

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """float32 fused multiply-add: a * b + c rounded once.  The product is exact in float64; the float64 sum is rounded to odd (TwoSum
    gives its error), so the final rounding to float32 is the rounding of the exact value."""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def axis_taps(n_in, n_out):
    """eval_math.h bilinear_axis for every output index of one axis -> (i0, i1, l float32)"""
    scale = F32(n_in) / F32(n_out)
    s = fma32(scale, np.arange(n_out, dtype=F32) + F32(0.5), F32(-0.5))
    s = np.where(s < 0, F32(0), s).astype(F32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    return i0, i1, (s - i0.astype(F32)).astype(F32)


def resize(plane, Hb, Wb):
    """eval_math.h bilinear_sample over the whole (Hb, Wb) image; the plane itself at equal sizes."""
    plane = np.asarray(plane, F32)
    h, w = plane.shape
    if (h, w) == (Hb, Wb):
        return plane.copy()
    y0, y1, ly = axis_taps(h, Hb)
    x0, x1, lx = axis_taps(w, Wb)
    ly, lx = ly[:, None], lx[None, :]
    hy, hx = F32(1) - ly, F32(1) - lx
    with np.errstate(all="ignore"):
        t = fma32(hx, plane[y0][:, x0], lx * plane[y0][:, x1])
        b = fma32(hx, plane[y1][:, x0], lx * plane[y1][:, x1])
        return (hy * t + ly * b).astype(F32)


def calib(P, T):
    """cu, cv, fu, fv, bx, by and ti = [R' | -R' t] (3x4), as mcav_pseudo_lidar_project forms them"""
    P, T = np.asarray(P, F64).reshape(3, 4), np.asarray(T, F64).reshape(4, 4)
    cu, cv, fu, fv = P[0, 2], P[1, 2], P[0, 0], P[1, 1]
    bx, by = P[0, 3] / (-fu), P[1, 3] / (-fv)
    ti = np.zeros((3, 4))
    for i in range(3):
        ti[i, :3] = T[:3, i]
        acc = F64(0.0)
        for j in range(3):
            acc = acc + (-T[j, i]) * T[j, 3]
        ti[i, 3] = acc
    return cu, cv, fu, fv, bx, by, ti


def depth_image(m_b, Hb, Wb, input="disparity", scale=1.0):
    """float32 [Hb, Wb]"""
    v = resize(m_b, Hb, Wb)
    with np.errstate(all="ignore"):
        return depth_of(v, scale) if input == "disparity" else (v * F32(scale)).astype(F32)


def points(d, P, T):
    """d float32 [Hb, Wb] -> q float64 [Hb, Wb, 3]"""
    cu, cv, fu, fv, bx, by, ti = calib(P, T)
    Hb, Wb = d.shape
    r, c = np.meshgrid(np.arange(Hb, dtype=F64), np.arange(Wb, dtype=F64), indexing="ij")
    d = d.astype(F64)
    with np.errstate(all="ignore"):
        x = ((c - cu) * d) / fu + bx
        y = ((r - cv) * d) / fv + by
        return np.stack([((x * ti[j, 0] + y * ti[j, 1]) + d * ti[j, 2]) + ti[j, 3] for j in range(3)], axis=-1)


def kept(q, d, max_height=1.0, max_depth=np.inf):
    with np.errstate(all="ignore"):
        return (q[..., 0] >= 0) & (q[..., 2] < F64(max_height)) & (d.astype(F64) <= F64(max_depth))


def table_bin(tab, v):
    """k with tab[k] <= v < tab[k+1]; -1 outside the table or for a NaN"""
    tab = np.asarray(tab, F64)
    with np.errstate(all="ignore"):
        inside = (v >= tab[0]) & (v < tab[-1])
    k = np.searchsorted(tab, np.where(inside, v, tab[0]), side="right") - 1
    return np.where(inside, k, -1)


def cells_of(q, elev, azim):
    """-> (beam, azimuth bin) per point, -1 where it is in front of no cell"""
    q0, q1, q2 = q[..., 0], q[..., 1], q[..., 2]
    with np.errstate(all="ignore"):
        s = (q2 * np.abs(q2)) / (q0 * q0 + q1 * q1)
        a = q1 / q0
        front = q0 > 0
    beam = np.where(front, table_bin(elev, s), -1)
    az = np.where(front, table_bin(azim, a), -1)
    bad = (beam < 0) | (az < 0)
    return np.where(bad, -1, beam), np.where(bad, -1, az)


def range32(q):
    with np.errstate(all="ignore"):
        return ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]).astype(F32)


def beam_winners(q, keep, elev, azim, order=None):
    """-> the flat pixel indices of the winners in (beam, azimuth) order.  order: the pixel order in which the cells are filled (any
    permutation gives the same winners: the minimum of (range bits, pixel index) does not depend on it)."""
    nb, na = len(elev) - 1, len(azim) - 1
    beam, az = cells_of(q, elev, azim)
    key = range32(q).view(np.uint32).astype(np.uint64).reshape(-1)
    beam, az, keep = beam.reshape(-1), az.reshape(-1), keep.reshape(-1)
    cells = np.full(nb * na, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    idx = np.flatnonzero(keep & (beam >= 0))
    if order is not None:
        idx = np.asarray(order)[np.isin(order, idx)]
    word = (key[idx] << np.uint64(32)) | idx.astype(np.uint64)
    np.minimum.at(cells, beam[idx] * na + az[idx], word)
    return (cells[cells != np.uint64(0xFFFFFFFFFFFFFFFF)] & np.uint64(0xFFFFFFFF)).astype(np.int64)


def project_batch(m, sizes=None, P=None, T=None, Hg=None, Wg=None, input="disparity", scale=1.0, intensity=None, max_height=1.0,
                  max_depth=np.inf, sparsity=0, beams=None, order=None):
    """m [B, h, w]; sizes B pairs (Hb, Wb) (default: (h, w)); P [B, 3, 4] or [3, 4]; T [B, 4, 4] or [4, 4]; beams: (elev, azim) tables.
    Hg, Wg only bound the sizes.  -> (cloud float32 [n, 4], offsets int32 [B + 1])"""
    m = np.asarray(m, F32)
    B, h, w = m.shape
    sizes = [(h, w)] * B if sizes is None else [tuple(int(v) for v in s) for s in sizes]
    P = np.broadcast_to(np.asarray(P, F64), (B, 3, 4))
    T = np.broadcast_to(np.asarray(T, F64), (B, 4, 4))
    assert not (beams is not None and sparsity), "sparsity has no meaning in beam mode"
    rows, offsets = [], [0]
    for b in range(B):
        Hb, Wb = sizes[b]
        assert (Hg is None or Hb <= Hg) and (Wg is None or Wb <= Wg)
        d = depth_image(m[b], Hb, Wb, input, scale)
        q = points(d, P[b], T[b])
        keep = kept(q, d, max_height, max_depth)
        if beams is None:
            idx = np.flatnonzero(keep.reshape(-1))
            if sparsity:
                idx = idx[0::int(sparsity)]
        else:
            idx = beam_winners(q, keep, beams[0], beams[1], order)
        with np.errstate(all="ignore"):
            xyz = q.reshape(-1, 3)[idx].astype(F32)
        i = np.zeros(len(idx), F32) if intensity is None else resize(intensity[b], Hb, Wb).reshape(-1)[idx]
        rows.append(np.concatenate([xyz, i[:, None]], axis=1).astype(F32))
        offsets.append(offsets[-1] + len(idx))
    return np.concatenate(rows).reshape(-1, 4), np.asarray(offsets, np.int32)

