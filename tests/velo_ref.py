"""The definition of mcav_velo_depth_map (include/mcav_depth.h) in numpy, and a transcription of monodepth2's generate_depth_map to compare
it with; seeded KITTI-like scans and point_at for the tests and tools/velo_bench.py.

restated(): keep x >= 0 (float32), q_k = ((P[k,0] x + P[k,1] y) + P[k,2] z) + P[k,3] in float64 (each operation rounded on its own, in this
order), u = rint(q0 / q2) - 1, v = rint(q1 / q2) - 1 (half to even), land iff 0 <= u < W and 0 <= v < H in float64, d = q2 (or x), per
pixel the float32 of the minimum d; +0.0 without a point and for a minimum with the sign bit set; u -> W - 1 - u with the flip."""
from collections import Counter

import numpy as np

# KITTI raw calibration values (2011_09_26; P_rect_02 of both dates as in tests/kitti_tree.py)
P_RECT_02 = {"2011_09_26": [721.5377, 0.0, 609.5593, 44.85728, 0.0, 721.5377, 172.854, 0.2163791, 0.0, 0.0, 1.0, 0.002745884],
             "2011_09_28": [707.0493, 0.0, 604.0814, 45.75831, 0.0, 707.0493, 180.5066, -0.3454157, 0.0, 0.0, 1.0, 0.004981016]}
KITTI_SIZES = {"2011_09_26": (375, 1242), "2011_09_28": (370, 1226)}
R_RECT_00 = [9.999239e-01, 9.837760e-03, -7.445048e-03, -9.869795e-03, 9.999421e-01, -4.278459e-03, 7.402527e-03, 4.351614e-03, 9.999631e-01]
R_VELO = [7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01, 9.998621e-01, 7.523790e-03, 1.480755e-02]
T_VELO = [-4.069766e-03, -7.631618e-02, -2.717806e-01]


def compose(P_rect, R_rect=R_RECT_00, R=R_VELO, T=T_VELO):
    """monodepth2's composition: np.dot(np.dot(P_rect, R_cam2rect), velo2cam)."""
    v2c = np.vstack((np.hstack((np.reshape(R, (3, 3)), np.reshape(T, (3, 1)))), [0, 0, 0, 1.0]))
    Rc = np.eye(4)
    Rc[:3, :3] = np.reshape(R_rect, (3, 3))
    return np.dot(np.dot(np.reshape(P_rect, (3, 4)), Rc), v2c)


def kitti_P(date):
    return compose(P_RECT_02[date])


def scan(seed, n=120000):
    """A KITTI-like HDL-64E sweep: uniform azimuth, elevation -0.43..0.035 rad, range 1..90 m; 1 % of the points at 0 <= x < 0.3 m (some of
    them land with negative camera depth).  float32 [n, 4]."""
    rng = np.random.RandomState(seed)
    az = rng.uniform(-np.pi, np.pi, n)
    el = rng.uniform(-0.43, 0.035, n)
    r = rng.uniform(1.0, 90.0, n)
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.rand(n)], 1).astype(np.float32)
    k = n // 100
    pts[:k, 0] = rng.uniform(0, 0.3, k)
    return pts


def point_at(P, u, v, d, r=0.5):
    """A float32 point that lands on pixel (u, v) (0-based, after the -1) at camera depth ~d: solves P[:, :3] p = d (u + 1, v + 1, 1) - P[:, 3]."""
    q = d * np.array([u + 1.0, v + 1.0, 1.0]) - np.asarray(P)[:, 3]
    p = np.linalg.solve(np.asarray(P)[:, :3], q)
    return np.array([p[0], p[1], p[2], r], np.float32)


def project(P, velo):
    """-> (keep, q0, q1, q2, u, v) in float64, the fixed order of the definition."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    x, y, z = (velo[:, i].astype(np.float64) for i in range(3))
    keep = velo[:, 0] >= 0
    with np.errstate(all="ignore"):
        q = [((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z) + P[k, 3] for k in range(3)]
        u = np.round(q[0] / q[2]) - 1
        v = np.round(q[1] / q[2]) - 1
    return keep, q[0], q[1], q[2], u, v


def landing(P, velo, shape, depth_from_x=False):
    """-> (mask of the points that land, u, v as int64 (valid under the mask), d float64)."""
    H, W = shape
    keep, _, _, q2, u, v = project(P, velo)
    with np.errstate(invalid="ignore"):
        ok = keep & (u >= 0) & (v >= 0) & (u < W) & (v < H)
    ui = np.where(ok, u, 0).astype(np.int64)
    vi = np.where(ok, v, 0).astype(np.int64)
    d = velo[:, 0].astype(np.float64) if depth_from_x else q2
    return ok, ui, vi, d


def depth_key(d32):
    """The order-preserving uint32 key of float32 depths (csrc/velo_math.h depth_key)."""
    bits = np.asarray(d32, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def restated(P, velo, shape, flip=False, depth_from_x=False):
    """The definition: float32 [H, W]."""
    H, W = shape
    ok, u, v, d = landing(P, velo, shape, depth_from_x)
    if flip:
        u = W - 1 - u
    best = np.full(H * W, np.inf)
    hit = np.zeros(H * W, bool)
    idx = v[ok] * W + u[ok]
    np.minimum.at(best, idx, d[ok])
    hit[idx] = True
    with np.errstate(over="ignore"):
        out = np.where(hit, best, 0.0).astype(np.float32)
    out[np.signbit(out)] = 0.0
    return out.reshape(H, W)


def restated_batch(Ps, scans, sizes, Hg, Wg, flips=None, depth_from_x=False):
    """The zero-padded [B, Hg, Wg] float32 maps of a batch."""
    out = np.zeros((len(scans), Hg, Wg), np.float32)
    for b, (P, s, (H, W)) in enumerate(zip(Ps, scans, sizes)):
        out[b, :H, :W] = restated(P, s, (H, W), bool(flips[b]) if flips is not None else False, depth_from_x)
    return out


def sub2ind(matrixSize, rowSub, colSub):
    m, n = matrixSize
    return rowSub * (n - 1) + colSub - 1


def monodepth2(P, velo, im_shape, vel_depth=False):
    """monodepth2 kitti_utils.generate_depth_map after the calibration step, transcribed (float64 [H, W])."""
    velo = velo.copy()
    velo[:, 3] = 1.0
    velo = velo[velo[:, 0] >= 0, :]
    with np.errstate(all="ignore"):
        velo_pts_im = np.dot(P, velo.T).T
        velo_pts_im[:, :2] = velo_pts_im[:, :2] / velo_pts_im[:, 2][..., np.newaxis]
        if vel_depth:
            velo_pts_im[:, 2] = velo[:, 0]
        velo_pts_im[:, 0] = np.round(velo_pts_im[:, 0]) - 1
        velo_pts_im[:, 1] = np.round(velo_pts_im[:, 1]) - 1
        val_inds = (velo_pts_im[:, 0] >= 0) & (velo_pts_im[:, 1] >= 0)
        val_inds = val_inds & (velo_pts_im[:, 0] < im_shape[1]) & (velo_pts_im[:, 1] < im_shape[0])
    velo_pts_im = velo_pts_im[val_inds, :]
    depth = np.zeros((im_shape[:2]))
    depth[velo_pts_im[:, 1].astype(int), velo_pts_im[:, 0].astype(int)] = velo_pts_im[:, 2]
    inds = sub2ind(depth.shape, velo_pts_im[:, 1], velo_pts_im[:, 0])
    dupe_inds = [item for item, count in Counter(inds).items() if count > 1]
    for dd in dupe_inds:
        pts = np.where(inds == dd)[0]
        x_loc = int(velo_pts_im[pts[0], 0])
        y_loc = int(velo_pts_im[pts[0], 1])
        depth[y_loc, x_loc] = velo_pts_im[pts, 2].min()
    depth[depth < 0] = 0
    return depth


def edge_aliasing_case(P, shape, seed=7, n=20000):
    """A sweep plus 42 row pairs with points at (r, W-1) and (r+1, 0) (sub2ind aliases them), and 50 points near the sensor with negative
    camera depth; float32 [N, 4]."""
    H, W = shape
    rng = np.random.RandomState(seed)
    extra = []
    for r in range(10, min(300, H - 2), 7):
        extra += [point_at(P, W - 1, r, 30.0), point_at(P, W - 1, r, 20.0), point_at(P, 0, r + 1, 10.0)]
    for _ in range(50):
        extra.append(np.array([rng.uniform(0.0, 0.2), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 0.5], np.float32))
    return np.concatenate([scan(seed + 1000, n), np.stack(extra)])


# a dyadic P, q = (y, z, x): every operation exact, so .5 ties are real ties
P_DYADIC = np.array([[0, 1.0, 0, 0], [0, 0, 1.0, 0], [1.0, 0, 0, 0]])


def tie_points():
    """y / x = 2.5, 3.5, 1.5, 0.5 and z / x = 1.5, 2.5, 0.5, 4.5: half to even gives u = 1, 3, 1, -1 (dropped), v = 1, 1, -1 (dropped), 3."""
    return np.array([[2, 5, 3, 1], [2, 7, 5, 1], [4, 6, 2, 1], [2, 1, 9, 1]], np.float32)


def special_points():
    """NaN, +-inf, huge, x < 0 and x = -0.0 points (KITTI P)."""
    return np.array([[np.nan, 1, 1, 1], [np.inf, 0, 0, 1], [10, np.inf, 0, 1], [10, 0, np.nan, 1], [-1, 0, 0, 1], [-0.0, 0, 0, 1],
                     [1e38, 1e38, 1e38, 1], [-np.inf, 0, 0, 1], [10, -np.inf, 1, 1], [np.nan, np.nan, np.nan, np.nan]], np.float32)


# q = (2y, 2z, 4x): the point (1e38, 2e38, 2e38) lands on (0, 0) at depth 4e38, above FLT_MAX: +inf in the float32 map
P_OVERFLOW = np.array([[0, 2.0, 0, 0], [0, 0, 2.0, 0], [4.0, 0, 0, 0]])
