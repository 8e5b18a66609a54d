"""TEST INFRASTRUCTURE: the cases of the batch pseudo-LiDAR projection, shared by the CPU tests (restatement vs csrc/pl_math.h on the host)
and the GPU tests (restatement vs the kernels).  Everything is seeded numpy; a case's reference is computed once (reference()).

Calibration: KITTI's P_rect_02 rescaled to each image's true size, so the field of view stays at about 81 x 29 degrees, and the two dates'
velodyne -> camera transforms.  Scene: a tilted ground plane 1.65 m below the camera, boxes standing on it and a far backdrop above the
horizon, 2..90 m, at the network's resolution; the backdrop rises above max_height, a few pixels carry a negative value (behind q0 = 0),
one a NaN and one +inf."""
import functools

import numpy as np

import pl_batch_ref as R
from velo_ref import P_RECT_02, R_VELO, T_VELO

DATES = ("2011_09_26", "2011_09_28")
# calib_velo_to_cam of the second date (KITTI raw 2011_09_28)
R_VELO_28 = [6.927964e-03, -9.999722e-01, -2.757829e-03, -1.162982e-03, 2.749836e-03, -9.999955e-01, 9.999753e-01, 6.931141e-03, -1.143899e-03]
T_VELO_28 = [-2.457729e-02, -6.127237e-02, -3.321029e-01]


def scaled_P(date, H, W):
    """P_rect_02 of a 375 x 1242 image rescaled to H x W"""
    P = np.array(P_RECT_02[date], np.float64).reshape(3, 4)
    P[0] *= W / 1242.0
    P[1] *= H / 375.0
    return P


def velo_T(date):
    R_, T_ = (R_VELO, T_VELO) if date == DATES[0] else (R_VELO_28, T_VELO_28)
    return np.vstack([np.hstack([np.reshape(R_, (3, 3)), np.reshape(T_, (3, 1))]), [0.0, 0.0, 0.0, 1.0]])


def scene_depth(h, w, seed):
    """float32 [h, w] depths in 2..90 m"""
    rng = np.random.RandomState(seed)
    P = scaled_P(DATES[0], h, w)
    r, c = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    yn, xn = (r - P[1, 2]) / P[1, 1], (c - P[0, 2]) / P[0, 0]
    slope = yn + 0.03 * xn + rng.uniform(-0.01, 0.01)
    d = np.where(slope > 1.65 / 90.0, 1.65 / np.maximum(slope, 1e-6), rng.uniform(60.0, 90.0, (h, w)))
    for _ in range(3):                                             # boxes: constant depth, from above the horizon down to the ground
        z = rng.uniform(5.0, 35.0)
        c0 = rng.randint(0, max(w - 3, 1))
        cols = slice(c0, c0 + max(w // 6, 2))
        rows = slice(max(int(P[1, 2] - 0.25 * h), 0), min(int(P[1, 2] + 1.65 / z * P[1, 1]) + 1, h))
        d[rows, cols] = np.minimum(d[rows, cols], z)
    d = d * (1.0 + 0.01 * rng.randn(h, w))
    return np.clip(d, 2.0, 90.0).astype(np.float32)


def network_map(h, w, seed, input):
    """The plane the projection takes: sigmoid disparity (depth = 1 / (10 m + 0.01)) or depth, with the special pixels."""
    d = scene_depth(h, w, seed).astype(np.float64)
    m = ((1.0 / d - 0.01) / 10.0 if input == "disparity" else d).astype(np.float32)
    rng = np.random.RandomState(seed + 1000)
    flat = m.reshape(-1)
    idx = rng.choice(flat.size, 6, replace=False)
    flat[idx[:4]] = np.float32(-0.05 if input == "disparity" else -3.0)      # negative depth: behind q0 = 0
    flat[idx[4]] = np.nan
    flat[idx[5]] = np.inf
    return m


def uniform_tables(n_beams, n_azimuth, elevation=(-23.6, 2.0), azimuth=(-45.0, 45.0)):
    """pseudo_lidar.beam_tables' formula in numpy (the tests hand these very arrays to both sides)"""
    e = np.tan(np.deg2rad(np.linspace(elevation[0], elevation[1], n_beams + 1)))
    return e * np.abs(e), np.tan(np.deg2rad(np.linspace(azimuth[0], azimuth[1], n_azimuth + 1)))


SHAPES = {
    # name: (padded (Hg, Wg), true sizes, network (h, w), dates)
    "odd": ((23, 37), [(23, 37), (20, 33), (23, 30)], (8, 13), [0, 1, 0]),          # non-dyadic ratios, a partial last block, two dates
    "direct": ((8, 16), [(8, 16)], (8, 16), [0]),                                     # the direct-read path
    "chunks": ((375, 400), [(375, 400), (370, 396)], (24, 40), [0, 1]),              # 1172 blocks: past the scan's 1024-entry chunk
}
VARIANTS = {
    "dense": {},
    "sparse3": dict(sparsity=3),
    "depth": dict(input="depth", scale=1.25),
    "intensity": dict(with_intensity=True),
    "maxdepth": dict(max_depth=40.0, scale=1.25),
    "beams8x16": dict(beams=(8, 16)),
    "beams64x512": dict(beams=(64, 512)),
    "beams8x16_intensity_depth": dict(beams=(8, 16), with_intensity=True, input="depth", max_depth=60.0),
}
CASES = ["%s-%s" % (s, v) for s in SHAPES for v in VARIANTS]


@functools.lru_cache(maxsize=None)
def build(case):
    """-> dict of project_batch arguments (numpy): m, sizes, P, T, Hg, Wg, input, scale, intensity, max_height, max_depth, sparsity, beams"""
    shape, variant = case.split("-")
    (Hg, Wg), sizes, (h, w), dates = SHAPES[shape]
    v = dict(VARIANTS[variant])
    input = v.get("input", "disparity")
    B = len(sizes)
    seed = 17 * (sorted(SHAPES).index(shape) + 1)
    m = np.stack([network_map(h, w, seed + b, input) for b in range(B)])
    intensity = None
    if v.get("with_intensity"):
        intensity = np.random.RandomState(seed + 7).rand(B, h, w).astype(np.float32)
    beams = uniform_tables(*v["beams"]) if "beams" in v else None
    return dict(m=m, sizes=sizes, P=np.stack([scaled_P(DATES[k], H, W) for k, (H, W) in zip(dates, sizes)]),
                T=np.stack([velo_T(DATES[k]) for k in dates]), Hg=Hg, Wg=Wg, input=input, scale=v.get("scale", 1.0), intensity=intensity,
                max_height=1.0, max_depth=v.get("max_depth", np.inf), sparsity=v.get("sparsity", 0), beams=beams)


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (cloud float32 [n, 4], offsets int32 [B + 1]); shared, do not write into it"""
    cloud, offsets = R.project_batch(**build(case))
    cloud.setflags(write=False)
    offsets.setflags(write=False)
    return cloud, offsets


def check_non_trivial(case):
    """A kernel that drops everything must not pass: at least a quarter of every image's pixels in the plain dense cloud, at least 30 cells
    of every image in beam mode."""
    a = build(case)
    _, offsets = reference(case)
    n = np.diff(offsets)
    if a["beams"] is not None:
        assert (n >= 30).all(), (case, n.tolist())
    elif not a["sparsity"] and not np.isfinite(a["max_depth"]):
        assert all(4 * k >= H * W for k, (H, W) in zip(n, a["sizes"])), (case, n.tolist(), a["sizes"])
    else:
        assert (n > 0).all(), (case, n.tolist())
