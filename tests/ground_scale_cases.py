"""TEST INFRASTRUCTURE: the scenes of the ground-plane scale estimator, shared by the CPU tests (restatement vs csrc/ground_math.h on the
host, float32 vs float64) and the GPU tests (restatement vs the kernels).  Seeded numpy; a case's reference is computed once.

Scene, at the network's resolution, on the rays of the definition (tests/ground_scale_ref.py): the ground is the plane
Y + 0.03 X + 0.01 Z = 1.65, d = 1.65 / (yn + 0.03 xn + 0.01) where that lies below 80 m; elsewhere a sloped backdrop 80 - 20 xn; two
constant-depth boxes stand on the ground; multiplicative noise 1 + sigma randn, clipped to 2..90 m; the result is divided by s_true and
turned into a disparity.  The estimator must answer s_true * sqrt(1 + 0.03^2 + 0.01^2)."""
import functools

import numpy as np

import ground_scale_ref as G
from pl_batch_cases import DATES, scaled_P, velo_T

CAMERA_HEIGHT = 1.65
PLANE = (0.03, 1.0, 0.01)
ANALYTIC = float(np.sqrt(1.0 + 0.03 ** 2 + 0.01 ** 2))


def scene_depth(h, w, size, P, sigma, seed, ground=True):
    """float64 [h, w] metric depths, 2..90 m"""
    rng = np.random.RandomState(seed)
    xn = G.rays(size[1], w, P[0, 2], P[0, 0], np.float64)[None, :]
    yn = G.rays(size[0], h, P[1, 2], P[1, 1], np.float64)[:, None]
    back = 80.0 - 20.0 * xn + 0.0 * yn
    if not ground:
        d = back
    else:
        slope = yn + PLANE[0] * xn + PLANE[2]
        d = np.where(slope > CAMERA_HEIGHT / 80.0, CAMERA_HEIGHT / np.maximum(slope, 1e-9), back)
        for k, z in enumerate((9.0, 21.0)):                      # boxes: constant depth, from above the horizon down to their foot
            c0 = (w // 5, (3 * w) // 5)[k]
            foot = np.nonzero(d[:, c0] <= z)[0]
            r1 = int(foot[0]) if foot.size else h
            d[max(r1 - h // 4, 0):r1, c0:c0 + max(w // 8, 2)] = z
    d = d * (1.0 + sigma * rng.randn(h, w))
    return np.clip(d, 2.0, 90.0)


def to_map(d, s_true, input):
    d = d / s_true
    return ((1.0 / d - 0.01) / 10.0 if input == "disparity" else d).astype(np.float32)


SIZES3 = [(370, 1226), (375, 1242), (188, 620)]
# name: network (h, w), true sizes, dates, s_true, sigma, and the call's other arguments
SPECS = {
    "odd": dict(hw=(23, 37), sizes=SIZES3, dates=[0, 1, 0], s_true=[1.0, 0.37, 5.3], sigma=1e-3),
    "tiles": dict(hw=(48, 80), sizes=[(375, 1242), (370, 1226)], dates=[0, 1], s_true=[1.0, 5.3], sigma=1e-3),
    "full": dict(hw=(192, 640), sizes=[(375, 1242), (370, 1226)], dates=[0, 1], s_true=[1.0, 0.37], sigma=1e-4),
    "flat": dict(hw=(24, 40), sizes=[(375, 1242), (375, 1242)], dates=[0, 0], s_true=[1.0, 5.3], sigma=0.0),
    "noground": dict(hw=(24, 40), sizes=SIZES3, dates=[0, 1, 0], s_true=[1.0, 1.0, 0.37], sigma=1e-3, ground=[True, False, True]),
    "special": dict(hw=(24, 40), sizes=[(375, 1242), (370, 1226)], dates=[0, 1], s_true=[1.0, 0.37], sigma=1e-3, special=True),
    "box": dict(hw=(23, 37), sizes=SIZES3, dates=[0, 1, 0], s_true=[1.0, 0.37, 5.3], sigma=1e-3, box="lower"),
    "depth": dict(hw=(23, 37), sizes=SIZES3, dates=[0, 1, 0], s_true=[1.0, 0.37, 5.3], sigma=1e-3, input="depth"),
    "angle": dict(hw=(24, 40), sizes=[(375, 1242), (188, 620)], dates=[0, 1], s_true=[1.0, 5.3], sigma=1e-3, max_angle_deg=8.0,
                  camera_height=1.72),
}
# min_ground at the reference's own smallest count (every image valid) and one above it (that image falls back): built from "odd"
CASES = list(SPECS) + ["min_at", "min_above"]


def planted(h, w, seed):
    """three pixels on the ground (lower third, away from the border) for NaN, +inf and a negative disparity"""
    rng = np.random.RandomState(seed)
    rows = rng.choice(np.arange(h - h // 3, h - 2), 3, replace=False)
    cols = rng.choice(np.arange(2, w - 2), 3, replace=False)
    return list(zip(rows.tolist(), cols.tolist()))


@functools.lru_cache(maxsize=None)
def build(case):
    """-> dict: m [B, h, w] float32, sizes, P [B, 3, 4], T [B, 4, 4], s_true, sigma, valid (images with ground), and the keywords of
    ground_scale_ref.ground_scale (camera_height, max_angle_deg, boxes, min_ground, fallback, input)"""
    if case in ("min_at", "min_above"):
        a = dict(build("odd"))
        counts = reference("odd")[0][:, 2].astype(int)
        a["min_ground"] = int(counts.min()) + (case == "min_above")
        a["fallback"] = -3.0
        return a
    s = SPECS[case]
    h, w = s["hw"]
    B = len(s["sizes"])
    seed = 31 * (sorted(SPECS).index(case) + 1)
    input = s.get("input", "disparity")
    P = np.stack([scaled_P(DATES[k], H, W) for k, (H, W) in zip(s["dates"], s["sizes"])])
    ground = s.get("ground", [True] * B)
    m = np.stack([to_map(scene_depth(h, w, s["sizes"][b], P[b], s["sigma"], seed + b, ground[b]), s["s_true"][b], input) for b in range(B)])
    special = []
    if s.get("special"):
        for b in range(B):
            pts = planted(h, w, seed + 100 + b)
            for (r, c), val in zip(pts, (np.nan, np.inf, -0.05)):
                m[b, r, c] = val
            special.append(pts)
    boxes = None
    if s.get("box") == "lower":
        boxes = [(h // 2, h + 5, -2, w)] * B                     # reaches outside the plane: the call clamps it
    m.setflags(write=False)
    return dict(m=m, sizes=s["sizes"], P=P, T=np.stack([velo_T(DATES[k]) for k in s["dates"]]), s_true=s["s_true"], sigma=s["sigma"],
                valid=ground, special=special, camera_height=s.get("camera_height", CAMERA_HEIGHT),
                max_angle_deg=s.get("max_angle_deg", G.DEFAULT_ANGLE), boxes=boxes, min_ground=100, fallback=float("nan"), input=input)


def call_kw(a):
    return {k: a[k] for k in ("sizes", "P", "camera_height", "max_angle_deg", "boxes", "min_ground", "fallback", "input")}


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float32):
    """-> (rows [B, 4], mask uint8 [B, h, w], hgt [B, h, w], ny [B, h, w]); shared, do not write into it"""
    a = build(case)
    out = G.ground_scale(a["m"], dtype=dtype, **call_kw(a))
    for x in out:
        x.setflags(write=False)
    return out
