"""TEST INFRASTRUCTURE: the definition of the ground-plane scale estimator (include/mcav_depth.h: mcav_ground_scale; DNet's dense
geometrical constraint, Xue et al., IROS 2020) in numpy.  csrc/ground_math.h and the kernels of csrc/ground_scale.hip must match it bit
for bit with dtype=np.float32: every operation below is one numpy operation on arrays of that type, so each is rounded on its own, in
this order.  dtype=np.float64 evaluates the same definition in double as the arbiter (tests/test_ground_scale_cpu.py).

Per image b of m [B, h, w] (sigmoid disparity, or depth), true size (Hb, Wb) and P (3x4 float64):
  rays    xn[c] = (((c + 0.5) * Wb) / w - 0.5 - cu) / fu in float64, then rounded to dtype; yn[r] alike from Hb, h, cv, fv
  depth   d = 1 / (10 v + 0.01)    (or v);   point Pt = (xn d, yn d, d)
  normal  the eight differences to the neighbours R D L U DR DL UL UR, eight cross products of the pairs (R,D) (D,L) (L,U) (U,R) (DR,DL)
          (DL,UL) (UL,UR) (UR,DR), each normalised, summed in that order from +0, the sum normalised
  height  hgt = (n.x X + n.y Y) + n.z Z of the centre
  ground  every length finite and > 0, n.y >= cos_max, hgt finite and > 0, the pixel interior and inside the box
  row     scale = camera_height / median(hgt of the ground pixels), med, count, status; fallback below min_ground pixels
"""
import numpy as np

NEIGHBOURS = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1))       # R D L U DR DL UL UR as (dr, dc)
PAIRS = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4))
DEFAULT_ANGLE = 5.0


def cos_max_of(max_angle_deg):
    """the host float the call takes: cos of the cone's half angle, rounded to float32"""
    return np.float32(np.cos(np.deg2rad(np.float64(max_angle_deg))))


def rays(n_true, n_net, centre, focal, dtype=np.float32):
    """xn / yn of one axis: float64 in the stated order, rounded once to dtype"""
    i = np.arange(n_net, dtype=np.float64)
    return ((((i + 0.5) * np.float64(n_true)) / np.float64(n_net) - 0.5 - np.float64(centre)) / np.float64(focal)).astype(dtype)


def depth_of(v, input="disparity", dtype=np.float32):
    v = np.asarray(v).astype(dtype)
    if input == "depth":
        return v
    with np.errstate(all="ignore"):
        return dtype(1.0) / (dtype(10.0) * v + dtype(0.01))


def clamp_box(box, h, w):
    """[y0, y1) x [x0, x1) in network pixels as the kernels clamp it; None = everything"""
    if box is None:
        return 0, h, 0, w
    y0 = min(max(int(box[0]), 0), h)
    y1 = min(max(int(box[1]), y0), h)
    x0 = min(max(int(box[2]), 0), w)
    x1 = min(max(int(box[3]), x0), w)
    return y0, y1, x0, x1


def pixel_pass(v, size, P, cos_max=None, box=None, input="disparity", dtype=np.float32):
    """One image -> (mask bool [h, w], hgt dtype [h, w] (defined on the interior, 0 elsewhere), ny dtype [h, w])"""
    h, w = v.shape
    assert h >= 3 and w >= 3
    cos_max = cos_max_of(DEFAULT_ANGLE) if cos_max is None else np.float32(cos_max)
    P = np.asarray(P, np.float64).reshape(3, 4)
    xn = rays(size[1], w, P[0, 2], P[0, 0], dtype)
    yn = rays(size[0], h, P[1, 2], P[1, 1], dtype)
    d = depth_of(v, input, dtype)
    with np.errstate(all="ignore"):
        X, Y, Z = xn[None, :] * d, yn[:, None] * d, d
        ctr = (slice(1, h - 1), slice(1, w - 1))
        e = []
        for dr, dc in NEIGHBOURS:
            nb = (slice(1 + dr, h - 1 + dr), slice(1 + dc, w - 1 + dc))
            e.append((X[nb] - X[ctr], Y[nb] - Y[ctr], Z[nb] - Z[ctr]))
        acc = [np.zeros((h - 2, w - 2), dtype) for _ in range(3)]
        ok = np.ones((h - 2, w - 2), bool)
        for i, j in PAIRS:
            a, b = e[i], e[j]
            cx = a[1] * b[2] - a[2] * b[1]
            cy = a[2] * b[0] - a[0] * b[2]
            cz = a[0] * b[1] - a[1] * b[0]
            ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
            ok &= np.isfinite(ln) & (ln > 0)
            acc[0] = acc[0] + cx / ln
            acc[1] = acc[1] + cy / ln
            acc[2] = acc[2] + cz / ln
        L = np.sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2])
        ok &= np.isfinite(L) & (L > 0)
        nx, ny, nz = acc[0] / L, acc[1] / L, acc[2] / L
        hgt = (nx * X[ctr] + ny * Y[ctr]) + nz * Z[ctr]
        ok &= (ny >= dtype(cos_max)) & np.isfinite(hgt) & (hgt > 0)
    y0, y1, x0, x1 = clamp_box(box, h, w)
    inbox = np.zeros((h, w), bool)
    inbox[y0:y1, x0:x1] = True
    mask = np.zeros((h, w), bool)
    mask[ctr] = ok & inbox[ctr]
    H = np.zeros((h, w), dtype)
    H[ctr] = hgt
    N = np.zeros((h, w), dtype)
    N[ctr] = ny
    return mask, H, N


def median_of(values):
    """np.median of dtype values from the two middle order statistics: ranks floor((n-1)/2) and n/2, (a + b) / 2 in dtype"""
    s = np.sort(values)
    n = s.size
    return (s[(n - 1) // 2] + s[n // 2]) / s.dtype.type(2.0)


def image_row(mask, hgt, camera_height=1.65, min_ground=100, fallback=np.nan, dtype=np.float32):
    """-> [scale, med, count, status] as dtype"""
    vals = hgt[mask]
    n = int(vals.size)
    med = median_of(vals) if n else dtype(np.nan)
    if n >= min_ground:
        with np.errstate(all="ignore"):
            return np.array([dtype(camera_height) / med, med, n, 1], dtype)
    return np.array([fallback, med, n, 0], dtype)


def ground_scale(m, sizes=None, P=None, camera_height=1.65, max_angle_deg=DEFAULT_ANGLE, boxes=None, min_ground=100, fallback=np.nan,
                 input="disparity", dtype=np.float32, cos_max=None):
    """m [B, h, w]; sizes B pairs (default (h, w)); P [3, 4] or [B, 3, 4]; boxes None, one box or B boxes.
    -> rows [B, 4] dtype, mask uint8 [B, h, w], hgt [B, h, w], ny [B, h, w]"""
    m = np.asarray(m)
    B, h, w = m.shape
    sizes = [(h, w)] * B if sizes is None else [tuple(int(x) for x in s) for s in sizes]
    P = np.broadcast_to(np.asarray(P, np.float64), (B, 3, 4))
    if boxes is not None and np.ndim(boxes) == 1:
        boxes = [boxes] * B
    cm = cos_max_of(max_angle_deg) if cos_max is None else np.float32(cos_max)
    rows = np.zeros((B, 4), dtype)
    mask = np.zeros((B, h, w), np.uint8)
    hgt = np.zeros((B, h, w), dtype)
    ny = np.zeros((B, h, w), dtype)
    for b in range(B):
        mk, hgt[b], ny[b] = pixel_pass(m[b], sizes[b], P[b], cm, None if boxes is None else boxes[b], input, dtype)
        mask[b] = mk
        rows[b] = image_row(mk, hgt[b], camera_height, min_ground, fallback, dtype)
    return rows, mask, hgt, ny
