"""TEST INFRASTRUCTURE: the definition of oriented-box overlap and greedy suppression (include/mcav_depth.h: mcav_box_iou, mcav_box_nms;
pseudo_lidar.boxes_iou_bev, boxes_iou3d, nms) in numpy, one operation per rounding with the project's emulated fmaf (pfn_ref.fma32), an
independent float64 formulation to hold it against, and the greedy rule in plain Python over either.

    box      7 float32 (x, y, z, dx, dy, dz, heading); VALID iff all finite, MIN_EXTENT <= dx, dy, dz <= MAX_EXTENT, |heading| <= MAX_HEADING
    sincos   k = rint(h 2/pi) by fl(fmaf(h, 2/pi, 1.5 2^23) - 1.5 2^23); r = fmaf(k, -LO, fmaf(k, -MID, fmaf(k, -HI, h))); z = r r;
             s = fmaf(r z, fmaf(fmaf(S3, z, S2), z, S1), r); c = fmaf(z z, fmaf(fmaf(C3, z, C2), z, C1), fmaf(z, -0.5, 1)); quadrant k mod 4
    prepare  hx = dx / 2, hy = dy / 2; a = hx c, b = hy s, d = hx s, e = hy c; corners about the box's own centre, counter-clockwise:
             (a - b, d + e), (-(a + b), -(d - e)), (-(a - b), -(d + e)), (a + b, d - e); area = dx dy; vol = area dz;
             zlo = z - dz / 2, zhi = z + dz / 2; r = sqrt(fmaf(hy, hy, hx hx))
    inter    tx = Bx - Ax, ty = By - Ay; +0 unless fmaf(ty, ty, tx tx) <= ((rA + rB)^2) CIRCLE_SLACK; q = B's corners + (tx, ty);
             A's corners clipped against B's edges q0q1, q1q2, q2q3, q3q0: side(p) = fmaf(ex, py - q0y, -(ey (px - q0x))), e = q1 - q0;
             for vertex i with predecessor h (cyclic): if sides strictly opposite in sign, emit p_h + t (p_i - p_h) by fmaf, t = sp / (sp - sq);
             then emit p_i if side >= 0; a ninth vertex is dropped; fewer than 3 vertices: +0.  acc = sum in order of
             fmaf(x_i, y_j, -(x_j y_i)), j = i + 1 cyclic; area = acc / 2; +0 unless > 0; min(area, areaA, areaB)
    iou      bev: inter / ((areaA + areaB) - inter); 3d: i3 / ((volA + volB) - i3), i3 = min(inter * (min(zhi) - max(zlo)), volA, volB),
             +0 unless the intersection and the shared height are > 0
    nms      candidates: valid box and score >= score_thresh; order (score descending with -0.0 as +0.0, index ascending), the first pre_max;
             walked in order, kept iff no earlier kept row of the same class has iou(earlier, later) > iou_thresh; stop at post_max.

The float64 formulation (`inter_f64`, `iou_f64`) takes the same float32 boxes and does everything else in float64 in the ORIGINAL frame: float64
sin / cos, corners, a general convex clip against half-planes with an interpolated crossing, the shoelace sum; axis-aligned pairs (headings
0) have the exact closed form (`inter_axis_aligned`) which the tests hold it against.

THE BOUND on |inter - inter_f64| (`bound_inter`), u = 2^-24, r the half-diagonal, R = rA + rB, M = BOX_SINCOS_MAX_ULP:
  corners  c~ = c (1 + t), |t| <= 2 M u (M ulp, an ulp at most 2 u |c|).  x = fl(fl(hx c~) - fl(hy s~)) is off by at most
           (2 M + 1) u (hx |c| + hy |s|) + u |x| <= (2 M + 2) r u  (Cauchy-Schwarz: hx |c| + hy |s| <= r); a corner moves by at most
           eA = sqrt(2) (2 M + 2) rA u.  B's corners also take tx = fl(Bx - Ax) (u |tx|, |tx| <= 1.0001 R) and q = fl(p + tx) (u |q|,
           |q| <= R + rB): eB = sqrt(2) ((2 M + 2) rB + 3.0001 R) u.  The sincos share of both is 2 sqrt(2) M r u.
  area     a polygon whose vertices move by at most e changes by at most e perimeter + pi e^2 in area (Steiner), and so does its
           intersection with anything: T_in = eA perA + eB perB, per = 2 (dx + dy), (the squares are below 1e-6 of that: a 1.001 covers them).
  clip     the clip's own arithmetic (side tests, crossings, shoelace; every coordinate is at most 2 R here because of the translation)
           is NOT derived.  It was measured on this CPU against inter_f64 over every pair of tests/box_cases.py (the indication was
           "a plain float32 clip stays under 1.7 u R^2"): the largest |inter - inter_f64| / (u R^2) found was 1.732 (a box against
           itself turned by a quarter) -- that figure still contains the derived terms --, and the committed term is C_CLIP u R^2
           with C_CLIP = 7 = 4 x 1.732 rounded up.
  =>       |inter - inter_f64| <= min(1.001 T_in + C_CLIP u R^2, min(areaA, areaB))        (both lie in [0, min area])
and on the overlap (`bound_iou`), with b the bound above, U = areaA + areaB - inter_f64 >= max area, and (areaA + areaB) / U <= 2:
  bev      |iou - iou_f64| <= 2 b / (U - b) + 8 u     (areas 1 rounding each, the sum 2, the division 1, with iou <= 1)
  3d       b3 = b h + inter_f64 dh + u inter_f64 h, dh = u (|zloA| + |zhiA| + |zloB| + |zhiB| + h) (the four z ends and the difference);
           |iou - iou_f64| <= 2 b3 / (U3 - b3) + 10 u, U3 = volA + volB - i3_f64
`mutant=` builds the wrong definitions the tests must tell from the right one (MUTANTS).
"""
import numpy as np

import pfn_ref

F = np.float32
U = 2.0 ** -24
MIN_EXTENT, MAX_EXTENT, MAX_HEADING, CIRCLE_SLACK = F(1e-3), F(1024.0), F(32.0), F(1.0001)
BOX_SINCOS_MAX_ULP = 1.5625                                 # csrc/box_math.h; test_box_cpu.py compares the two
NMS_MAX_CANDIDATES = 4096
SC_TWO_OVER_PI, SC_ROUND = F(0.6366197466850281), F(12582912.0)
SC_PIO2 = (F(1.5707969665527344), F(-6.397578431460715e-07), F(5.390302953474238e-15))
SC_S = (F(-1.6666654611e-1), F(8.3321608736e-3), F(-1.9515295891e-4))
SC_C = (F(4.166664568298827e-2), F(-1.388731625493765e-3), F(2.443315711809948e-5))
C_CLIP = 7.0
MODES = {"bev": 0, "3d": 1}
PAIR_MUTANTS = ("heading-sign", "dx-dy-swapped", "no-translation", "no-clamp", "union-without-inter")
RULE_MUTANTS = (">=", "all-earlier", "index-descending", "classes-ignored")
MUTANTS = PAIR_MUTANTS + RULE_MUTANTS

fma = pfn_ref.fma32


def valid(b):
    b = np.asarray(b, F).reshape(-1, 7)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(b).all(axis=1) & (b[:, 3:6] >= MIN_EXTENT).all(axis=1) & (b[:, 3:6] <= MAX_EXTENT).all(axis=1)
                & (np.abs(b[:, 6]) <= MAX_HEADING))


def box_sincos(h):
    """csrc/box_math.h box_sincos, bit for bit: float32 in, (sin, cos) float32 out, for |h| <= MAX_HEADING"""
    h = np.atleast_1d(np.asarray(h, F))
    kf = (fma(h, SC_TWO_OVER_PI, SC_ROUND) - SC_ROUND).astype(F)
    r = h
    for part in SC_PIO2:
        r = fma(kf, -part, r)
    z = (r * r).astype(F)
    s = fma((r * z).astype(F), fma(fma(SC_S[2], z, SC_S[1]), z, SC_S[0]), r)
    c = fma((z * z).astype(F), fma(fma(SC_C[2], z, SC_C[1]), z, SC_C[0]), fma(z, F(-0.5), F(1.0)))
    k = kf.astype(np.int64) & 3
    sn = np.where(k == 0, s, np.where(k == 1, c, np.where(k == 2, -s, -c))).astype(F)
    cs = np.where(k == 0, c, np.where(k == 1, -s, np.where(k == 2, -c, s))).astype(F)
    return sn, cs


def prepare(boxes, mutant=None):
    """csrc/box_math.h prepare over rows -> dict of float32 arrays (px, py [n, 4]); an invalid row is all zeros"""
    b = np.asarray(boxes, F).reshape(-1, 7)
    ok = valid(b)
    v = np.where(ok[:, None], b, F(0.0)).astype(F)
    if mutant == "dx-dy-swapped":
        v = v[:, [0, 1, 2, 4, 3, 5, 6]]
    s, c = box_sincos(-v[:, 6] if mutant == "heading-sign" else v[:, 6])
    hx, hy, hz = v[:, 3] * F(0.5), v[:, 4] * F(0.5), v[:, 5] * F(0.5)
    a, bb, d, e = hx * c, hy * s, hx * s, hy * c
    px0, py0, px3, py3 = a - bb, d + e, a + bb, d - e
    area = v[:, 3] * v[:, 4]
    p = dict(cx=v[:, 0], cy=v[:, 1], zlo=v[:, 2] - hz, zhi=v[:, 2] + hz, px=np.stack([px0, -px3, -px0, px3], 1), py=np.stack([py0, -py3, -py0, py3], 1),
             area=area, vol=area * v[:, 5], r=np.sqrt(fma(hy, hy, hx * hx)), ok=ok.astype(F), c=c, s=s, hx=hx, hy=hy)
    for key, val in p.items():
        p[key] = np.where(ok.reshape((-1,) + (1,) * (val.ndim - 1)), val, F(0.0)).astype(F)
    return p


def take(p, idx):
    return {k: v[idx] for k, v in p.items()}


def _clip(x, y, n, qx, qy):
    """Sutherland-Hodgman of the polygons (x, y)[:, :n] against the four edges of (qx, qy), all float32, as the header does it"""
    rows = np.arange(len(n))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(4):
            q0x, q0y = qx[:, k], qy[:, k]
            ex, ey = qx[:, (k + 1) & 3] - q0x, qy[:, (k + 1) & 3] - q0y
            sd = fma(ex[:, None], y - q0y[:, None], -(ey[:, None] * (x - q0x[:, None])))
            nx, ny, m = np.zeros_like(x), np.zeros_like(y), np.zeros_like(n)
            for i in range(8):
                live = i < n
                h = np.where(i == 0, n - 1, i - 1) % 8
                sp, sq = sd[rows, h], sd[:, i]
                cross = live & (((sp > 0) & (sq < 0)) | ((sp < 0) & (sq > 0)))
                t = (sp / (sp - sq)).astype(F)
                cx, cy = fma(t, x[:, i] - x[rows, h], x[rows, h]), fma(t, y[:, i] - y[rows, h], y[rows, h])
                put = cross & (m < 8)
                nx[rows[put], m[put]], ny[rows[put], m[put]] = cx[put], cy[put]
                m = m + cross                                # the header counts only what it stores: m stays <= 8 below
                m = np.minimum(m, 8)
                put = live & (sq >= 0) & (m < 8)
                nx[rows[put], m[put]], ny[rows[put], m[put]] = x[put, i], y[put, i]
                m = m + put
            n = np.where(m < 3, 0, m)
            x, y = nx, ny
    return x, y, n


def inter_bev(pa, pb, mutant=None):
    """csrc/box_math.h inter_bev on pairs of prepared rows (dicts of equal length) -> float32 [n]"""
    count = len(pa["cx"])
    out = np.zeros(count, F)
    with np.errstate(invalid="ignore", over="ignore"):
        if mutant == "no-translation":
            tx, ty = pb["cx"] - pa["cx"], pb["cy"] - pa["cy"]
        else:
            tx, ty = (pb["cx"] - pa["cx"]).astype(F), (pb["cy"] - pa["cy"]).astype(F)
        rr = pa["r"] + pb["r"]
        near = (pa["ok"] > 0) & (pb["ok"] > 0) & (fma(ty, ty, tx * tx) <= (rr * rr) * CIRCLE_SLACK)
    idx = np.nonzero(near)[0]
    if len(idx) == 0:
        return out
    A, B = take(pa, idx), take(pb, idx)
    if mutant == "no-translation":                            # both quadrilaterals in the original frame
        x = np.concatenate([A["px"] + A["cx"][:, None], np.zeros((len(idx), 4), F)], 1).astype(F)
        y = np.concatenate([A["py"] + A["cy"][:, None], np.zeros((len(idx), 4), F)], 1).astype(F)
        qx, qy = (B["px"] + B["cx"][:, None]).astype(F), (B["py"] + B["cy"][:, None]).astype(F)
    else:
        x = np.concatenate([A["px"], np.zeros((len(idx), 4), F)], 1)
        y = np.concatenate([A["py"], np.zeros((len(idx), 4), F)], 1)
        qx, qy = (B["px"] + tx[idx, None]).astype(F), (B["py"] + ty[idx, None]).astype(F)
    x, y, n = _clip(x, y, np.full(len(idx), 4, np.int64), qx, qy)
    rows = np.arange(len(idx))
    acc = np.zeros(len(idx), F)
    for i in range(8):
        j = np.where(i + 1 == n, 0, i + 1) % 8
        term = fma(x[:, i], y[rows, j], -(x[rows, j] * y[:, i]))
        acc = np.where(i < n, acc + term, acc).astype(F)
    area = acc * F(0.5)
    if mutant != "no-clamp":
        area = np.minimum(area, np.minimum(A["area"], B["area"]))
    out[idx] = np.where((area > 0) & (n >= 3), area, F(0.0))
    return out


def iou(pa, pb, mode, mutant=None):
    """csrc/box_math.h iou on pairs of prepared rows -> float32 [n]"""
    inter = inter_bev(pa, pb, mutant)
    with np.errstate(invalid="ignore", divide="ignore"):
        if MODES.get(mode, mode) == 0:
            union = (pa["area"] + pb["area"]) if mutant == "union-without-inter" else (pa["area"] + pb["area"]) - inter
            return np.where(inter > 0, inter / union, F(0.0)).astype(F)
        h = np.minimum(pa["zhi"], pb["zhi"]) - np.maximum(pa["zlo"], pb["zlo"])
        i3 = np.where((inter > 0) & (h > 0), inter * h, F(0.0)).astype(F)
        if mutant != "no-clamp":
            i3 = np.minimum(i3, np.minimum(pa["vol"], pb["vol"]))
        union = (pa["vol"] + pb["vol"]) if mutant == "union-without-inter" else (pa["vol"] + pb["vol"]) - i3
        return np.where(i3 > 0, i3 / union, F(0.0)).astype(F)


def pairs_iou(a, b, mode, mutant=None):
    """row i of a against row i of b -> (inter, iou) float32"""
    pa, pb = prepare(a, mutant), prepare(b, mutant)
    return inter_bev(pa, pb, mutant), iou(pa, pb, mode, mutant)


def iou_matrix(a, b, mode):
    """mcav_box_iou: [na, nb] float32"""
    pa, pb = prepare(a), prepare(b)
    na, nb = len(pa["cx"]), len(pb["cx"])
    i, j = np.repeat(np.arange(na), nb), np.tile(np.arange(nb), na)
    return iou(take(pa, i), take(pb, j), mode).reshape(na, nb)


# ---------------------------------------------------------------------------------------------- float64 formulation
def corners_f64(b):
    b = np.asarray(b, F).astype(np.float64).reshape(-1, 7)
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    sx, sy = np.array([1.0, -1.0, -1.0, 1.0]), np.array([1.0, 1.0, -1.0, -1.0])
    lx, ly = sx[None] * b[:, 3:4] / 2, sy[None] * b[:, 4:5] / 2
    return b[:, 0:1] + lx * c[:, None] - ly * s[:, None], b[:, 1:2] + lx * s[:, None] + ly * c[:, None]


def inter_f64(a, b):
    """area of the intersection of the two rectangles of every pair, float64, in the original frame: a general clip of a convex polygon
    (lists of vertices per pair) against B's four half-planes, crossings by linear interpolation of the signed distances"""
    a, b = np.asarray(a, F).reshape(-1, 7), np.asarray(b, F).reshape(-1, 7)
    ok = valid(a) & valid(b)
    ax, ay = corners_f64(np.where(ok[:, None], a, F(1.0)))
    bx, by = corners_f64(np.where(ok[:, None], b, F(1.0)))
    out = np.zeros(len(a))
    ra = np.hypot(a[:, 3].astype(np.float64), a[:, 4].astype(np.float64)) / 2
    rb = np.hypot(b[:, 3].astype(np.float64), b[:, 4].astype(np.float64)) / 2
    with np.errstate(invalid="ignore", over="ignore"):
        far = np.hypot(a[:, 0].astype(np.float64) - b[:, 0], a[:, 1].astype(np.float64) - b[:, 1]) > (ra + rb) * (1 + 1e-9)
    for i in np.nonzero(ok & ~far)[0]:
        poly = list(zip(ax[i], ay[i]))
        for k in range(4):
            q0, q1 = (bx[i, k], by[i, k]), (bx[i, (k + 1) % 4], by[i, (k + 1) % 4])
            ex, ey = q1[0] - q0[0], q1[1] - q0[1]
            dist = [ex * (p[1] - q0[1]) - ey * (p[0] - q0[0]) for p in poly]
            new = []
            for j, p in enumerate(poly):
                h = j - 1
                sp, sq = dist[h], dist[j]
                if (sp > 0 > sq) or (sp < 0 < sq):
                    t = sp / (sp - sq)
                    new.append((poly[h][0] + t * (p[0] - poly[h][0]), poly[h][1] + t * (p[1] - poly[h][1])))
                if sq >= 0:
                    new.append(p)
            poly = new
            if len(poly) < 3:
                break
        if len(poly) >= 3:
            x0, y0 = poly[0]
            acc = 0.0
            for j in range(1, len(poly) - 1):
                acc += (poly[j][0] - x0) * (poly[j + 1][1] - y0) - (poly[j + 1][0] - x0) * (poly[j][1] - y0)
            out[i] = max(acc / 2, 0.0)
    return out


def inter_axis_aligned(a, b):
    """the exact intersection area of pairs whose headings are 0: the product of the two interval overlaps, float64"""
    a, b = np.asarray(a, F).astype(np.float64).reshape(-1, 7), np.asarray(b, F).astype(np.float64).reshape(-1, 7)
    w = np.minimum(a[:, 0] + a[:, 3] / 2, b[:, 0] + b[:, 3] / 2) - np.maximum(a[:, 0] - a[:, 3] / 2, b[:, 0] - b[:, 3] / 2)
    h = np.minimum(a[:, 1] + a[:, 4] / 2, b[:, 1] + b[:, 4] / 2) - np.maximum(a[:, 1] - a[:, 4] / 2, b[:, 1] - b[:, 4] / 2)
    return np.maximum(w, 0) * np.maximum(h, 0)


def iou_f64(a, b, mode):
    """-> dict(inter, iou, bound_inter, bound_iou), float64 [n]: the float64 formulation of every pair and THE BOUND of the docstring"""
    a, b = np.asarray(a, F).reshape(-1, 7), np.asarray(b, F).reshape(-1, 7)
    ok = valid(a) & valid(b)
    A, B = np.where(ok[:, None], a, F(1.0)).astype(np.float64), np.where(ok[:, None], b, F(1.0)).astype(np.float64)
    inter = inter_f64(a, b)
    sa, sb = A[:, 3] * A[:, 4], B[:, 3] * B[:, 4]
    ra, rb = np.hypot(A[:, 3], A[:, 4]) / 2, np.hypot(B[:, 3], B[:, 4]) / 2
    R, M = ra + rb, BOX_SINCOS_MAX_ULP
    ea, eb = np.sqrt(2) * (2 * M + 2) * ra * U, np.sqrt(2) * ((2 * M + 2) * rb + 3.0001 * R) * U
    t_in = ea * 2 * (A[:, 3] + A[:, 4]) + eb * 2 * (B[:, 3] + B[:, 4])
    bi = np.minimum(1.001 * t_in + C_CLIP * U * R * R, np.minimum(sa, sb))
    if MODES.get(mode, mode) == 0:
        union = sa + sb - inter
        val = inter / union
        bound = 2 * bi / np.maximum(union - bi, 1e-300) + 8 * U
    else:
        zlo_a, zhi_a, zlo_b, zhi_b = A[:, 2] - A[:, 5] / 2, A[:, 2] + A[:, 5] / 2, B[:, 2] - B[:, 5] / 2, B[:, 2] + B[:, 5] / 2
        h = np.maximum(np.minimum(zhi_a, zhi_b) - np.maximum(zlo_a, zlo_b), 0.0)
        dh = U * (np.abs(zlo_a) + np.abs(zhi_a) + np.abs(zlo_b) + np.abs(zhi_b) + h)
        i3 = inter * h
        b3 = bi * h + inter * dh + U * i3
        union = sa * A[:, 5] + sb * B[:, 5] - i3
        val = i3 / union
        bound = 2 * b3 / np.maximum(union - b3, 1e-300) + 10 * U
    return dict(inter=np.where(ok, inter, 0.0), iou=np.where(ok, val, 0.0), bound_inter=np.where(ok, bi, 0.0), bound_iou=np.where(ok, bound, 0.0))


# ---------------------------------------------------------------------------------------------- the greedy rule
def order_of(boxes, scores, score_thresh, pre_max, mutant=None):
    """one image: the candidates' anchor indices in the order walked, cut at pre_max"""
    scores = np.asarray(scores, F)
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(valid(boxes) & (scores >= F(score_thresh)))[0]
    s = scores[cand] + F(0.0)                                # -0.0 -> +0.0
    tie = -cand if mutant == "index-descending" else cand
    return cand[np.lexsort((tie, -s.astype(np.float64)))][:pre_max]


def overlaps(boxes, order, mode, f64=False):
    """the pairs (i, j), i < j positions in `order`, that can overlap at all, and their iou(earlier, later): float32 restatement, or the
    float64 formulation with its bound -> (i, j, iou[, bound])"""
    b = np.asarray(boxes, F).reshape(-1, 7)[order]
    n = len(b)
    r = np.hypot(b[:, 3].astype(np.float64), b[:, 4].astype(np.float64)) / 2
    ii, jj = [], []
    for lo in range(0, n, 256):                               # a float64 prefilter wider than the definition's circle test
        d = np.hypot(b[lo:lo + 256, None, 0].astype(np.float64) - b[None, :, 0], b[lo:lo + 256, None, 1].astype(np.float64) - b[None, :, 1])
        i, j = np.nonzero(d <= (r[lo:lo + 256, None] + r[None, :]) * 1.001)
        keep = lo + i < j
        ii.append(lo + i[keep])
        jj.append(j[keep])
    i, j = (np.concatenate(ii), np.concatenate(jj)) if ii else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    if f64:
        ref = iou_f64(b[i], b[j], mode)
        return i, j, ref["iou"], ref["bound_iou"]
    p = prepare(b)
    return i, j, iou(take(p, i), take(p, j), mode)


def greedy(n, i, j, value, iou_thresh, classes=None, post_max=None, mutant=None):
    """the walk over n ordered candidates given the sparse overlaps (i < j, value): -> the kept positions.  classes: per position"""
    hit = value >= iou_thresh if mutant == ">=" else value > iou_thresh
    if classes is not None and mutant != "classes-ignored":
        hit = hit & (classes[i] == classes[j])
    killers = [[] for _ in range(n)]
    for a, b in zip(i[hit].tolist(), j[hit].tolist()):
        killers[b].append(a)
    alive, kept = np.zeros(n, bool), []
    for k in range(n):
        if post_max is not None and len(kept) >= post_max:
            break
        if mutant == "all-earlier":
            dead = len(killers[k]) > 0
        else:
            dead = any(alive[a] for a in killers[k])
        if not dead:
            alive[k] = True
            kept.append(k)
    return np.array(kept, np.int64)


def nms(boxes, scores, classes=None, score_thresh=0.1, iou_thresh=0.01, pre_max=4096, post_max=500, mode="bev", f64=False, mutant=None):
    """mcav_box_nms on [B, A, 7], [B, A], [B, A] -> dict(keep [B, post_max] int32, num [B] int32, boxes, scores float32); f64: the float64
    rule (the kept sets must be the restatement's wherever check_non_trivial holds)"""
    boxes, scores = np.asarray(boxes, F), np.asarray(scores, F)
    B, A = scores.shape
    keep, num = np.full((B, post_max), -1, np.int32), np.zeros(B, np.int32)
    out_boxes, out_scores = np.zeros((B, post_max, 7), F), np.zeros((B, post_max), F)
    for b in range(B):
        order = order_of(boxes[b], scores[b], score_thresh, pre_max, mutant)
        found = overlaps(boxes[b], order, mode, f64)
        cls = None if classes is None else np.asarray(classes)[b][order]
        kept = order[greedy(len(order), found[0], found[1], found[2], F(iou_thresh) if not f64 else float(F(iou_thresh)), cls, post_max, mutant)]
        num[b] = len(kept)
        keep[b, :len(kept)] = kept
        out_boxes[b, :len(kept)], out_scores[b, :len(kept)] = boxes[b][kept], scores[b][kept]
    return dict(keep=keep, num=num, boxes=out_boxes, scores=out_scores)
