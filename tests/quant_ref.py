"""TEST INFRASTRUCTURE: the definition of the soft-occupancy grid (include/mcav_depth.h: mcav_cloud_occupancy, mcav_cloud_occupancy_bwd;
pseudo_lidar.occupancy) in numpy, one operation per rounding, and a plain float64 formulation to hold it against.

    points [n_max, 4] float32 (x, y, z, i), offsets int32 [B + 1]: image b owns rows offsets[b] .. offsets[b+1]; n = min(offsets[B], n_max);
    rows at and beyond n are never read.
    cell     pillar_ref's rule on three axes: f = floor((v - origin) / size) in float32; kept iff 0 <= f < cells on every axis, compared as
             floats (NaN and +-inf drop out, -0.0 is 0).  n(m') = the kept points of an image in cell m'.
    centre   pillar_ref.centre: (float)i * size + (size * 0.5 + origin), float32
    term     for a kept point of cell m' and a cell m of the 3 x 3 x 3 block around m' inside the grid: dx = x - cx(m), dy, dz (float32);
             d2 = dx * dx; d2 = fmaf(dy, dy, d2); d2 = fmaf(dz, dz, d2); t = -(d2 / sigma2); e = quant_exp(t)
    sum      q = rint(float64(e) * 2^40 / float64(n(m') * (1 if m == m' else 26))) as an integer; S(m) = the integer sum of q;
             canvas[b, iz, iy, ix] = float32(float64(S(m)) * 2^-40)
    record   point_count[i] = n(m') for a kept row below n, 0 for a dropped one
    backward d_points[i][a] = float32 of the float64 sum, over the block's cells in ascending (dz, dy, dx) order from +0, of
             ((g(m) * (w / n)) * e) * ((-2 * d_a) / sigma2), w = 1 or 1 / 26; column 3, dropped rows and rows at and beyond n: +0.0

The float64 formulation (`occupancy_f64`, `occupancy_bwd_f64`) keeps the cells, the counts and the float32 centres and sigma2 and replaces
everything else by float64 arithmetic: D = p - c, T = -|D|^2 / sigma2, E = exp(T), V(m) = sum (w / n) E, and the analytic gradient
sum g (w / n) E (-2 D_a / sigma2).  THE BOUND between the two, with u = 2^-24, derived and not fitted:
    dx = fl(x - cx) = Dx (1 + d), |d| <= u.  Each square is then off by at most (1 + u)^2 - 1; d2 takes three more roundings (the
    product and the two fmaf), each of a partial sum of non-negative numbers that is at most the total: d2 = |D|^2 (1 + a),
    |a| <= (1 + u)^5 - 1.  The division rounds once more: t = T (1 + b), |b| <= (1 + u)^6 - 1 =: r6 (6.000002 u).
    exp(t) = E exp(T b): off from E by at most E expm1(|T| r6).  quant_exp(t) is within QEXP_MAX_ULP ulp of exp(t), and an ulp of v is at
    most 2^-23 v = 2 u v: e = E (1 + c), |c| <= rel(T) := (1 + expm1(|T| r6)) (1 + 2 QEXP_MAX_ULP u) - 1, about (6 |T| + 1.875) u.
    Below the cut-off (t < QEXP_CUT) e is +0 and the error is E itself: rel = 1 there.
    q 2^-40 differs from e / den by the float64 division's rounding (2^-53, relative) and by half a unit of rint: 2^-41 per term.  The
    integer sum is exact, S 2^-40 is exact in float64 (S < 2^42), the store rounds once: u, relative.
    => |canvas(m) - V(m)| <= A + u (V + A) + 2^-40 V,  A = sum over the terms on m of (w / n) E (rel(T) + 2^-52) + 2^-41 per term;
       the last summand covers the float64 formulation's own roundings (a few 2^-53 per term).
    For sigma2 = 0.01 on 0.1 m cells |T| <= 6.75 and rel <= 42.4 u: the "about 40 x 2^-24 of the sum of the terms' magnitudes plus 2^-41
    per term" one expects.
    The backward multiplies e by dx: e d_a = E D_a (1 + c)(1 + d), so a term is off by at most its magnitude times rel(T) + u (1 + rel(T));
    the factors are exact promotions and every float64 operation adds 2^-53: 2^-50 per term covers the six of them.  The store rounds
    once.  => |d_points - G| <= A' + u (|G| + A'),  A' = sum |g| (w / n) E |2 D_a / sigma2| (rel(T) + u (1 + rel(T)) + 2^-50).
`mutant=` builds the wrong definitions the tests must tell from the right one (tests/quant_cases.py MUTANTS).
"""
import collections

import numpy as np

import pfn_ref
import pillar_ref as PR

F = np.float32
U = 2.0 ** -24
Grid = collections.namedtuple("Grid", "x0 y0 z0 vx vy vz nx ny nz")

QEXP_CUT = F(-87.0)
QEXP_MAX_ULP = 0.9375                                        # csrc/quant_math.h; test_quant_cpu.py compares the two
QEXP_LOG2E, QEXP_LN2_HI, QEXP_LN2_LO, QEXP_ROUND = F(1.44269504088896341), F(0.693359375), F(-2.12194440e-4), F(12582912.0)
QEXP_COEFFS = [F(1.0) / F(d) for d in (5040.0, 720.0, 120.0, 24.0, 6.0)] + [F(0.5), F(1.0), F(1.0)]
FIXED_ONE = 2.0 ** 40
OFFSETS = [(oz, oy, ox) for oz in (-1, 0, 1) for oy in (-1, 0, 1) for ox in (-1, 0, 1)]      # ascending (dz, dy, dx)
MUTANTS = ("weight-1/27", "count-of-target", "no-own-term", "border-neighbours", "half-sigma", "backward-without-2")


def make_grid(x=(0.0, 70.0), y=(-40.0, 40.0), z=(-2.5, 1.0), size=(0.1, 0.1, 0.1)):
    """PIXOR's grid by default: 700 x 800 x 35.  Cells per axis = round((hi - lo) / size) in float64; the kernel's scalars are float32."""
    n = [int(np.round((np.float64(r[1]) - np.float64(r[0])) / np.float64(s))) for r, s in zip((x, y, z), size)]
    return Grid(F(x[0]), F(y[0]), F(z[0]), F(size[0]), F(size[1]), F(size[2]), n[0], n[1], n[2])


def quant_exp(t):
    """csrc/quant_math.h quant_exp, bit for bit: float32 in, float32 out; t below the cut-off (or NaN) gives +0"""
    t = np.atleast_1d(np.asarray(t, F))
    with np.errstate(invalid="ignore"):
        live = t >= QEXP_CUT
    ts = np.where(live, t, F(0.0)).astype(F)
    kf = (pfn_ref.fma32(ts, QEXP_LOG2E, QEXP_ROUND) - QEXP_ROUND).astype(F)
    r = pfn_ref.fma32(kf, -QEXP_LN2_HI, ts)
    r = pfn_ref.fma32(kf, -QEXP_LN2_LO, r)
    p = np.full(ts.shape, QEXP_COEFFS[0], F)
    for c in QEXP_COEFFS[1:]:
        p = pfn_ref.fma32(p, r, c)
    bits = p.view(np.uint32).astype(np.int64) + (kf.astype(np.int64) << 23)
    return np.where(live, bits.astype(np.uint32).view(F), F(0.0)).astype(F)


def cells_of(points, grid):
    """-> ix, iy, iz (int64) and the keep mask, per row"""
    ix, okx = PR.axis_cells(points[:, 0], grid.x0, grid.vx, grid.nx)
    iy, oky = PR.axis_cells(points[:, 1], grid.y0, grid.vy, grid.ny)
    iz, okz = PR.axis_cells(points[:, 2], grid.z0, grid.vz, grid.nz)
    return ix, iy, iz, okx & oky & okz


def located(points, offsets, grid):
    """the kept rows below n: dict(rows, b, ix, iy, iz, count) with count = n(m') per kept row, and n"""
    points = np.asarray(points, F)
    n = PR.live_rows(points, offsets)
    ix, iy, iz, keep = cells_of(points[:n], grid)
    rows = np.nonzero(keep)[0]
    b = PR.image_of(np.asarray(offsets), rows.astype(np.int64))
    ix, iy, iz = ix[rows], iy[rows], iz[rows]
    table = np.zeros((len(offsets) - 1, grid.nz, grid.ny, grid.nx), np.int64)
    np.add.at(table, (b, iz, iy, ix), 1)
    return dict(rows=rows, b=b, ix=ix, iy=iy, iz=iz, count=table[b, iz, iy, ix], table=table), n


def neighbour(loc, grid, off):
    """the cells at offset (oz, oy, ox) from every kept row's own: jx, jy, jz and which of them lie inside the grid"""
    jz, jy, jx = loc["iz"] + off[0], loc["iy"] + off[1], loc["ix"] + off[2]
    inside = (jx >= 0) & (jx < grid.nx) & (jy >= 0) & (jy < grid.ny) & (jz >= 0) & (jz < grid.nz)
    return jx, jy, jz, inside


def term32(p, jx, jy, jz, grid, sigma2):
    """-> e, (dx, dy, dz), t: float32, as the header's term()"""
    d = [(p[:, a] - PR.centre(j, o, s)).astype(F) for a, (j, o, s) in
         enumerate(((jx, grid.x0, grid.vx), (jy, grid.y0, grid.vy), (jz, grid.z0, grid.vz)))]
    d2 = (d[0] * d[0]).astype(F)
    d2 = pfn_ref.fma32(d[1], d[1], d2)
    d2 = pfn_ref.fma32(d[2], d[2], d2)
    with np.errstate(over="ignore"):
        t = (-(d2 / F(sigma2)).astype(F)).astype(F)
    return quant_exp(t), d, t


def occupancy(points, offsets, grid, sigma2=0.01):
    """-> dict(canvas float32 [B, nz, ny, nx], point_count int32 [n], S int64 [B, nz, ny, nx]); point_count covers the rows below n"""
    points = np.asarray(points, F)
    loc, n = located(points, offsets, grid)
    B = len(offsets) - 1
    S = np.zeros((B, grid.nz, grid.ny, grid.nx), np.int64)
    p = points[loc["rows"]]
    for off in OFFSETS:
        jx, jy, jz, inside = neighbour(loc, grid, off)
        e, _, _ = term32(p[inside], jx[inside], jy[inside], jz[inside], grid, sigma2)
        den = (loc["count"][inside] * (1 if off == (0, 0, 0) else 26)).astype(np.float64)
        q = np.rint(e.astype(np.float64) * FIXED_ONE / den).astype(np.int64)
        np.add.at(S, (loc["b"][inside], jz[inside], jy[inside], jx[inside]), q)
    count = np.zeros(n, np.int32)
    count[loc["rows"]] = loc["count"]
    return dict(canvas=(S.astype(np.float64) * 2.0 ** -40).astype(F), point_count=count, S=S)


def occupancy_bwd(points, offsets, point_count, d_canvas, grid, sigma2=0.01):
    """-> d_points float32 [n_max, 4].  point_count: what the forward recorded (its rows below n)"""
    points, g = np.asarray(points, F), np.asarray(d_canvas, F)
    loc, n = located(points, offsets, grid)
    p = points[loc["rows"]]
    cnt = np.asarray(point_count)[loc["rows"]].astype(np.float64)
    acc = np.zeros((len(loc["rows"]), 3), np.float64)
    s2 = np.float64(F(sigma2))
    for off in OFFSETS:
        jx, jy, jz, inside = neighbour(loc, grid, off)
        e, d, _ = term32(p[inside], jx[inside], jy[inside], jz[inside], grid, sigma2)
        w = 1.0 if off == (0, 0, 0) else 1.0 / 26.0
        c = (g[loc["b"][inside], jz[inside], jy[inside], jx[inside]].astype(np.float64) * (w / cnt[inside])) * e.astype(np.float64)
        for a in range(3):
            acc[inside, a] = acc[inside, a] + c * ((-2.0 * d[a].astype(np.float64)) / s2)
    out = np.zeros((points.shape[0], 4), F)
    out[loc["rows"], :3] = acc.astype(F)
    return out


# ---------------------------------------------------------------------------------------------- the float64 formulation and the bound
def rel_of(T, t32):
    """rel(T) of the docstring, per term"""
    r6 = (1.0 + U) ** 6 - 1.0
    rel = (1.0 + np.expm1(np.abs(T) * r6)) * (1.0 + 2.0 * QEXP_MAX_ULP * U) - 1.0
    with np.errstate(invalid="ignore"):
        return np.where(t32 < QEXP_CUT, 1.0, rel)


def _terms64(points, offsets, grid, sigma2, mutant=None):
    """every term of the float64 formulation: yields (inside rows' selection, b, jx, jy, jz, weight / count, E, D [3], rel)"""
    points = np.asarray(points, F)
    loc, n = located(points, offsets, grid)
    p = points[loc["rows"]]
    s2 = np.float64(F(sigma2)) * (2.0 if mutant == "half-sigma" else 1.0)
    for off in OFFSETS:
        own = off == (0, 0, 0)
        if own and mutant == "no-own-term":
            continue
        jx, jy, jz, inside = neighbour(loc, grid, off)
        sel = np.nonzero(inside)[0]
        b, jx, jy, jz = loc["b"][sel], jx[sel], jy[sel], jz[sel]
        D = [p[sel, a].astype(np.float64) - PR.centre(j, o, s).astype(np.float64) for a, (j, o, s) in
             enumerate(((jx, grid.x0, grid.vx), (jy, grid.y0, grid.vy), (jz, grid.z0, grid.vz)))]
        T = -(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]) / s2
        _, _, t32 = term32(p[sel], jx, jy, jz, grid, sigma2)
        count = loc["table"][b, jz, jy, jx] if mutant == "count-of-target" and not own else loc["count"][sel]
        if own:
            w = np.ones(len(sel))
        elif mutant == "weight-1/27":
            w = np.full(len(sel), 1.0 / 27.0)
        elif mutant == "border-neighbours":              # |N_m| = the neighbours of the TARGET cell that lie inside the grid
            span = lambda j, m: np.minimum(j + 1, m - 1) - np.maximum(j - 1, 0) + 1
            w = 1.0 / np.maximum(span(jx, grid.nx) * span(jy, grid.ny) * span(jz, grid.nz) - 1, 1)
        else:
            w = np.full(len(sel), 1.0 / 26.0)
        with np.errstate(divide="ignore"):
            wn = np.where(count > 0, w / np.maximum(count, 1), 0.0)          # (count-of-target: an empty target has no mean)
        yield loc["rows"][sel], b, jx, jy, jz, wn, np.exp(T), D, rel_of(T, t32), s2


def occupancy_f64(points, offsets, grid, sigma2=0.01, mutant=None):
    """-> dict(canvas float64 [B, nz, ny, nx], bound float64 likewise): V and the docstring's bound on |canvas32 - V|"""
    shape = (len(offsets) - 1, grid.nz, grid.ny, grid.nx)
    V, A = np.zeros(shape), np.zeros(shape)
    for _, b, jx, jy, jz, wn, E, _, rel, _ in _terms64(points, offsets, grid, sigma2, mutant):
        np.add.at(V, (b, jz, jy, jx), wn * E)
        np.add.at(A, (b, jz, jy, jx), wn * E * (rel + 2.0 ** -52) + 2.0 ** -41)
    return dict(canvas=V, bound=A + U * (V + A) + 2.0 ** -40 * V)


def occupancy_bwd_f64(points, offsets, d_canvas, grid, sigma2=0.01, mutant=None):
    """-> dict(d_points float64 [n_max, 4], bound likewise): the analytic gradient G and the docstring's bound on |d_points32 - G|"""
    g = np.asarray(d_canvas, F).astype(np.float64)
    n_max = np.asarray(points).shape[0]
    G, A = np.zeros((n_max, 4)), np.zeros((n_max, 4))
    two = 1.0 if mutant == "backward-without-2" else 2.0
    for rows, b, jx, jy, jz, wn, E, D, rel, s2 in _terms64(points, offsets, grid, sigma2, mutant):
        c = g[b, jz, jy, jx] * wn * E
        for a in range(3):
            np.add.at(G[:, a], rows, c * (-two * D[a] / s2))
            np.add.at(A[:, a], rows, np.abs(c * (two * D[a] / s2)) * (rel + U * (1.0 + rel) + 2.0 ** -50))
    return dict(d_points=G, bound=A + U * (np.abs(G) + A))
