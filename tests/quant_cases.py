"""TEST INFRASTRUCTURE: the cases of the soft-occupancy grid, shared by the CPU tests (restatement vs the float64 formulation and vs
csrc/quant_math.h on the host) and the GPU tests (restatement vs the kernels).  Seeded numpy; a case's reference is computed once.

The canvas kernels work on tiles of TILE_Y x TILE_X = 4 x 64 columns (csrc/quant_math.h; test_quant_cpu.py compares the constants).  The
grids have cells of 0.125 x 0.25 x 0.25 from (-1, -1, -1): every face is a binary fraction, so points can sit exactly on one.
    ODD  : 139 x 11 columns = two full tiles and a partial one of 11 in x, two full and one of 3 in y; nx is no multiple of 4 (dword stores)
    WIDE : 136 x 10 columns = two full tiles and one of 8 in x, two full and one of 2 in y; nx is a multiple of 4 (16-byte stores)
An image is ~500 random points in a box larger than the grid; one planted cell of 300 points (more than a workgroup's 256 threads) on a
tile corner, so that its neighbours lie in four tiles; one point in each of the eight corner cells of the grid and a few along its borders;
rows with NaN / +-inf / -0.0 coordinates; rows exactly on lower, inner and upper faces; all shuffled.  Shapes (B = 3):
    mixed : populated, no rows at all, every row outside the grid;   40 NaN rows behind offsets[B] (n_max > n)
    pair  : populated, populated (another seed), no rows;            the same padding
    over  : as pair, with offsets[B] 37 rows beyond n_max: the cloud buffer was too small, the last image is cut
Cases: shape-grid-nz-sigma2: nz = 1, 5 (odd and small) and 64; sigma2 = 0.02 (about a cell), 1e-4 ("sharp": every neighbour term and
most own terms underflow to +0) and 100 ("flat": every term is near 1).
"""
import functools

import numpy as np

import quant_ref as R

F = np.float32
TILE_X, TILE_Y, MAX_NZ = 64, 4, 64
THREADS = 256                                                # of a workgroup of the count and canvas kernels
SIZE = (0.125, 0.25, 0.25)
SHAPES = ("mixed", "pair", "over")
SIGMA2 = dict(cell=0.02, sharp=1e-4, flat=100.0)
CASES = ["mixed-odd-z5-cell", "mixed-wide-z1-cell", "pair-odd-z64-cell", "pair-wide-z5-sharp", "pair-odd-z1-flat", "over-wide-z5-cell",
         "over-odd-z5-flat"]
HARDEST = "over-odd-z5-flat"                                 # a cut image, dword rows, every neighbour term alive
MUTANT_CASE = "mixed-odd-z5-cell"
PLANTED = (64, 4)                                            # (ix, iy): the first column of the second tile in x and in y
PLANTED_COUNT = 300


def grid_of(kind, nz):
    nx, ny = (139, 11) if kind == "odd" else (136, 10)
    return R.make_grid(x=(-1.0, -1.0 + nx * SIZE[0]), y=(-1.0, -1.0 + ny * SIZE[1]), z=(-1.0, -1.0 + nz * SIZE[2]), size=SIZE)


def in_cell(rng, g, ix, iy, iz, k):
    x = g.x0 + g.vx * (ix + rng.uniform(0.02, 0.98, k))
    y = g.y0 + g.vy * (iy + rng.uniform(0.02, 0.98, k))
    z = g.z0 + g.vz * (iz + rng.uniform(0.02, 0.98, k))
    return np.stack([x, y, z, rng.rand(k)], axis=1).astype(F)


def special_rows(g):
    x1, y1, z1 = g.x0 + g.vx * g.nx, g.y0 + g.vy * g.ny, g.z0 + g.vz * g.nz
    nan, inf = np.nan, np.inf
    below = lambda v: np.nextafter(F(v), F(-1e9))
    rows = [(nan, 0, -0.9), (0, nan, -0.9), (0, 0, nan), (inf, 0, -0.9), (-inf, 0, -0.9), (0, inf, -0.9), (0, -inf, -0.9), (0, 0, inf), (0, 0, -inf),
            (-0.0, -0.0, g.z0),
            (g.x0, g.y0, g.z0),                              # three lower faces: the first cell
            (g.x0 + 70 * g.vx, g.y0 + 5 * g.vy, g.z0),       # inner faces: the upper cell
            (x1, 0.1, -0.9), (0.1, y1, -0.9), (0.1, 0.1, z1),        # upper faces: out
            (below(g.x0), 0.1, -0.9), (0.1, below(g.y0), -0.9), (0.1, 0.1, below(g.z0)),      # just below the lower faces: out
            (below(x1), below(y1), below(z1)),               # the last cell, unless v - origin rounds up to the face (then out)
            (x1 - 0.01, y1 - 0.01, z1 - 0.01)]               # the last cell
    return np.asarray([r + (0.5,) for r in rows], F)


def border_rows(rng, g):
    parts = [in_cell(rng, g, ix, iy, iz, 1) for ix in (0, g.nx - 1) for iy in (0, g.ny - 1) for iz in sorted({0, g.nz - 1})]       # corners
    parts += [in_cell(rng, g, int(rng.randint(g.nx)), iy, int(rng.randint(g.nz)), 2) for iy in (0, g.ny - 1)]
    parts += [in_cell(rng, g, ix, int(rng.randint(g.ny)), int(rng.randint(g.nz)), 2) for ix in (0, g.nx - 1, TILE_X - 1, 2 * TILE_X)]
    return np.concatenate(parts)


def image_points(seed, g):
    rng = np.random.RandomState(seed)
    x1, y1, z1 = g.x0 + g.vx * g.nx, g.y0 + g.vy * g.ny, g.z0 + g.vz * g.nz
    box = np.stack([rng.uniform(g.x0 - 1.0, x1 + 1.0, 500), rng.uniform(g.y0 - 0.4, y1 + 0.4, 500),
                    rng.uniform(g.z0 - 0.2 * (z1 - g.z0), z1 + 0.2 * (z1 - g.z0), 500), rng.rand(500)], axis=1).astype(F)
    dense = np.stack([rng.uniform(3.0, 5.0, 250), rng.uniform(-0.5, 0.5, 250), rng.uniform(g.z0, z1, 250), rng.rand(250)], axis=1).astype(F)
    parts = [box, dense, in_cell(rng, g, PLANTED[0], PLANTED[1], g.nz // 2, PLANTED_COUNT), border_rows(rng, g), special_rows(g)]
    parts.append(box[rng.choice(len(box), 12, replace=False)])                  # duplicates
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))]


def outside_points(seed, g):
    rng = np.random.RandomState(seed)
    x1, z1 = g.x0 + g.vx * g.nx, g.z0 + g.vz * g.nz
    p = np.stack([rng.uniform(x1 + 0.5, x1 + 9.0, 150), rng.uniform(-9.0, 9.0, 150), rng.uniform(g.z0, z1, 150), rng.rand(150)], axis=1).astype(F)
    p[::3, 0] = rng.uniform(0.0, 2.0, 50)                    # inside in x and y, above the grid in z
    p[::3, 1] = rng.uniform(-1.0, 1.0, 50)
    p[::3, 2] = z1 + 0.5
    return p


@functools.lru_cache(maxsize=None)
def build(case):
    """-> dict(points [n_max, 4], offsets int32 [B + 1], grid, sigma2)"""
    shape, kind, nz, width = case.split("-")
    g, seed = grid_of(kind, int(nz[1:])), 100 * SHAPES.index(shape) + (7 if kind == "wide" else 0)
    empty = np.zeros((0, 4), F)
    if shape == "mixed":
        images = [image_points(seed + 1, g), empty, outside_points(seed + 2, g)]
    else:
        images = [image_points(seed + 1, g), image_points(seed + 2, g), empty]
    if shape == "pair":
        images = [images[0], empty, images[1]]               # the empty image in the middle
    offsets = np.concatenate([[0], np.cumsum([len(im) for im in images])]).astype(np.int32)
    pts = np.concatenate(images)
    if shape == "over":
        pts = pts[:len(pts) - 37]
    else:
        pts = np.concatenate([pts, np.full((40, 4), np.nan, F)])
    pts = np.ascontiguousarray(pts)
    pts.setflags(write=False)
    offsets.setflags(write=False)
    return dict(points=pts, offsets=offsets, grid=g, sigma2=SIGMA2[width])


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> quant_ref.occupancy's dict; shared, do not write into it"""
    out = R.occupancy(**build(case))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def upstream(case):
    """the gradient of the canvas: seeded, some exact zeros, some large values"""
    g, B = build(case)["grid"], len(build(case)["offsets"]) - 1
    rng = np.random.RandomState(4242)
    d = rng.standard_normal((B, g.nz, g.ny, g.nx)).astype(F)
    d[rng.rand(*d.shape) < 0.1] = 0.0
    d[rng.rand(*d.shape) < 0.01] *= F(1000.0)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference_bwd(case):
    a = build(case)
    out = R.occupancy_bwd(a["points"], a["offsets"], reference(case)["point_count"], upstream(case), a["grid"], a["sigma2"])
    out.setflags(write=False)
    return out


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    view = np.uint32 if got.dtype == F else got.dtype
    assert np.array_equal(got.view(view), want.view(view)), "%d of %d elements differ" % ((got.view(view) != want.view(view)).sum(), got.size)


def check_non_trivial(case):
    """the tiling is spanned, the planted cell came out as planted, borders, corners and special rows did what the case says"""
    a, want = build(case), reference(case)
    g, off = a["grid"], a["offsets"]
    shape, _, _, width = case.split("-")
    assert g.nx > 2 * TILE_X and g.nx % TILE_X and g.ny > 2 * TILE_Y and g.ny % TILE_Y and 1 <= g.nz <= MAX_NZ
    loc, n = R.located(a["points"], off, g)
    assert n == (len(a["points"]) if shape == "over" else len(a["points"]) - 40) and (shape != "over" or off[-1] > len(a["points"]))
    table = loc["table"]
    assert table[0, g.nz // 2, PLANTED[1], PLANTED[0]] >= PLANTED_COUNT > THREADS and (table == 1).sum() > 100
    for ix in (0, g.nx - 1):
        for iy in (0, g.ny - 1):
            for iz in (0, g.nz - 1):
                assert table[0, iz, iy, ix] >= 1
    empty = [b for b in range(len(off) - 1) if off[b] == off[b + 1]]
    assert empty == ([1] if shape != "over" else [2])
    if shape == "mixed":
        assert off[3] > off[2] and table[2].sum() == 0 and not want["canvas"][2].any()
    assert (want["point_count"] == 0).sum() >= 100 and want["point_count"].max() >= PLANTED_COUNT
    assert not want["canvas"][empty[0]].any() and np.isfinite(want["canvas"]).all() and want["canvas"].min() >= 0
    c = want["canvas"][0]
    if width == "sharp":                                     # neighbour terms are gone: an empty cell stays empty
        assert not c[table[0] == 0].any() and c[table[0] > 0].any()
    elif width == "flat":                                    # every term is near 1
        assert c[table[0] > 0].min() > 0.99 and c.max() <= 2.0 + 1e-6
    else:
        assert c[table[0] == 0].any() and (c[table[0] > 0] > 0).all()
