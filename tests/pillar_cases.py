"""TEST INFRASTRUCTURE: the cases of the pillar voxeliser, shared by the CPU tests (restatement vs the sequential transcription and vs
csrc/pillar_math.h on the host) and the GPU tests (restatement vs the kernels).  Seeded numpy; a case's reference is computed once.

The grid is 7 x 9 cells of 0.5 x 0.25 (a multiple of no block size; every edge is a binary fraction, so points can sit exactly on one).  An
image is ~400 random points in a box larger than the grid, five planted cells that hold exactly N, N + 1, 65, 130 and 300 points (one
chunk, two chunks and five chunks of the selection), duplicated rows, rows with NaN / +-inf / -0.0 coordinates and rows exactly on lower
and upper edges, all shuffled.  Shapes (B = 3):
    mixed : populated, no rows at all, every row outside the grid;      50 unused rows of in-range values behind offsets[B]
    pair  : populated, populated (another seed), no rows;               the same padding
    over  : as pair, with offsets[B] 37 rows beyond n_max: the cloud buffer was too small, the last image is cut
TILE_CASES, a list of its own (the GPU tests take it; the CPU suites' sequential transcription does not):
    tiles : B = 5 on PointPillars' own 432 x 496 grid: 1 071 360 cells = 1047 tiles of 1024 cells, more than the 1024 tile sums that the
            one-block scan takes per pass, and ny * nx is no multiple of 1024, so image boundaries fall inside tiles.  600 uniform
            in-range points per image, N = 4, 4 columns: nearly every pillar stands in a tile of its own, each offset by the tiles before.
            (test_pillar_gpu.py's test_scan_past_its_first_pass reaches the same second pass with dense random clouds and decorated
            columns; this case keeps the shape among the shared cases, with its properties asserted by check_non_trivial.)
"""
import functools

import numpy as np

import pillar_ref as R

F = np.float32
GRID = R.make_grid(x=(-1.0, 2.5), y=(-1.0, 1.25), z=(-1.0, 1.0), size=(0.5, 0.25))
PLANTED = [(1, 1), (5, 7), (3, 4), (1, 7), (5, 2)]          # (ix, iy) of the cells with N, N + 1, 65, 130, 300 points
POINTS = (1, 4, 5, 32, 64)
SHAPES = ("mixed", "pair", "over")
CASES = ["mixed-N%d-c%d" % (n, c) for n in POINTS for c in (4, 9)] + ["pair-N5-c9", "pair-N32-c4", "over-N4-c9", "over-N64-c4"]
HARDEST = "over-N5-c9"                                       # chunks, a cut image, the decorated columns, a block that starts off 16 bytes
CASES.append(HARDEST)
TILE_CASES = ["tiles"]
TILE = 1024                                                  # cells per workgroup of the scan passes (csrc/pillarize.hip)


def planted_counts(N):
    return [N, N + 1, 65, 130, 300]


def in_cell(rng, ix, iy, k, g=GRID):
    x = g.x0 + g.vx * (ix + rng.uniform(0.02, 0.98, k))
    y = g.y0 + g.vy * (iy + rng.uniform(0.02, 0.98, k))
    return np.stack([x, y, rng.uniform(-0.9, 0.9, k), rng.rand(k)], axis=1).astype(F)


def special_rows(g=GRID):
    x1, y1 = g.x0 + g.vx * g.nx, g.y0 + g.vy * g.ny
    nan, inf = np.nan, np.inf
    rows = [(nan, 0, 0), (0, nan, 0), (0, 0, nan), (inf, 0, 0), (-inf, 0, 0), (0, inf, 0), (0, 0, inf), (0, 0, -inf), (-0.0, -0.0, -0.0),
            (g.x0, g.y0, g.z0),                              # three lower edges: in
            (g.x0 + 2 * g.vx, g.y0 + 5 * g.vy, 0.5),         # inner edges: the upper cell
            (x1, 0.1, 0), (0.1, y1, 0), (0.1, 0.1, g.z1),    # upper edges: out
            (np.nextafter(F(x1), F(0)), np.nextafter(F(y1), F(0)), np.nextafter(g.z1, F(0)))]
    return np.asarray([r + (0.5,) for r in rows], F)


def image_points(seed, N, g=GRID):
    rng = np.random.RandomState(seed)
    box = np.stack([rng.uniform(-1.5, 3.0, 400), rng.uniform(-1.4, 1.6, 400), rng.uniform(-1.3, 1.3, 400), rng.rand(400)], axis=1).astype(F)
    ix, iy, keep = R.cells_of(box, g)
    planted = np.zeros(len(box), bool)
    for cx, cy in PLANTED:
        planted |= keep & (ix == cx) & (iy == cy)
    parts = [box[~planted]] + [in_cell(rng, cx, cy, k) for (cx, cy), k in zip(PLANTED, planted_counts(N))]
    parts.append(parts[0][rng.choice(len(parts[0]), 12, replace=False)])       # duplicates
    parts.append(special_rows(g))
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))]


def outside_points(seed):
    rng = np.random.RandomState(seed)
    p = np.stack([rng.uniform(3.0, 9.0, 150), rng.uniform(-9.0, 9.0, 150), rng.uniform(-0.5, 0.5, 150), rng.rand(150)], axis=1).astype(F)
    p[::3, 0] = rng.uniform(0.0, 2.0, 50)                    # inside in x and y, above the grid in z
    p[::3, 1] = rng.uniform(-1.0, 1.0, 50)
    p[::3, 2] = 1.5
    return p


@functools.lru_cache(maxsize=None)
def build(case):
    """-> dict(points [n_max, 4], offsets int32 [B + 1], grid, max_points, decorate)"""
    if case == "tiles":
        g, B, per = R.make_grid(x=(0.0, 69.12), y=(-39.68, 39.68), z=(-3.0, 1.0), size=(0.16, 0.16)), 5, 600
        rng = np.random.RandomState(77)
        pts = np.stack([rng.uniform(0.0, 69.12, B * per), rng.uniform(-39.68, 39.68, B * per), rng.uniform(-3.0, 1.0, B * per),
                        rng.rand(B * per)], axis=1).astype(F)
        offsets = (np.arange(B + 1) * per).astype(np.int32)
        pts.setflags(write=False)
        offsets.setflags(write=False)
        return dict(points=pts, offsets=offsets, grid=g, max_points=4, decorate=False)
    shape, n, c = case.split("-")
    N, seed = int(n[1:]), 100 * SHAPES.index(shape)
    empty = np.zeros((0, 4), F)
    if shape == "mixed":
        images = [image_points(seed + 1, N), empty, outside_points(seed + 2)]
    else:
        images = [image_points(seed + 1, N), image_points(seed + 2, N), empty]
    offsets = np.concatenate([[0], np.cumsum([len(im) for im in images])]).astype(np.int32)
    pts = np.concatenate(images)
    if shape == "over":
        pts = pts[:len(pts) - 37]
    else:
        pts = np.concatenate([pts, in_cell(np.random.RandomState(seed + 9), 4, 6, 50)])       # never read: they would swell cell (4, 6)
    pts.setflags(write=False)
    offsets.setflags(write=False)
    return dict(points=pts, offsets=offsets, grid=GRID, max_points=N, decorate=c == "c9")


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> pillar_ref.pillarize's dict; shared, do not write into it"""
    out = R.pillarize(**build(case))
    for v in out.values():
        v.setflags(write=False)
    return out


def check_non_trivial(case):
    """the planted cells came out as planted, both populated images have pillars, the padding rows would have added pillar points"""
    a, want = build(case), reference(case)
    if case == "tiles":
        g, c = a["grid"], want["coords"].astype(np.int64)
        cell = (c[:, 0] * g.ny + c[:, 2]) * g.nx + c[:, 3]                                 # flat over (image, iy, ix), as the kernels count
        assert (cell >= 1 << 20).any()                                                     # beyond the first pass of the tile scan
        assert len(np.unique(cell[cell < 1 << 20] // TILE)) >= 3                           # cross-tile offsets inside the first pass
        assert g.ny * g.nx % TILE != 0                                                     # an image boundary inside a tile
        return
    N = a["max_points"]
    P = int(want["offsets"][-1])
    assert P == len(want["coords"]) >= 40
    counts = R.cell_counts(a["points"], a["offsets"], a["grid"])
    shape = case.split("-")[0]
    for (cx, cy), k in zip(PLANTED, planted_counts(N)):
        if shape != "over":
            assert counts[0, cy, cx] == k, (case, cx, cy, counts[0, cy, cx], k)
    if shape == "mixed":
        assert want["offsets"].tolist() == [0, P, P, P]
    else:
        o = want["offsets"].tolist()
        assert 0 < o[1] < o[2] == o[3]
        assert R.live_rows(a["points"], a["offsets"]) == (len(a["points"]) if shape == "over" else len(a["points"]) - 50)
    assert (want["num_points"] == N).any() and (N == 1 or (want["num_points"] < N).any())
