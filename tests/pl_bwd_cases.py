"""TEST INFRASTRUCTURE: the cases of the two backwards from pillar voxels to the network's plane, shared by the CPU tests (restatement vs
float64 autograd and vs csrc/pl_bwd_math.h on the host) and the GPU tests (restatement vs the kernels).  Seeded numpy; a case's forward
and reference are computed once and are read-only.

Projection: pl_batch_cases' shapes `odd` (B = 3, 8 x 13 -> up to 23 x 37: non-dyadic ratios, differing sizes, 851 padded pixels per image
= 4 workgroups with a partial last one, rows of three images) and `direct` (8 x 16, the no-tap path), with the plane's NaN and infinity
and its four negative entries per image replaced by finite positive values: every blend of the resize then has one sign, no kept pixel
sits where 10 v + 0.01 nearly cancels, and the derived constant bound of pl_bwd_ref holds on every element.  `odd-negatives` keeps the
negative entries (they fall behind the camera; their resized neighbours land just in front of it): the ill-conditioned demonstration,
held bit for bit like the rest and against float64 under its own, labelled bound.  Variants: dense, sparsity 3, a
depth input with scale 1.25, max_depth, a max_height that keeps the sky (so that the first source row is reached), 8 x 16 beams, a
per-image scale table with a NaN entry (image 1: empty cloud, zero plane), a capacity below the row count.

Pillars: a 4 x 3 grid of 0.5 x 0.5 cells, N = 3, B = 3: image 0 has a cell with 5 points (two overflow rows), image 1 is empty, image 2
is populated; about a third of the rows lie outside the grid in x, y or z; 7 unused rows behind offsets[B].  Plain and decorated, and
one decorated case with a capacity that ends inside the last image."""
import functools

import numpy as np

import pillar_ref as PR
import pl_batch_cases as PC
import pl_bwd_ref as BR

F = np.float32

# ---------------------------------------------------------------------------------------------- projection
PROJECT = {
    # name: (pl_batch_cases case, extra arguments)
    "odd-dense": ("odd-dense", {}),
    "odd-sparse3": ("odd-sparse3", {}),
    "odd-depth": ("odd-depth", {}),
    "odd-maxdepth": ("odd-maxdepth", {}),
    "odd-beams8x16": ("odd-beams8x16", {}),
    "odd-scales": ("odd-dense", dict(scales=[1.0, float("nan"), 0.75], scale=1.5)),
    "odd-capacity": ("odd-dense", dict(capacity=700)),
    "odd-tall": ("odd-dense", dict(max_height=100.0)),           # the backdrop above the horizon stays: the first source row is reached
    "odd-negatives": ("odd-dense", dict(keep_negatives=True)),   # blends across a sign change: ill-conditioned slopes
    "direct-dense": ("direct-dense", {}),
    "direct-depth": ("direct-depth", {}),
    "direct-beams8x16": ("direct-beams8x16", {}),
}
PROJECT_CASES = list(PROJECT)


@functools.lru_cache(maxsize=None)
def project_build(case):
    """-> dict of pl_bwd_ref.project_forward's arguments (m finite)"""
    base, extra = PROJECT[case]
    a = dict(PC.build(base))
    m = a["m"].copy()
    fill = (0.02, 0.004) if a["input"] == "disparity" else (30.0, 12.0)
    m[np.isnan(m)] = F(fill[0])
    m[np.isinf(m)] = F(fill[1])
    assert np.isfinite(m).all() and (m < 0).sum() == 4 * len(m)
    extra = dict(extra)
    if not extra.pop("keep_negatives", False):
        m[m < 0] = F(0.03 if a["input"] == "disparity" else 25.0)
    m.setflags(write=False)
    a.update(m=m, scales=None, capacity=None)
    a.update(extra)
    if a["scales"] is not None:
        a["scales"] = np.asarray(a["scales"], F)
    return a


@functools.lru_cache(maxsize=None)
def project_forward(case):
    out = BR.project_forward(**project_build(case))
    for v in out.values():
        v.setflags(write=False)
    return out


def project_capacity(case):
    """the rows of the cloud buffer a test allocates: the case's capacity, or five more rows than there are"""
    a = project_build(case)
    return a["capacity"] if a["capacity"] is not None else int(project_forward(case)["offsets"][-1]) + 5


@functools.lru_cache(maxsize=None)
def project_upstream(case):
    """seeded normals [capacity, 4] float32, NaN behind the rows that exist (never to be read); column 3 is noise that must be ignored"""
    cap, n = project_capacity(case), len(project_forward(case)["pixels"])
    g = np.full((cap, 4), np.nan, F)
    g[:n] = np.random.RandomState(4000 + len(case)).standard_normal((n, 4)).astype(F)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def project_reference(case):
    a = project_build(case)
    out = BR.project_bwd(project_upstream(case), project_forward(case), **a)
    for v in out.values():
        v.setflags(write=False)
    return out


def project_non_trivial(case):
    """every image with a cloud gets a non-zero d_m; an image without a usable scale an all-zero one; both tap-coincidence edges are hit
    -- the first and the last source row and column receive a gradient -- in image 0 of `odd-tall`: the other cases' scenes drop the sky,
    so edge coverage rests on that one case (the restatement sums over every (r, c) without a window, so a window that misses an edge
    shows there bit for bit)"""
    a, fwd, ref = project_build(case), project_forward(case), project_reference(case)
    B = a["m"].shape[0]
    n = np.diff(np.minimum(fwd["offsets"], len(fwd["pixels"])))
    for b in range(B):
        assert (n[b] > 0) == bool((ref["d_m"][b] != 0).any()), (case, b, n[b])
    assert (n > 0).sum() >= (1 if case.startswith("direct") else 2)
    if case == "odd-scales":
        assert n[1] == 0 and n[0] > 0 and n[2] > 0
    if case == "odd-capacity":
        assert int(fwd["offsets"][-1]) > a["capacity"] == len(fwd["pixels"])
    if case == "odd-tall":
        d = ref["d_m"][0]
        assert (d[0] != 0).any() and (d[-1] != 0).any() and (d[:, 0] != 0).any() and (d[:, -1] != 0).any(), case


# ---------------------------------------------------------------------------------------------- pillars
GRID = PR.make_grid(x=(0.0, 2.0), y=(-0.75, 0.75), z=(-1.0, 1.0), size=(0.5, 0.5))
N_SLOTS = 3
PILLAR = {"plain": dict(decorate=False), "decorated": dict(decorate=True), "decorated-capacity": dict(decorate=True, capacity=9)}
PILLAR_CASES = list(PILLAR)
FULL_CELL = (2, 1)                                           # (ix, iy) of image 0's cell with 5 points


def _image(rng, n, planted):
    pts = np.stack([rng.uniform(-0.3, 2.3, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.3, 1.3, n), rng.rand(n)], axis=1).astype(F)
    ix, iy, keep = PR.cells_of(pts, GRID)
    if planted:
        pts = pts[~(keep & (ix == FULL_CELL[0]) & (iy == FULL_CELL[1]))]
        x = GRID.x0 + GRID.vx * (FULL_CELL[0] + rng.uniform(0.1, 0.9, 5))
        y = GRID.y0 + GRID.vy * (FULL_CELL[1] + rng.uniform(0.1, 0.9, 5))
        pts = np.concatenate([pts, np.stack([x, y, rng.uniform(-0.9, 0.9, 5), rng.rand(5)], axis=1).astype(F)])
        pts = pts[rng.permutation(len(pts))]
    return pts


@functools.lru_cache(maxsize=None)
def pillar_build(case):
    """-> dict(points [n_max, 4], offsets int32 [4], grid, max_points, decorate, capacity)"""
    rng = np.random.RandomState(31)
    images = [_image(rng, 30, True), np.zeros((0, 4), F), _image(rng, 26, False)]
    offsets = np.concatenate([[0], np.cumsum([len(im) for im in images])]).astype(np.int32)
    pad = np.tile(np.array([[1.2, 0.0, 0.0, 0.5]], F), (7, 1))                       # inside the full cell: never read
    pts = np.concatenate(images + [pad])
    pts.setflags(write=False)
    offsets.setflags(write=False)
    return dict(dict(points=pts, offsets=offsets, grid=GRID, max_points=N_SLOTS, capacity=None), **PILLAR[case])


@functools.lru_cache(maxsize=None)
def pillar_forward(case):
    """-> pillar_ref.pillarize's dict plus slot_points [P', N]"""
    a = pillar_build(case)
    out = PR.pillarize(a["points"], a["offsets"], a["grid"], a["max_points"], a["decorate"], a["capacity"])
    out["slot_points"] = BR.pillar_slots(a["points"], a["offsets"], a["grid"], a["max_points"], a["capacity"])
    for v in out.values():
        v.setflags(write=False)
    return out


def pillar_capacity(case):
    a = pillar_build(case)
    return a["capacity"] if a["capacity"] is not None else len(pillar_forward(case)["coords"]) + 4


@functools.lru_cache(maxsize=None)
def pillar_upstream(case):
    """seeded normals [capacity, N, C] float32, NaN behind the pillars that exist; the padded slots of a pillar carry noise too (it must
    be ignored)"""
    a, fwd = pillar_build(case), pillar_forward(case)
    cap, P = pillar_capacity(case), len(fwd["coords"])
    g = np.full((cap, N_SLOTS, 9 if a["decorate"] else 4), np.nan, F)
    g[:P] = np.random.RandomState(5000 + len(case)).standard_normal(g[:P].shape).astype(F)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def pillar_reference(case):
    a, fwd = pillar_build(case), pillar_forward(case)
    out = BR.pillarize_bwd(pillar_upstream(case), fwd["slot_points"], fwd["num_points"], len(a["points"]))
    for v in out.values():
        v.setflags(write=False)
    return out


def pillar_non_trivial(case):
    """the full cell overflows and its overflow rows get +0.0, image 1 is empty, rows outside the grid exist and get +0.0, a cut
    capacity drops pillars whose rows then get +0.0"""
    a, fwd, ref = pillar_build(case), pillar_forward(case), pillar_reference(case)
    counts = PR.cell_counts(a["points"], a["offsets"], a["grid"])
    assert counts[0, FULL_CELL[1], FULL_CELL[0]] == 5 and counts[1].sum() == 0 and counts[2].sum() > 5
    o = fwd["offsets"].tolist()
    assert o[1] == o[2] and o[0] < o[1] < o[3]
    held = np.zeros(len(a["points"]), bool)
    held[fwd["slot_points"][fwd["slot_points"] >= 0]] = True
    n = PR.live_rows(a["points"], a["offsets"])
    _, _, keep = PR.cells_of(a["points"][:n], a["grid"])
    assert (~keep).sum() >= 10 and not held[:n][~keep].any() and not held[n:].any()
    assert keep.sum() - held.sum() >= (2 if a["capacity"] is None else 3)                    # overflow (and dropped pillars)
    assert (ref["d_points"][~held].view(np.uint32) == 0).all() and (ref["d_points"][held, :3] != 0).all()
    assert (fwd["num_points"] == N_SLOTS).any() and (fwd["num_points"] < N_SLOTS).any()
    if a["capacity"] is not None:
        assert o[2] < a["capacity"] < o[3]


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%d of %d elements differ, first at %s: %r vs %r" % (bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])
