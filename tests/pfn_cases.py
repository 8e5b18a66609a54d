"""TEST INFRASTRUCTURE: the cases of the pillar feature net and its pseudo-image, shared by the CPU tests (restatement vs a float64 torch
composition and vs csrc/pfn_math.h on the host) and the GPU tests (restatement vs the kernel).  Seeded numpy; a case's reference is
computed once.  Pillars come from pillar_ref.pillarize (numpy) or are planted, so the kernel is tested apart from mcav_pillarize.

    <pillar case>-o<C_out>  the pillars of a case of tests/pillar_cases.py (the 7 x 9 grid, B = 3: an image without pillars, partly filled
                            and full pillars, N = 1, 5, 32 and 64, C = 4 and 9) under a layer of C_out channels
    fullrow-o32             planted: B = 2, 7 x 9, every cell of row 3 of image 0 next to rows without any, the corners of image 1
    special-o32             planted: slots whose intensity is NaN, +inf and -inf under a zero, a positive and a negative weight: NaN (inf x 0
                            and a propagated NaN), +inf and +0.0 come out (check_non_trivial asserts it)
    wide-o128               planted: B = 2, nx = 1100, ny = 2, C = 9, N = 4: more than one column tile, a last tile of 76 columns, pillars
                            at columns 0, TILE - 1, TILE, nx - 1 and between, NaN rows among them.  nx x 128 channels does not fit the LDS.
    real-o64                B = 2 on PointPillars' 432 x 496 grid, 2 x 2200 points, N = 8: the canvas is 110 MB
Layer: weights from a seeded normal with exact zeros; channel 1 is negative for every finite input with intensity >= 0 (feature +0.0),
channel 2 has a positive bias and small weights, so bias_pad = bias and bias_pad = 0 differ on partly filled pillars.
"""
import functools

import numpy as np

import pfn_ref as R
import pillar_cases as PC
import pillar_ref as PR

F = np.float32
TILE = 128                                                   # columns per workgroup (csrc/pfn_image.hip)
PILLAR_CASES = ["mixed-N1-c4-o32", "mixed-N5-c9-o64", "mixed-N32-c9-o128", "pair-N5-c9-o32", "pair-N5-c9-o64", "over-N64-c4-o128",
                "over-N64-c4-o64", "over-N5-c9-o96"]
PLANTED_CASES = ["fullrow-o32", "special-o32", "wide-o128"]
CASES = PILLAR_CASES + PLANTED_CASES
REAL_CASE = "real-o64"
HARDEST = "wide-o128"                                        # with a capacity that ends inside the second image: column tiles, NaN rows, a cut
WIDE_NX = 1100
WIDE_COLUMNS = [0, 1, 63, TILE - 1, TILE, TILE + 1, 500, 8 * TILE - 1, 8 * TILE, WIDE_NX - 2, WIDE_NX - 1]


def layer(C_out, C, seed):
    rng = np.random.RandomState(seed)
    w = (0.5 * rng.randn(C_out, C)).astype(F)
    w[rng.rand(C_out, C) < 0.1] = 0.0
    b = (0.3 * rng.randn(C_out)).astype(F)
    w[1] = 0.0
    w[1, 3], b[1] = -0.5, -0.25
    w[2] *= F(0.01)
    b[2] = 0.625
    return w, b


def planted(rows, B, N, C, seed):
    """rows: (b, iy, ix, n) in ascending order -> voxels, coords, num_points, offsets with seeded points in the used slots"""
    rng = np.random.RandomState(seed)
    P = len(rows)
    vox = np.zeros((P, N, C), F)
    for p, (_, _, _, n) in enumerate(rows):
        vox[p, :n] = rng.uniform(-2.0, 2.0, (n, C)).astype(F)
        vox[p, :n, 3] = rng.rand(n).astype(F)
    coords = np.array([(b, 0, iy, ix) for b, iy, ix, _ in rows], np.int32).reshape(P, 4)
    num = np.array([n for _, _, _, n in rows], np.int32)
    offsets = np.searchsorted(coords[:, 0], np.arange(B + 1)).astype(np.int32)
    assert sorted(rows) == list(rows)
    return vox, coords, num, offsets


@functools.lru_cache(maxsize=None)
def build(case):
    """-> dict(voxels [P, N, C], coords, num_points, offsets int32 [B + 1], nx, ny, weight, bias); shared, read-only"""
    name, o = case.rsplit("-o", 1)
    C_out = int(o)
    if name == "fullrow":
        rows = [(0, 3, ix, 1 + ix % 3) for ix in range(7)] + [(1, 0, 0, 3), (1, 0, 6, 1), (1, 8, 0, 2), (1, 8, 6, 3)]
        vox, coords, num, off = planted(rows, 2, 3, 4, 11)
        nx, ny = 7, 9
    elif name == "special":
        rows = [(0, 2, 1, 1), (0, 2, 3, 1), (0, 5, 5, 1), (0, 6, 0, 2)]
        vox, coords, num, off = planted(rows, 1, 2, 4, 12)
        vox[:3, 0, :3] = 0.0
        vox[0, 0, 3], vox[1, 0, 3], vox[2, 0, 3] = np.nan, np.inf, -np.inf
        nx, ny = 7, 9
    elif name == "wide":
        rows = [(b, iy, ix, 1 + (ix + iy + b) % 4) for b in range(2) for iy in range(2) for ix in WIDE_COLUMNS]
        vox, coords, num, off = planted(rows, 2, 4, 9, 13)
        vox[5, 0, 3] = np.nan                                # column TILE + 1 of the first row
        vox[len(WIDE_COLUMNS) * 2 + 3, 0, 2] = np.nan        # column TILE - 1 of the second image
        nx, ny = WIDE_NX, 2
    elif name == "real":
        g = PR.make_grid()
        rng = np.random.RandomState(14)
        per = 2200
        pts = np.stack([rng.uniform(0.0, 69.12, 2 * per), rng.uniform(-39.68, 39.68, 2 * per), rng.uniform(-3.0, 1.0, 2 * per),
                        rng.rand(2 * per)], axis=1).astype(F)
        for i in range(20):                                  # twenty cells of ten points each per image: partly filled and full pillars
            for b in range(2):
                cell = pts[b * per + i, :2]
                pts[b * per + 200 + 10 * i:b * per + 210 + 10 * i, :2] = cell
        corners = np.array([[0.01, -39.67, 0, 1], [69.11, 39.67, 0, 1]], F)
        pts[:2], pts[per:per + 2] = corners, corners
        out = PR.pillarize(pts, np.array([0, per, 2 * per], np.int32), g, max_points=8)
        vox, coords, num, off = out["voxels"], out["coords"], out["num_points"], out["offsets"]
        nx, ny = g.nx, g.ny
    else:
        out, g = PC.reference(name), PC.build(name)["grid"]
        vox, coords, num, off = out["voxels"], out["coords"], out["num_points"], out["offsets"]
        nx, ny = g.nx, g.ny
    w, b = layer(C_out, vox.shape[2], 1000 + C_out + vox.shape[2])
    if name == "special":
        w[0, 3], w[3, 3], w[4, 3] = 0.0, 1.5, -2.0           # beside channels 1 (negative weight) and 2 (positive bias)
        b[0], b[3], b[4] = -1.0, -1.0, -1.0
    d = dict(voxels=np.ascontiguousarray(vox), coords=np.ascontiguousarray(coords), num_points=np.ascontiguousarray(num),
             offsets=np.ascontiguousarray(off), nx=nx, ny=ny, weight=w, bias=b)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(case, pad="bias", capacity=None):
    """-> pfn_ref.pseudo_image's dict with bias_pad = bias ("bias") or 0 ("zero"); shared, do not write into it"""
    a = build(case)
    out = R.pseudo_image(a["voxels"], a["coords"], a["num_points"], a["offsets"], a["nx"], a["ny"], a["weight"], a["bias"],
                         bias_pad=bias_pad(a, pad), capacity=capacity)
    for v in out.values():
        v.setflags(write=False)
    return out


def bias_pad(a, pad):
    return a["bias"] if pad == "bias" else np.zeros_like(a["bias"])


def cut_capacity(case):
    """a capacity that ends three pillars inside the second image"""
    off = build(case)["offsets"]
    cap = int(off[1]) + 3
    assert int(off[1]) < cap < int(off[2])
    return cap


def same_bits(got, want):
    """finite values (and the infinities) bit for bit, NaNs by class"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F, (got.shape, want.shape, got.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaNs at other places: %d vs %d" % (gn.sum(), wn.sum())
    g, w = np.where(gn, F(0), got).view(np.uint32), np.where(wn, F(0), want).view(np.uint32)
    bad = g != w
    assert not bad.any(), "%d of %d elements differ, first at %s: %r vs %r" % (
        bad.sum(), bad.size, np.argwhere(bad)[0].tolist(), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def check_non_trivial(case):
    """the case holds what its name promises, and the two paddings differ"""
    a, want, zero = build(case), reference(case), reference(case, "zero")
    name = case.rsplit("-o", 1)[0]
    feat, N = want["features"], a["voxels"].shape[1]
    P = len(feat)
    assert P == int(a["offsets"][-1]) == len(a["coords"]) >= 4
    assert (a["weight"] == 0).sum() >= 4 and a["bias"][2] > 0
    finite = ~np.isnan(a["voxels"]).any(axis=(1, 2)) & ~np.isinf(a["voxels"]).any(axis=(1, 2))
    assert (feat[finite, 1].view(np.uint32) == 0).all()                                   # the negative channel: +0.0, sign bit clear
    partly = a["num_points"] < N
    if partly.any():
        assert not np.array_equal(want["canvas"].view(np.uint32), zero["canvas"].view(np.uint32))      # bias_pad matters
        assert (feat[partly & finite, 2] >= a["bias"][2]).all()
    else:
        assert N == 1
    occupied = np.zeros(want["canvas"].shape[:1] + want["canvas"].shape[2:], bool)
    occupied[a["coords"][:, 0], a["coords"][:, 2], a["coords"][:, 3]] = True
    assert occupied.sum() == P and (want["canvas"].transpose(0, 2, 3, 1)[~occupied].view(np.uint32) == 0).all()
    if name == "fullrow":
        assert occupied[0, 3].all() and not occupied[0, 2].any() and not occupied[0, 4].any()
    elif name == "special":
        f = feat[:3]
        assert np.isnan(f[0]).all()                                                        # a NaN slot: every channel, the zero weight included
        assert np.isnan(f[1, 0]) and np.isnan(f[2, 0])                                     # inf x 0
        assert f[1, 3] == np.inf and f[2, 4] == np.inf
        assert f[1, 4].view(np.uint32) == 0 and f[2, 3].view(np.uint32) == 0               # -inf -> +0.0
        assert np.isfinite(feat[3]).all()
    elif name == "wide":
        assert a["nx"] > 8 * TILE and a["nx"] % TILE not in (0, 1) and np.isnan(feat).any() and not np.isnan(feat).all(axis=1).all()
        cols = set(a["coords"][:, 3].tolist())
        assert {0, TILE - 1, TILE, a["nx"] - 1} <= cols
    elif name == "real":
        assert (np.diff(a["offsets"]) > 1500).all() and (a["num_points"] == N).any() and partly.any()
        assert a["coords"][0].tolist() == [0, 0, 0, 0] and a["coords"][-1].tolist() == [1, 0, 495, 431]
    else:
        assert (np.diff(a["offsets"]) == 0).any()                                          # an image without pillars
