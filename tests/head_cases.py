"""Shapes for the one-channel disparity head (csrc/narrow_conv.hip: conv3x3r_c1_fwd_kernel, conv3x3r_c1_bwd_kernel and its finalize), chosen by
where the image border falls relative to the kernels' fixed grids -- the 16-row tile, the 1024 / C pixel columns of a workgroup, the four-row
prefetch group -- and by how many tiles a workgroup walks, not by workload.  Shared by tests/test_head_cpu.py (every class below is hit for
every channel count; the reference of tests/head_ref.py against itself and against its mutants) and tests/test_head_gpu.py (the launches).

A case is (B, H, W, C) of the 3x3 reflection-padded convolution C -> 1 on an H x W image."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

TH, PF = 16, 4                              # rows of a tile, rows of a prefetch group
FWD_BLOCKS, BWD_BLOCKS = 16384, 2048        # the most workgroups of a forward / backward launch: more tiles are walked grid-stride
CHANNELS = (16, 32, 64, 128)

Case = namedtuple("Case", "B H W C")


def pxb(C):
    """pixel columns of a tile: C / 4 lanes of the 256 own one pixel"""
    return 1024 // C


def tiles_y(c):
    return -(-c.H // TH)


def tiles_x(c):
    return -(-c.W // pxb(c.C))


def tiles(c):
    return c.B * tiles_y(c) * tiles_x(c)


def tile_origin(c, k):
    """(n, y0, x0) of linear tile k, as the kernels decode it"""
    per = tiles_y(c) * tiles_x(c)
    n, tr = k // per, k % per
    return n, tr // tiles_x(c) * TH, tr % tiles_x(c) * pxb(c.C)


def tile_rows(c, k):
    return min(TH, c.H - tile_origin(c, k)[1])


def tiles_per_workgroup(c, cap):
    """how many tiles workgroup g of min(tiles, cap) walks"""
    n = min(tiles(c), cap)
    return [len(range(g, tiles(c), n)) for g in range(n)]


# ------------------------------------------------------------------------------------------------ alignment classes
Cls = namedtuple("Cls", "name pred")
ROW_CLASSES = (
    Cls("H == 2", lambda c: c.H == 2),
    Cls("H == 3", lambda c: c.H == 3),
    Cls("H % 16 == 0", lambda c: c.H % TH == 0),
    Cls("H % 16 == 1", lambda c: c.H % TH == 1),                  # the last forward tile reads 3 rows: shorter than one prefetch group
    Cls("H % 16 == 2", lambda c: c.H % TH == 2 and c.H > 2),
    Cls("H % 16 == 3", lambda c: c.H % TH == 3 and c.H > 3),      # 5 forward rows: one alone in the second prefetch group
    Cls("H % 16 == 15", lambda c: c.H % TH == TH - 1),
    Cls("rows 1, H-2 in one tile", lambda c: c.H > 3 and 1 // TH == (c.H - 2) // TH),
    Cls("rows 1, H-2 in different tiles", lambda c: 1 // TH != (c.H - 2) // TH),
    Cls("rows H-2, H-1 in different tiles", lambda c: (c.H - 2) // TH != (c.H - 1) // TH),
)
COL_CLASSES = (
    Cls("W == 2", lambda c: c.W == 2),
    Cls("W == 3", lambda c: c.W == 3),
    Cls("3 < W < P", lambda c: 3 < c.W < pxb(c.C)),
    Cls("W == P", lambda c: c.W == pxb(c.C)),
    Cls("W % P == 0, two or more tile columns", lambda c: c.W % pxb(c.C) == 0 and c.W >= 2 * pxb(c.C)),
    Cls("W % P == 1", lambda c: c.W % pxb(c.C) == 1 and c.W > pxb(c.C)),      # column W - 2 is the last lane of the previous tile
    Cls("W % P == 2", lambda c: c.W % pxb(c.C) == 2 and c.W > pxb(c.C)),
    Cls("W % P == P - 1", lambda c: c.W % pxb(c.C) == pxb(c.C) - 1),
)


# ------------------------------------------------------------------------------------------------ the cases
def _base(C):
    P = pxb(C)
    # B varies so that the tile counts of one C cover several residues
    return tuple(Case(B, H, W, C) for B, (H, W) in zip((1, 2, 3, 1, 2, 1, 3, 2, 1, 3, 2, 1), (
        (2, 2), (3, 3), (16, P), (17, P + 1), (18, P + 2), (19, 2 * P - 1), (15, P - 1), (5, 2 * P), (35, 2 * P + 1), (33, 3), (2, P + 1), (13, 2))))


CASES = tuple(c for C in CHANNELS for c in _base(C))

# H = 33, W = 3: one tile column and three tile rows of 16, 16 and 1 rows per image.  Neither cap is a multiple of 3, so the second tile of a
# workgroup has another row count than its first.
WALK_CASES = (
    Case(684, 33, 3, 16),       # 2052 tiles: backward workgroups 0 .. 3 walk two
    Case(684, 33, 3, 128),
    Case(5462, 33, 3, 16),      # 16386 tiles: forward workgroups 0 and 1 walk two, backward workgroups eight or nine
)
FWD_WALK_CASE = WALK_CASES[2]


def walk_tiles(c, cap=BWD_BLOCKS):
    """the tile supports of a walk case: a tile walked first by a workgroup that goes on to a tile of another row count, that second tile,
    and the very last tile"""
    differ = [g for g in range(min(tiles(c) - cap, 3)) if tile_rows(c, g) != tile_rows(c, g + cap)]
    g = max(differ, key=lambda g: tile_rows(c, g + cap))           # (a one-row first tile and a 16-row second one where there is the choice)
    return (g, g + cap, tiles(c) - 1)


def case_id(c):
    return "%dx%dx%d_c%d" % c


# ------------------------------------------------------------------------------------------------ dy supports
def support_mask(c, support):
    """[B, 1, H, W] bool: where dy is non-zero.  'band': rows {0, 1, H-2, H-1} and columns {0, 1, W-2, W-1} of the last image;
    ('tile', k): exactly the k-th 16 x P tile; 'dense'."""
    m = torch.zeros(c.B, 1, c.H, c.W, dtype=torch.bool)
    if support == "dense":
        m[:] = True
    elif support == "band":
        for r in (0, 1, c.H - 2, c.H - 1):
            m[-1, 0, r, :] = True
        for q in (0, 1, c.W - 2, c.W - 1):
            m[-1, 0, :, q] = True
    else:
        n, y0, x0 = tile_origin(c, support[1])
        m[n, 0, y0:y0 + TH, x0:x0 + pxb(c.C)] = True
    return m


def supports(c):
    """the supports of a base case: those whose weight gradient is judged by the elementwise envelope, then 'dense' (judged in the max-norm)"""
    out = ["band", ("tile", tiles(c) - 1)]
    if tiles(c) > 1:
        out.append(("tile", 0))
    return out + ["dense"]


def support_id(s):
    return s if isinstance(s, str) else "tile%d" % s[1]


# ------------------------------------------------------------------------------------------------ inputs (float32, NCHW, on the CPU)
@functools.lru_cache(maxsize=None)
def inputs(c):
    g = torch.Generator().manual_seed(5000 + 7 * c.B + 131 * c.H + 17 * c.W + 3 * c.C)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    return dict(x=F.elu(r(c.B, c.C, c.H, c.W)),                      # the head's input is an ELU output
                w=r(1, c.C, 3, 3) * 0.2, b=0.1 * r(1),
                y=torch.sigmoid(r(c.B, 1, c.H, c.W)),                # the saved disparity, given so that the backward needs no transcendental
                dy=r(c.B, 1, c.H, c.W), addend=r(c.B, c.C, c.H, c.W))


# ------------------------------------------------------------------------------------------------ where an element lies
def pixel_class(c, y, x):
    """of a pixel: the first that holds of corner, second line, border line, tile seam, interior"""
    by, bx = y in (0, c.H - 1), x in (0, c.W - 1)
    sy, sx = y in (1, c.H - 2), x in (1, c.W - 2)
    if (by or sy) and (bx or sx):
        return "corner"
    if sy or sx:
        return "second line"
    if by or bx:
        return "border line"
    P = pxb(c.C)
    if y % TH in (0, TH - 1) or x % P in (0, P - 1):
        return "tile seam"
    return "interior"
