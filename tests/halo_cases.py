"""Shapes for the halo-tile convolution kernels (csrc/conv_halo.hip), chosen by where the image border falls relative to the kernels' fixed
grids -- the 8 x 32 output tile, the 16-pixel MFMA fragment, the two-row wavefront slice -- not by workload.  Shared by tests/test_halo_cpu.py
(the planner takes every (case, form) to the halo family with this file's tile arithmetic; every class below is hit) and
tests/test_halo_gpu.py (the launches, against tests/halo_ref.py).

A case is (B, H, W, C, Cout) of a 3x3 stride-1 convolution C -> Cout on an H x W image; a form is one way the kernels run it."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

HT_H, HT_W, FRAG, SLICE = 8, 32, 16, 2      # output tile, MFMA fragment width, rows of a wavefront
MAX_SPLITS = 512                            # weight gradient: workgroups walk tiles grid-stride beyond this many
T_GENERAL, T_NINE_TAP = 0x200, 0x400       # desc.tile bits: the general kernels; the 9-tap halo kernel on an upsampled source

Case = namedtuple("Case", "B H W C Cout")


def tiles_y(c):
    return -(-c.H // HT_H)


def tiles_x(c):
    return -(-c.W // HT_W)


def tiles(c):
    return c.B * tiles_y(c) * tiles_x(c)


def tile_origin(c, k):
    """(n, y0, x0) of linear tile k, as the kernels decode it"""
    return k // (tiles_x(c) * tiles_y(c)), (k // tiles_x(c)) % tiles_y(c) * HT_H, k % tiles_x(c) * HT_W


def tiles_per_workgroup(c):
    """weight gradient: how many tiles workgroup g of min(tiles, 512) walks"""
    n = min(tiles(c), MAX_SPLITS)
    return [len(range(g, tiles(c), n)) for g in range(n)]


# ------------------------------------------------------------------------------------------------ alignment classes
# name -> (predicate, an even H x W can be in it)
Cls = namedtuple("Cls", "name pred even_ok")
ROW_CLASSES = (
    Cls("H == 2", lambda c: c.H == 2, True),
    Cls("H == 3", lambda c: c.H == 3, False),
    Cls("H % 8 == 0", lambda c: c.H % HT_H == 0, True),
    Cls("H % 8 == 1", lambda c: c.H % HT_H == 1, False),
    Cls("H % 8 == 2", lambda c: c.H % HT_H == 2, True),
    Cls("H odd: H-2, H-1 in different slices", lambda c: c.H > 3 and (c.H - 2) // SLICE != (c.H - 1) // SLICE, False),
    Cls("rows 1, H-2 in one tile", lambda c: c.H > 3 and 1 // HT_H == (c.H - 2) // HT_H, True),
    Cls("rows 1, H-2 in different tiles", lambda c: 1 // HT_H != (c.H - 2) // HT_H, True),
)
COL_CLASSES = (
    Cls("W == 2", lambda c: c.W == 2, True),
    Cls("W == 3", lambda c: c.W == 3, False),
    Cls("W < 16", lambda c: 3 < c.W < FRAG, True),
    Cls("16 < W < 32", lambda c: FRAG < c.W < HT_W, True),
    Cls("W % 32 == 0", lambda c: c.W % HT_W == 0, True),
    Cls("W % 32 == 1", lambda c: c.W % HT_W == 1, False),
    Cls("W % 32 == 2", lambda c: c.W % HT_W == 2 and c.W > 2, True),
    Cls("W % 16 == 1, W % 32 != 1", lambda c: c.W % FRAG == 1 and c.W % HT_W != 1, False),
    Cls("W % 16 == 2, W % 32 != 2", lambda c: c.W % FRAG == 2 and c.W % HT_W != 2, True),
)
# merged-tap forms (even sizes): the 6 x 18 low-resolution halo with one source row / column
UP_CLASSES = (
    Cls("H / 2 == 1", lambda c: c.H == 2, True),
    Cls("W / 2 == 1", lambda c: c.W == 2, True),
    Cls("last tile: one low-resolution row (H % 8 == 2)", lambda c: c.H % HT_H == 2 and c.H > 2, True),
    Cls("last tile: one low-resolution column (W % 32 == 2)", lambda c: c.W % HT_W == 2 and c.W > 2, True),
)

# ------------------------------------------------------------------------------------------------ kernel forms
# kind: fwd / adj / wgrad; even: needs even H and W (an upsampled source, the 2x2 pool); tile: desc.tile
Form = namedtuple("Form", "name kind even tile reflect up")
FORMS = (
    Form("fwd zero", "fwd", False, 0, False, False),
    Form("fwd reflect", "fwd", False, 0, True, False),
    Form("fwd up merged", "fwd", True, 0, True, True),
    Form("fwd up 9-tap", "fwd", True, T_NINE_TAP, True, True),
    Form("adj", "adj", False, 0, True, False),
    Form("adj n_begin 0|16", "adj", False, 0, True, False),
    Form("adj pool elu' addend", "adj", True, 0, True, False),
    Form("wgrad bias", "wgrad", False, 0, True, False),
    Form("wgrad no bias", "wgrad", False, 0, False, False),
    Form("wgrad up merged", "wgrad", True, 0, True, True),
    Form("wgrad up 9-tap", "wgrad", True, T_NINE_TAP, True, True),
    Form("wgrad dy_choff", "wgrad", False, 0, True, False),
)
FORM = {f.name: f for f in FORMS}
CHOFF, CDY_EXTRA = 8, 12                    # "wgrad dy_choff": dy is channels [8, 8 + Cout) of a pixel of Cout + 12


def up16(v):
    return (v + 15) // 16 * 16


def applies(form, c):
    if form.even and (c.H % 2 or c.W % 2):
        return False
    if form.name == "adj n_begin 0|16":
        return c.C == 32
    if form.name == "adj pool elu' addend":
        return not (c.C == 32 and c.Cout > 16)      # 32 -> 32 pooled: mcav.nn takes the 4x4 stride-2 form on the general kernels instead
    if form.kind == "wgrad":
        if c.C == 32 and c.Cout > 16:               # 144 filter registers per lane: the planner declines
            return False
        if form.name == "wgrad up merged":
            return c.C == 16 and c.Cout <= 16       # the one merged-tap instantiation
    return True


def launch_shape(form, c):
    """(kernel channels, outputs of the launch) as the host code sets them up: an adjoint reads dy padded to 16 channels and writes C."""
    if form.kind == "adj":
        return up16(c.Cout), (16 if form.name == "adj n_begin 0|16" else c.C)
    return c.C, c.Cout


def instantiation(form, c):
    """which template instantiation (C, NF) runs, and in how many launches: '16x1', '16x2', '32x1', '32x1 twice'; '+mask' when the last
    16-channel block is partly masked"""
    kc, n = launch_shape(form, c)
    if form.kind == "wgrad":
        return "%dx%d" % (kc, 2 if n > 16 else 1)
    nf = 2 if (n > 16 and kc == 16) else 1
    launches = -(-n // (16 * nf))
    return "%dx%d%s%s" % (kc, nf, " twice" if launches == 2 else "", " +mask" if n % 16 else "")


def launches(form, c):
    kc, n = launch_shape(form, c)
    return -(-n // (16 * (2 if (n > 16 and kc == 16) else 1)))


CHANNELS = tuple((C, Cout) for C in (16, 32) for Cout in (8, 16, 24, 32))


def instantiations_of(form):
    """every instantiation the form can reach over C in {16, 32}, Cout in {8, 16, 24, 32}"""
    even = Case(1, 8, 32, 0, 0)
    return sorted({instantiation(form, even._replace(C=C, Cout=Cout)) for C, Cout in CHANNELS if applies(form, even._replace(C=C, Cout=Cout))})


# ------------------------------------------------------------------------------------------------ the cases
CASES = tuple(Case(*c) for c in (
    # even sizes, 32 -> 16 (every forward / adjoint form applies): one grid of every residue modulo 8
    (2, 16, 64, 32, 16),      # 8 tiles; H % 8 == 0, W % 32 == 0
    (1, 2, 2, 32, 16),        # 1 tile; H == W == 2: both row rules and both column rules on two lines
    (2, 8, 32, 32, 16),       # 2
    (3, 4, 6, 32, 16),        # 3; W < 16
    (1, 10, 34, 32, 16),      # 4; the last tiles hold one low-resolution row / column; rows 1 and H - 2 in different tiles
    (5, 2, 4, 32, 16),        # 5
    (3, 10, 18, 32, 16),      # 6; W = 18: W - 2 and W - 1 in the second fragment
    (7, 4, 2, 32, 16),        # 7; W == 2
    # odd sizes and the remaining alignments
    (1, 3, 3, 16, 8),         # H == W == 3: lines 1 = H - 2
    (2, 3, 17, 32, 16),       # W = 17: W - 1 alone in the second fragment
    (1, 9, 33, 32, 8),        # H - 1 alone in the second tile row, W - 1 alone in the second tile column
    (1, 17, 49, 16, 16),      # W = 49; H - 1 alone in the third tile row
    (1, 17, 50, 32, 24),      # W = 50
    (3, 17, 66, 16, 8),       # 27 tiles
    (2, 9, 35, 16, 32),
    (1, 5, 12, 16, 16),       # W < 16, H odd
    (1, 6, 24, 32, 24),       # 16 < W < 32; 32 -> 24 from an even size: the second launch partly masked
    (1, 7, 21, 16, 24),       # 16 < W < 32, odd
    (1, 16, 49, 32, 32),      # 32 -> 32: two launches of 16
    (2, 2, 34, 16, 32),       # H == 2 with a one-column last tile
    (1, 10, 18, 16, 16),      # the merged-tap weight gradient's shapes: 16 -> 16 ...
    (2, 10, 2, 16, 16),
    (1, 2, 66, 16, 8),
    (2, 8, 64, 16, 16),
    (1, 16, 4, 16, 24),
    (1, 11, 31, 32, 24),      # 32 -> 24: the second launch partly masked
    (2, 7, 16, 32, 32),
    (1, 12, 20, 16, 32),
    (1, 3, 65, 16, 32),       # H == 3 across three tile columns
    (1, 13, 3, 32, 8),        # W == 3 across two tile rows
    (1, 8, 50, 32, 32),
    (2, 6, 12, 16, 16),       # W < 16, even
    (1, 4, 20, 32, 8),
))

# more than 512 tiles: 33 x 4 x 4 = 528, so workgroups 0 .. 15 walk two tiles (the second one in image 32) and 16 .. 511 one
WALK_CASES = (
    (Case(33, 32, 128, 16, 16), ("wgrad bias", "wgrad up merged")),
    (Case(33, 32, 128, 16, 24), ("wgrad bias",)),
    (Case(33, 32, 128, 32, 8), ("wgrad no bias",)),
)
WALK_TILES = (5, 517, 527)                  # walked first, walked second (>= 512), the very last


def case_id(c):
    return "%dx%dx%d_%dto%d" % c


# ------------------------------------------------------------------------------------------------ dy supports of the weight gradient
def support_mask(c, support):
    """[B, 1, H, W] bool: where dy is non-zero.  'band': rows {0, 1, H-2, H-1} and columns {0, 1, W-2, W-1} of the last image;
    ('tile', k): exactly the k-th 8 x 32 tile; 'dense'."""
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
        m[n, 0, y0:y0 + HT_H, x0:x0 + HT_W] = True
    return m


def supports(c):
    """the supports of an ordinary case: those judged by the elementwise envelope, then 'dense' (judged in the max-norm)"""
    out = ["band", ("tile", tiles(c) - 1)]
    if tiles(c) > 1:
        out.append(("tile", 0))
    return out + ["dense"]


# ------------------------------------------------------------------------------------------------ inputs (float32, NCHW, on the CPU)
@functools.lru_cache(maxsize=None)
def inputs(c):
    g = torch.Generator().manual_seed(1000 + 7 * c.B + 131 * c.H + 17 * c.W + 3 * c.C + c.Cout)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    d = dict(x=r(c.B, c.C, c.H, c.W), w=r(c.Cout, c.C, 3, 3) * (2.0 / (9 * c.C)) ** 0.5, b=0.1 * r(c.Cout), dy=r(c.B, c.Cout, c.H, c.W))
    d["xl"] = r(c.B, c.C, max(c.H // 2, 1), max(c.W // 2, 1))                  # the half-resolution source of the upsampled forms
    d["aux"] = F.elu(r(c.B, c.C, max(c.H // 2, 1), max(c.W // 2, 1)))          # the producer's ELU output
    d["add"] = r(c.B, c.C, max(c.H // 2, 1), max(c.W // 2, 1))
    d["wide"] = r(c.B, c.Cout + CDY_EXTRA, c.H, c.W)                           # what surrounds dy in a wider pixel
    return d


# ------------------------------------------------------------------------------------------------ descriptors, as mcav.nn fills them
X, WT, Y, BIAS, AUX, ADD, DY, DW, DB = (0x1000 * (i + 1) for i in range(9))      # stand-ins for device addresses (the planner reads none)


def igemm_desc(N, form, c, tile=None, n_begin=0):
    """mcav.nn.conv_fwd / conv_dgrad's descriptor of (form, case)"""
    d = N.IgemmDesc()
    tile = form.tile if tile is None else tile
    if form.kind == "fwd":
        d.x1, d.B, d.Hs, d.Ws, d.C1, d.C2, d.up1 = X, c.B, c.H, c.W, c.C, 0, int(form.up)
        d.w, d.kh, d.kw, d.Np, d.Kp = WT, 3, 3, up16(c.Cout), c.C
        d.mode, d.stride, d.sign, d.offset, d.pad_mode = N.G_DIRECT, 1, 1, -1, (N.PAD_REFLECT if form.reflect else N.PAD_ZERO)
        d.y, d.Hd, d.Wd, d.Cd, d.n_begin, d.n_count, d.y_choff = Y, c.H, c.W, c.Cout, 0, c.Cout, 0
        d.bias, d.act, d.tile, d.groups = BIAS, N.ACT_NONE, tile, 1
        return d
    pool = form.name == "adj pool elu' addend"
    n_count = launch_shape(form, c)[1]
    d.x1, d.B, d.Hs, d.Ws, d.C1, d.C2, d.up1 = X, c.B, c.H, c.W, up16(c.Cout), 0, 0
    d.w, d.kh, d.kw, d.Np, d.Kp = WT, 3, 3, up16(c.C), up16(c.Cout)
    d.mode, d.stride, d.sign, d.offset, d.pad_mode = N.G_ADJ_REFLECT, 1, -1, 1, N.PAD_ZERO
    d.y, d.Hd, d.Wd, d.Cd, d.n_begin, d.n_count, d.y_choff = Y, c.H, c.W, n_count, n_begin, n_count, 0
    d.act, d.tile, d.pool = N.ACT_NONE, tile, int(pool)
    if pool:
        d.dact_aux, d.dact, d.addend = AUX, N.ACT_ELU, ADD
    return d


def wgrad_desc(N, form, c, x=X, dy=DY, dw=DW, db=DB):
    """mcav.nn.conv_wgrad's descriptor of (form, case); 'wgrad dy_choff' is the same launch on channels [CHOFF, CHOFF + Cout) of a wider dy"""
    d = N.WgradDesc()
    choff = form.name == "wgrad dy_choff"
    d.x1, d.B, d.Hs, d.Ws, d.C1, d.C2, d.up1 = x, c.B, c.H, c.W, c.C, 0, int(form.up)
    d.kh, d.kw, d.Kp, d.mode = 3, 3, c.C, N.G_DIRECT
    d.stride, d.sign, d.offset, d.pad_mode = 1, 1, -1, (N.PAD_REFLECT if form.reflect else N.PAD_ZERO)
    d.dy, d.Hd, d.Wd, d.Cdy, d.dy_choff = dy, c.H, c.W, (c.Cout + CDY_EXTRA if choff else c.Cout), (CHOFF if choff else 0)
    d.Cout, d.Cin, d.dw_oihw, d.accumulate = c.Cout, c.C, dw, 1
    d.dbias = None if form.name == "wgrad no bias" else db
    d.tile, d.mma = form.tile, 0
    return d


def expected_igemm_route(N, form, c):
    """(family, variant, workgroups) from this file's tile arithmetic"""
    variant = (N.RV_ADJ | N.RV_REFLECT) if form.kind == "adj" else (N.RV_UPM if form.name == "fwd up merged" else 0)
    return N.IGEMM_HALO, variant, tiles(c) * launches(form, c)


def expected_wgrad_route(N, form, c):
    """(family, variant, workgroups, splits)"""
    n = min(tiles(c), MAX_SPLITS)
    return N.WGRAD_HALO, (N.RV_UPM if form.name == "wgrad up merged" else 0), n, n


# ------------------------------------------------------------------------------------------------ where an element lies
def pixel_class(c, y, x):
    """of a full-resolution output pixel: the first that holds of corner, second line, border line, tile seam, fragment seam, interior"""
    by, bx = y in (0, c.H - 1), x in (0, c.W - 1)
    sy, sx = y in (1, c.H - 2), x in (1, c.W - 2)
    if (by or sy) and (bx or sx):
        return "corner"
    if sy or sx:
        return "second line"
    if by or bx:
        return "border line"
    if y % HT_H in (0, HT_H - 1) or x % HT_W in (0, HT_W - 1):
        return "tile seam"
    if x % FRAG in (0, FRAG - 1):
        return "fragment seam"
    return "interior"
