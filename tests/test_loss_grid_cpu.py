"""CPU: the planner of the fused L1 loss launches (csrc/warp_loss.hip: l1_grid, through the query mcav_warp_loss_l1_grid with slots > 0,
which needs no device) against what the kernel body (csrc/warp_loss_l1_body.h) relies on, and a Python restatement of the body's tile walk.
tests/test_loss_walk_gpu.py runs the kernels in the regimes this planner produces."""
import ctypes
import itertools

import numpy as np
import pytest

TW, T2H, TH8 = 32, 16, 8                  # a tile of the fused L1 kernels: 32 x 16 pixels, two 8-row halves, 256 threads
SLAB = 40                                 # floats per workgroup in the slab
MAX_B = 4095
MIN_REPROJ, AUTOMASK, SSIM = 32, 64, 16

BS = [1, 2, 3, 12, 64, 255, 256, 257, 768, 1024, 4095]
SHAPES = [(3, 3), (16, 32), (17, 33), (72, 130), (192, 640), (320, 1024), (375, 1242)]
SLOTS = [1] + [p * c for p, c in itertools.product((2, 3), (64, 104, 256, 304))]


def ntiles_of(H, W):
    return ((W + TW - 1) // TW), ((H + T2H - 1) // T2H)


def align_up(v, a=256):
    return (v + a - 1) // a * a


@pytest.fixture(scope="module")
def h():
    from mcav import lib as L
    return L.lib()


def query(h, B, H, W, flags, stereo, slots):
    g0, g1 = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = h.mcav_warp_loss_l1_grid(B, H, W, flags, stereo, slots, ctypes.byref(g0), ctypes.byref(g1))
    return rc, g0.value, g1.value


@pytest.fixture(scope="module")
def sweep(h):
    out = {}
    for B, (H, W), slots, stereo in itertools.product(BS, SHAPES, SLOTS, (0, 1)):
        rc, g0, g1 = query(h, B, H, W, 0, stereo, slots)
        assert rc == 0, (B, H, W, slots, stereo, rc)
        out[(B, H, W, slots, stereo)] = (g0, g1)
    return out


def slab_region_bytes(h, B, H, W):
    """The slab region of mcav_warp_loss_workspace_bytes(B, H, W), from ws_layout restated: tickets (4096 words), the per-sample constants,
    the slab, 2 doubles per sample, each piece rounded up to 256 bytes.  The size of a sample's constants is read off the B = 64 answer
    (every piece is a multiple of 256 there)."""
    ntx, nty = ntiles_of(H, W)
    rows = max(((W + 31) // 32) * ((H + 7) // 8), ntx * 2 * nty)
    pc64 = h.mcav_warp_loss_workspace_bytes(64, H, W) - 4 * (MAX_B + 1) - 4 * SLAB * 64 * rows - 16 * 64
    assert pc64 > 0 and pc64 % (64 * 4) == 0, pc64
    pc = pc64 // 64
    region = h.mcav_warp_loss_workspace_bytes(B, H, W) - 4 * (MAX_B + 1) - align_up(pc * B) - align_up(16 * B)
    assert region == align_up(4 * SLAB * B * rows), (B, H, W, region)
    return region


def test_grid_is_what_the_kernel_body_relies_on(h, sweep):
    for (B, H, W, slots, stereo), (g0, g1) in sweep.items():
        ntx, nty = ntiles_of(H, W)
        case = (B, H, W, slots, stereo, g0, g1)
        assert 1 <= g0 <= ntx * nty and 1 <= g1 <= ntx * nty, case           # "the host keeps G <= ntiles": nmine >= 1 for every workgroup
        assert (g0 + g1) * B <= slots or g0 + g1 <= 2, case                  # one resident generation, or the smallest grid there is
    for B, (H, W) in itertools.product(BS, SHAPES):
        region = slab_region_bytes(h, B, H, W)
        worst = max(sum(sweep[(B, H, W, s, st)]) for s in SLOTS for st in (0, 1))
        assert 4 * SLAB * worst * B <= region, (B, H, W, worst, region)


def test_query_repeats_itself_and_ignores_unrelated_flags(h, sweep):
    for (B, H, W, slots, stereo), g in sweep.items():
        assert query(h, B, H, W, 0, stereo, slots) == (0,) + g
    for flags in (MIN_REPROJ, AUTOMASK, MIN_REPROJ | AUTOMASK, 1 | 2 | 4 | 8):       # slots given: the instantiation no longer matters
        assert query(h, 12, 192, 640, flags, 0, 768)[1:] == sweep[(12, 192, 640, 768, 0)]


def test_query_refuses_what_the_launch_refuses(h):
    ok = (12, 72, 130, 0, 0, 512)
    assert query(h, *ok)[0] == 0
    for bad in [(4096, 72, 130, 0, 0, 512), (0, 72, 130, 0, 0, 512), (12, 2, 130, 0, 0, 512), (12, 72, 2, 0, 0, 512),
                (12, 72, 130, 128, 0, 512), (12, 72, 130, SSIM, 0, 512), (12, 72, 130, SSIM | AUTOMASK, 1, 512), (12, 72, 130, 0, 0, -1)]:
        assert query(h, *bad) == (-1, -7, -7), bad                           # MCAV_E_INVALID, the outputs untouched
    assert h.mcav_warp_loss_l1_grid(12, 72, 130, 0, 0, 512, None, None) == -1


def walk(H, W, G):
    """The body's `pixel(j, ...)` for every workgroup g < G, thread and j < npix -> (count of visits per pixel [H, W], all tyi exact).
    t = g + (j >> 1) * G; tyi = int((t + 0.5f) * (1.0f / ntx)) in float32; txi = t - tyi * ntx; x = txi * 32 + tx;
    y = tyi * 16 + (j & 1) * 8 + ty0; the pixel is taken when (j >> 1) < nmine && x < W && y < H."""
    ntx, nty = ntiles_of(H, W)
    ntiles = ntx * nty
    inv_ntx = np.float32(1.0) / np.float32(ntx)
    count = np.zeros((H, W), dtype=np.int64)
    exact = True
    tx, ty0 = np.arange(256) & 31, np.arange(256) >> 5
    for g in range(G):
        nmine = (ntiles - g + G - 1) // G
        assert nmine >= 1
        j = np.arange(2 * nmine + 4)                                         # (the loops look up to three pixels past the end)
        t = g + (j >> 1) * G
        tyi = ((t.astype(np.float32) + np.float32(0.5)) * inv_ntx).astype(np.int32).astype(np.int64)
        live = (j >> 1) < nmine
        exact = exact and bool((tyi[live] == t[live] // ntx).all())
        txi = t - tyi * ntx
        x = txi[:, None] * TW + tx[None, :]
        y = tyi[:, None] * T2H + (j & 1)[:, None] * TH8 + ty0[None, :]
        take = live[:, None] & (x < W) & (y < H) & (x >= 0) & (y >= 0)
        np.add.at(count, (y[take], x[take]), 1)
    return count, exact


def test_tile_walk_visits_every_pixel_once(sweep):
    seen = {}
    for (B, H, W, slots, stereo), g in sweep.items():
        seen.setdefault((H, W), set()).update(g)
    for (H, W), gs in seen.items():
        ntiles = int(np.prod(ntiles_of(H, W)))
        assert 1 in gs                                                       # (one workgroup walks the whole sample)
        for G in sorted(gs):
            count, exact = walk(H, W, G)
            assert exact, "float32 tile row differs from t // ntx at %dx%d, G = %d" % (H, W, G)
            assert int(count.min()) == 1 and int(count.max()) == 1, "%dx%d, G = %d (%d tiles): a pixel is visited %d .. %d times" % (
                H, W, G, ntiles, count.min(), count.max())


def test_float32_tile_row_is_exact():
    """int((t + 0.5f) * (1.0f / ntx)) == t // ntx for every ntx <= 512 and t < 600 ntx: images up to 16384 x 9600 pixels."""
    for ntx in range(1, 513):
        t = np.arange(600 * ntx, dtype=np.int64)
        tyi = ((t.astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(ntx))).astype(np.int32)
        assert bool((tyi == t // ntx).all()), ntx
