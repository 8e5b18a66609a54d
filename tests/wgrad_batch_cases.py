"""One gradient bucket of weight-gradient descriptors for the batched slab reduction (mcav_wgrad_deferred + mcav_wgrad_reduce_plan +
mcav_wgrad_reduce_multi), shared by tests/test_wgrad_batch_cpu.py (the planner's answers: no tensors, small constants stand in for device
addresses) and tests/test_wgrad_batch_gpu.py (the launches).

The bucket mixes both reduction levels -- slabs of more than 8 pixel splits are summed in two levels (wgrad_presum_multi_kernel, then
wgrad_reduce_multi_kernel on the group sums), the others in one -- every kernel family that writes a slab (fp32 tiles, halo, stem, the bf16
patch kernel in its split and its one-plane form) and the two launches of a decoder level into one [Cout][C1 + C2][3][3] gradient.  The family,
the number of splits and whether a case is grouped are STATED here and asserted against mcav_wgrad_route by the CPU test, so a change of the
planner that empties one side of the mix fails there instead of silently thinning the GPU test.

A case carries WCase's fields (tests/test_conv_contract_gpu.py: wgrad_desc / wgrad_operands read them) and, beside them, the decoder fields
upm / cin_total / ci_offset, `share`: the cases of one decoder level (same dy, same gradient tensor), and what the planner must answer."""
import random

Z, R = 0, 1                                                   # pad modes
FP32, HALO, STEM, BF16_PATCH, BF16_TILE = range(5)            # enum mcav_wgrad_family
X1, DY, DW, DB = 0x1000, 0x2000, 0x3000, 0x4000               # stand-ins for device addresses (the planner dereferences nothing)


def up16(v):
    return (v + 15) // 16 * 16


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


class BCase:
    """conv = (B, H, W, Cin, Cout, k, stride, pad, pad_mode) with H x W the convolution's input, as tests/test_conv_contract_gpu.py:WCase."""

    def __init__(self, name, conv, family, splits, stored=None, up=False, smallc=False, bias=True, tile=0, mma=0, upm=0, cin_total=0, ci_offset=0,
                 share=None):
        self.name, self.conv, self.family, self.splits = name, conv, family, splits
        self.stored = stored if stored is not None else conv[3]
        self.up, self.smallc, self.bias, self.tile, self.mma = up, smallc, bias, tile, mma
        self.upm, self.cin_total, self.ci_offset, self.share = upm, cin_total, ci_offset, share
        self.planes, self.generic_ok = 0, False

    @property
    def grouped(self):
        """more than 8 splits: the two-level reduction (csrc/conv_plan.h: wgrad_slab_sizes)"""
        return self.splits > 8

    @property
    def groups(self):
        """-> (groups, per_group): eight groups at most, the last one ragged; (0, 0) on the single-level path"""
        if not self.grouped:
            return 0, 0
        per = (self.splits + 7) // 8
        return (self.splits + per - 1) // per, per

    @property
    def taps_out(self):
        return self.conv[5] ** 2

    @property
    def slab_taps(self):
        return 16 if self.upm else self.taps_out

    @property
    def kp(self):
        return 4 if self.smallc else up16(self.stored)


# B = 2 everywhere.  splits: max_splits = ceil(Mpix / 256) caps wgrad_fill_splits on these small maps; the halo / stem kernels bring their own.
BUCKET = [
    BCase("64->64 3x3 zero pad, 24x48", (2, 24, 48, 64, 64, 3, 1, 1, Z), FP32, 9),                          # 9 splits: 5 groups of 2, the last holds 1
    BCase("256->256 3x3, 3x10", (2, 3, 10, 256, 256, 3, 1, 1, Z), FP32, 1),
    BCase("64->128 1x1 stride 2, 9x15", (2, 9, 15, 64, 128, 1, 2, 0, Z), FP32, 1),
    BCase("256->12 1x1, 3x5", (2, 3, 5, 256, 12, 1, 1, 0, Z), FP32, 1),                                     # Cout below slabN = 16
    BCase("depth stem", (2, 45, 70, 3, 64, 7, 2, 3, Z), STEM, 24, stored=4, smallc=True, bias=False),
    BCase("pose stem", (2, 45, 70, 9, 16, 7, 2, 3, Z), STEM, 24, stored=16),
    BCase("16->16 3x3 reflect, 24x80 (halo)", (2, 24, 80, 16, 16, 3, 1, 1, R), HALO, 18),
    BCase("decoder level, skip half", (2, 12, 20, 64, 64, 3, 1, 1, R), FP32, 2, cin_total=128, ci_offset=64, share="dec"),
    BCase("decoder level, merged-tap half", (2, 12, 20, 64, 64, 3, 1, 1, R), FP32, 1, up=True, bias=False, upm=1, cin_total=128, ci_offset=0,
          share="dec"),
    BCase("64->64 3x3 split (patch kernel)", (2, 12, 20, 64, 64, 3, 1, 1, Z), BF16_PATCH, 8, mma=2),
    BCase("64->64 3x3 bf16", (2, 12, 20, 64, 64, 3, 1, 1, Z), BF16_PATCH, 8, mma=1),
]


def orders():
    """name -> the bucket's cases in launch order: as listed, reversed, one fixed shuffle"""
    idx = list(range(len(BUCKET)))
    shuffled = idx[:]
    random.Random(20).shuffle(shuffled)
    return {"as listed": idx, "reversed": idx[::-1], "shuffled": shuffled}


def plan_desc(N, c, x=X1, dy=DY, dw=DW, dbias=DB, accumulate=0):
    """The case's mcav_wgrad_desc with the given addresses (the defaults: constants for the planner entries)."""
    B, H, W, Cin, Cout, k, stride, pad, pm = c.conv
    d = N.WgradDesc()
    d.x1, d.B, d.Hs, d.Ws, d.C1, d.up1 = x, B, H, W, c.stored, int(c.up)
    d.kh, d.kw, d.Kp = k, k, c.kp
    d.mode = N.G_SMALLC if c.smallc else N.G_DIRECT
    d.stride, d.sign, d.offset, d.pad_mode = stride, 1, -pad, pm
    d.dy, d.Hd, d.Wd, d.Cdy, d.dy_choff = dy, out_size(H, k, stride, pad), out_size(W, k, stride, pad), Cout, 0
    d.Cout, d.Cin = Cout, Cin
    d.dw_oihw, d.accumulate, d.dbias = dw, accumulate, (dbias if c.bias else None)
    d.tile, d.mma = c.tile, c.mma
    d.upm, d.Cin_total, d.ci_offset = c.upm, c.cin_total, c.ci_offset
    return d

