"""GPU: the one-launch filter repack (include/mcav_conv.h: mcav_pack_weights_multi; mcav.nn.PackRegistry), which derives every packed filter
copy after every optimiser step, against tests/pack_ref.py -- bit for bit, padding zeros included: the copies are data movement, round-to-
nearest-even conversions and float32 sums in a stated order.

One hand-built record table mixes all kinds in one launch -- fp32 forward and transposed, bf16, the three split planes, merged-tap forward and
merged-tap adjoint -- on filters chosen for the kernel's paths: a forward filter too long for the LDS staging (Cin * taps > 5120), transposed
tiles of 1, 3 and 8 input channels (49, 25 and 1 / 9 taps) with a ragged last tile, Cout and Cin that are no multiples of 16, the 4-channel stem
record whose row stride (208) exceeds taps * Kp (196), merged-tap records whose element count is no multiple of a workgroup's share.  Every
destination is a guarded window that starts as sentinels (tests/guarded.py).  Each destination must also equal what the single-filter entry
points (the first step's path) write for the same filter.  The registry test goes through ConvSpec / PackRegistry themselves."""
import ctypes
import gc

import pytest
import torch

import pack_ref as R
from guarded import Guarded, P, is_sentinel

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Rec:
    """One record: filter f of FILTERS as `kind` ('f', 'b' fp32 forward / transposed; + '16' bf16; + '16s' planes; 'um' / 'ua' merged taps)."""

    def __init__(self, f, kind, Kp=None, C1=0, Np=None):
        self.f, self.kind, self.C1 = f, kind, C1
        Cout, Cin, k = FILTERS[f]
        self.Cout, self.Cin, self.k, self.taps = Cout, Cin, k, k * k
        self.base = kind[0] if kind not in ("um", "ua") else kind
        self.h = 3 if kind.endswith("16s") else (1 if kind.endswith("16") else 0)
        if kind == "um":
            self.Np, self.Kp, self.flags, self.shape = Np or R.up16(Cout), 0, 8, (4 * (Np or R.up16(Cout)), 4 * C1)
        elif kind == "ua":
            self.Np, self.Kp, self.flags = Np or R.up16(C1), R.up16(Cout), 16
            self.shape = (self.Np, 16 * self.Kp)
        elif self.base == "b":
            self.Np, self.Kp = R.up16(Cin), R.up16(Cout)
            self.flags, self.shape = 1 | (4 if self.h == 3 else 2 if self.h else 0), (self.Np, self.taps * self.Kp)
        else:
            self.Np, self.Kp = R.up16(Cout), Kp or R.up16(Cin)
            self.flags, self.shape = (4 if self.h == 3 else 2 if self.h else 0), (self.Np, R.kstride(self.taps, self.Kp))

    @property
    def name(self):
        return "%s of %d<-%d %dx%d%s" % (self.kind, self.Cout, self.Cin, self.k, self.k, " Kp %d" % self.Kp if self.Kp == 4 else "")

    def want(self, w):
        if self.kind == "um":
            return R.pack_upmerge(w, self.C1, self.Np).reshape(self.shape)
        if self.kind == "ua":
            return R.pack_upmerge_adj(w, self.C1, self.Np, self.Kp)
        p = R.pack_transposed(w) if self.base == "b" else R.pack_forward(w, self.Np, self.Kp)
        return R.planes(p) if self.h == 3 else (R.to_bf16(p) if self.h else p)

    def window(self):
        """the destination: a float32 window of sentinels; bf16 destinations are read through a 2-byte view of it"""
        n = self.shape[0] * self.shape[1] * max(self.h, 1)
        return Guarded((n // 2 if self.h else n,), band=256)

    def read(self, g):
        t = g.cpu()
        if self.h:
            return t.view(torch.bfloat16).view(self.h * self.shape[0], self.shape[1])
        return t.view(self.shape)


# Cout, Cin, k
FILTERS = [(64, 64, 3), (12, 9, 7), (32, 16, 5), (128, 64, 1), (16, 576, 3), (64, 3, 7), (32, 96, 3), (16, 32, 3), (12, 40, 3)]


def records():
    return [
        Rec(0, "f"), Rec(0, "b"), Rec(0, "f16"), Rec(0, "b16"), Rec(0, "f16s"), Rec(0, "b16s"),
        Rec(1, "f"), Rec(1, "b"), Rec(1, "f16s"), Rec(1, "b16"),                    # 49 taps: transposed tiles of ONE input channel
        Rec(2, "f"), Rec(2, "b"), Rec(2, "b16s"),                                   # 25 taps: tiles of 3, the last one holds a single channel of 16
        Rec(3, "f"), Rec(3, "b"), Rec(3, "b16"),                                    # 1 tap: tiles capped at 8; two 64-column blocks
        Rec(4, "f"), Rec(4, "f16"), Rec(4, "f16s"), Rec(4, "b"),                    # Cin * taps = 5184 > 5120: the forward copy is not staged in LDS
        Rec(5, "f", Kp=4), Rec(5, "f16", Kp=4), Rec(5, "f"),                        # the stem record: Kstride 208 > 196 = taps * Kp
        Rec(6, "um", C1=32), Rec(6, "ua", C1=32),
        Rec(7, "um", C1=16), Rec(7, "ua", C1=16),                                   # Cout = Np = 16
        Rec(8, "um", C1=20), Rec(8, "ua", C1=20, Np=32),                            # 5120 merged elements: 2.5 workgroups; rows and columns of zeros
    ]


def bits_equal(a, b):
    if a.dtype == torch.bfloat16:
        return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def where(a, b):
    bad = ((a.float() != b.float()) | (a.float().isnan() != b.float().isnan())).nonzero()
    return "%d elements differ, the first at %s: got %r, want %r" % (len(bad), tuple(bad[0].tolist()), float(a[tuple(bad[0])]), float(b[tuple(bad[0])]))


class Filters:
    def __init__(self):
        g = torch.Generator().manual_seed(31)
        self.cpu = [torch.randn(co, ci, k, k, generator=g) * 10.0 ** float(torch.randint(-2, 3, (1,), generator=g)) for co, ci, k in FILTERS]
        self.dev = [w.to(DEV) for w in self.cpu]
        self.want = {}

    def wanted(self, r):
        key = (r.f, r.kind, r.Kp, r.Np, r.C1)
        if key not in self.want:
            self.want[key] = r.want(self.cpu[r.f])
        return self.want[key]


@pytest.fixture(scope="module")
def filters():
    return Filters()


def blocks_of(h, r):
    """as PackRegistry._build asks: the transposed bit alone for the ordinary copies, the merged-tap bit with C1 in `taps`"""
    if r.kind in ("um", "ua"):
        return h.mcav_pack_weights_blocks(r.C1, r.flags, r.Np, max(r.Kp, 1))
    return h.mcav_pack_weights_blocks(r.taps, r.flags & 1, r.Np, r.Kp)


def multi(filters, recs):
    """ONE mcav_pack_weights_multi over `recs` -> their destination windows"""
    from mcav import lib as L
    from mcav import nn as N
    h = L.lib()
    items = (N._PackItem * len(recs))()
    dsts, blk = [], 0
    for it, r in zip(items, recs):
        g = r.window()
        it.src, it.dst = P(filters.dev[r.f]), P(g)
        it.Cout, it.Cin, it.taps, it.transposed = r.Cout, r.Cin, (r.C1 if r.kind in ("um", "ua") else r.taps), r.flags
        it.Np, it.Kp, it.Kstride, it.first_block = r.Np, r.Kp, (0 if r.kind in ("um", "ua") else r.shape[1]), blk
        n = blocks_of(h, r)
        assert n > 0, r.name
        blk += n
        dsts.append(g)
    assert ctypes.sizeof(N._PackItem) == 48
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(DEV)
    rc = h.mcav_pack_weights_multi(P(table), len(recs), blk, L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return dsts


def single(filters, r):
    """the same copy through the single-filter entry points, as ConvSpec derives it on first use -> destination window"""
    from mcav import lib as L
    h, w, s = L.lib(), filters.dev[r.f], L.stream()
    g = r.window()
    if r.kind == "um":
        rc = h.mcav_pack_weights_upmerge(P(w), r.Cout, r.Cin, r.C1, P(g), r.Np, s)
    elif r.kind == "ua":
        rc = h.mcav_pack_weights_upmerge_adj(P(w), r.Cout, r.Cin, r.C1, P(g), r.Np, r.Kp, s)
    else:
        f32 = g if not r.h else Guarded((r.shape[0] * r.shape[1],), band=256)
        rc = h.mcav_pack_weights(P(w), r.Cout, r.Cin, r.k, r.k, int(r.base == "b"), P(f32), r.Np, r.Kp, s)
        if r.h:
            conv = h.mcav_f32_to_bf16_planes if r.h == 3 else h.mcav_f32_to_bf16
            rc = rc or conv(P(f32), P(g), f32.t.numel(), s)
            torch.cuda.synchronize()
            assert f32.intact()
    torch.cuda.synchronize()
    assert rc == 0, r.name
    return g


def test_record_table_covers_the_paths_it_names():
    from mcav import lib as L
    h = L.lib()
    recs = records()
    assert {r.kind for r in recs} == {"f", "b", "f16", "b16", "f16s", "b16s", "um", "ua"}
    assert any(r.base == "f" and r.Cin * r.taps > 5120 for r in recs) and any(r.base == "f" and r.shape[1] > r.taps * r.Kp for r in recs)
    # transposed copies: ceil(Np / tile) x ceil(Kp / 64) workgroups with tiles of 79 // taps input channels, between 1 and 8
    tiles = {}
    for r in recs:
        if r.base == "b":
            ct = min(8, max(1, 79 // r.taps))
            tiles[r.taps] = ct
            assert blocks_of(h, r) == -(-r.Np // ct) * -(-r.Kp // 64), r.name
        elif r.base == "f":
            assert blocks_of(h, r) == r.Np, r.name
        else:
            assert blocks_of(h, r) == -(-r.shape[0] * r.shape[1] // 2048), r.name
    assert tiles == {9: 8, 49: 1, 25: 3, 1: 8}
    assert any(r.base == "b" and r.Np % tiles[r.taps] for r in recs), "no ragged last tile"
    assert any(r.kind == "um" and (r.shape[0] * r.shape[1]) % 2048 for r in recs)


@pytest.mark.parametrize("order", ["as listed", "reversed"])
def test_multi_launch_writes_every_kind_bit_exactly(filters, order):
    recs = records() if order == "as listed" else records()[::-1]
    dsts = multi(filters, recs)
    for r, g in zip(recs, dsts):
        assert g.intact(), "%s: wrote outside its destination" % r.name
        left = int(is_sentinel(g.cpu()).sum())
        assert left == 0, "%s: %d words of the destination were never written" % (r.name, left)
        got, want = r.read(g), filters.wanted(r)
        assert bits_equal(got, want), "%s (%s): %s" % (r.name, order, where(got, want))


def test_multi_launch_equals_the_single_filter_entry_points(filters):
    recs = records()
    dsts = multi(filters, recs)
    for r, g in zip(recs, dsts):
        one = single(filters, r)
        assert one.intact() and int(is_sentinel(one.cpu()).sum()) == 0, r.name
        assert bits_equal(r.read(g), r.read(one)), "%s: %s" % (r.name, where(r.read(g), r.read(one)))


SPEC_REF = {
    "f": lambda s, w: R.pack_forward(w, s.np, s.kp), "b": lambda s, w: R.pack_transposed(w),
    "f16": lambda s, w: R.to_bf16(R.pack_forward(w, s.np, s.kp)), "b16": lambda s, w: R.to_bf16(R.pack_transposed(w)),
    "f16s": lambda s, w: R.planes(R.pack_forward(w, s.np, s.kp)), "b16s": lambda s, w: R.planes(R.pack_transposed(w)),
    "um": lambda s, w: R.pack_upmerge(w, s._merge_c1, s.np),
    "ua": lambda s, w: R.pack_upmerge_adj(w, s._merge_c1, R.up16(s._merge_c1), R.up16(s.cout)),
}


def check_specs(specs, what):
    torch.cuda.synchronize()
    for name, s in specs.items():
        w = s.weight.detach().cpu()
        for kind, buf in s._packs.items():
            got, want = buf.detach().cpu(), SPEC_REF[kind](s, w)
            got = got.view(want.shape)
            assert bits_equal(got, want), "%s, %s of %s: %s" % (what, kind, name, where(got, want))
            assert s._keys[kind] == s._key(), "%s, %s of %s: the copy's key is stale" % (what, kind, name)


def test_registry_repacks_every_copy_of_every_spec_in_one_launch():
    from mcav import nn as N
    g = torch.Generator().manual_seed(32)

    def spec(cout, cin, k, stride, pad, pm, smallc=False):
        return N.ConvSpec(torch.nn.Parameter(torch.randn(cout, cin, k, k, generator=g).to(DEV)), None, stride, pad, pm, smallc)

    saved, N.PACKS = N.PACKS, N.PackRegistry()               # a registry of this test's own: other modules' live specs stay out of its table
    try:
        specs = {"trunk 64->64": spec(64, 64, 3, 1, 1, N.PAD_ZERO), "decoder 96->32": spec(32, 96, 3, 1, 1, N.PAD_REFLECT),
                 "stem 64<-3": spec(64, 3, 7, 2, 3, N.PAD_ZERO, smallc=True)}
        a, b, c = specs.values()
        a.packed_fwd(), a.packed_bwd(), a.packed_fwd16(), a.packed_bwd16s()
        b.packed_fwd(), b.packed_bwd(), b.packed_upmerge(32), b.packed_upmerge_adj(32)
        c.packed_fwd(), c.packed_fwd16s(), c.packed_bwd16()
        kinds = {n: sorted(s._packs) for n, s in specs.items()}
        assert kinds == {"trunk 64->64": ["b", "b16s", "f", "f16"], "decoder 96->32": ["b", "f", "ua", "um"], "stem 64<-3": ["b16", "f", "f16s"]}
        assert len(N.PACKS.entries) == 11 and N.PACKS.table is None
        check_specs(specs, "first use")                     # (the single-filter entry points)

        def change():
            with torch.no_grad():
                for s in specs.values():
                    s.weight.mul_(-1.5).add_(torch.randn(s.weight.shape, generator=g).to(DEV))
        change()
        assert all(s._keys[k] != s._key() for s in specs.values() for k in s._packs)
        b.packed_fwd()                                       # ONE copy of ONE spec is asked for ...
        check_specs(specs, "after the first repack")         # ... and every registered copy of every spec is fresh
        table = N.PACKS.table
        assert table is not None and table.numel() == 11 * 48
        change()
        a.packed_bwd16s()
        assert N.PACKS.table is table, "the table was rebuilt although nothing was added or removed"
        check_specs(specs, "after the second repack")
        # one spec goes away: the table is rebuilt without its records and the survivors are right
        del specs["stem 64<-3"], c
        gc.collect()
        change()
        b.packed_upmerge(32)
        assert N.PACKS.table is not table and N.PACKS.table.numel() == 8 * 48 and len(N.PACKS.entries) == 8
        check_specs(specs, "after a spec was deleted")
    finally:
        N.PACKS = saved
