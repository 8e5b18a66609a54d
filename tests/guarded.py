"""Output windows with sentinel bands, shared by the GPU test modules (a helper module, not a conftest).

Every buffer a kernel WRITES is a window of a larger allocation.  The bands before and after the window hold a sentinel bit pattern (a NaN), so
a store one row or one column outside the output shows as a changed band instead of landing in the caching allocator's neighbouring block; the
window itself starts as sentinels too, so an element a kernel skipped (a raw-buffer store that was wrongly masked is dropped in hardware) fails
the comparison as NaN instead of showing the previous launch's answer.

  Guarded            one window, built by the test (tests/test_nn_ops_gpu.py, tests/test_conv_contract_gpu.py)
  guard_allocations  every mcav.nn.empty() of the product inside the `with` becomes such a window; check() asserts all bands
  guarded_grad       param.grad as such a window: mcav.nn.grad_buffer hands it to mcav_wgrad as dw_oihw / dbias
"""
import numpy as np
import torch

DEV = "cuda"
F32 = torch.float32
GUARD = 64                       # elements on each side (256 bytes of float32: the windows stay 16-byte aligned)
SENT32 = 0x7FA5A5A5              # a NaN
SENT8 = 0xA5
ALIGN = 64                       # band widths are multiples of 64 float32 (256 bytes): a window keeps the alignment of its allocation

_ACTIVE = []                     # the guard_allocations blocks that are open, innermost last


def band_for(shape):
    """Band width in elements for an output of `shape`: at least 64 floats and two last-dimension strides, rounded up to 256 bytes."""
    last = int(shape[-1]) if len(shape) else 1
    return (max(GUARD, 2 * last) + ALIGN - 1) // ALIGN * ALIGN


def P(t):
    if isinstance(t, Guarded):
        t = t.t
    return t.data_ptr() if t is not None else None


class Guarded:
    """A float32 / uint8 output window of `shape` inside a larger allocation filled with sentinels; init: what the window starts with
    (a tensor or a number; None keeps the sentinels); band: elements on each side (GUARD when not given)."""

    def __init__(self, shape, dtype=F32, init=None, band=None, device=DEV):
        shape = tuple(int(v) for v in shape)
        n = int(np.prod(shape)) if len(shape) else 1
        self.band = GUARD if band is None else int(band)
        self.buf = torch.empty(n + 2 * self.band, dtype=dtype, device=device)
        self.sent = SENT32 if dtype == F32 else SENT8
        self.raw().fill_(self.sent)
        self.t = self.buf[self.band:self.band + n].view(shape)
        if init is not None:
            if torch.is_tensor(init):
                self.t.copy_(init)
            else:
                self.t.fill_(init)

    def raw(self):
        return self.buf.view(torch.int32) if self.buf.dtype == F32 else self.buf

    def intact(self):
        r = self.raw()
        return bool((r[:self.band] == self.sent).all()) and bool((r[-self.band:] == self.sent).all())

    def untouched(self):
        return bool((self.raw() == self.sent).all())

    def cpu(self):
        return self.t.detach().cpu()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == F32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def is_sentinel(t):
    """elementwise: the float32 element still holds the sentinel bit pattern (nothing stored it)"""
    return bits(t) == SENT32


class guard_allocations:
    """with guard_allocations() as g: ...; g.check()

    Replaces mcav.nn.empty for the duration: every activation, statistics slab, packed filter copy and intermediate the product allocates
    through it is a sentinel-filled window between two sentinel bands (band_for(shape) elements each, so the window stays 256-byte aligned:
    the kernels use 16-byte accesses and buffer resources on these pointers).  Every window is recorded -- and so kept alive, which is why
    whole-network tests stay on torch.empty.  check() waits for the device and asserts that every band still holds the sentinel."""

    def __init__(self):
        self.windows = []

    def _empty(self, shape, like):
        g = Guarded(tuple(shape), F32, band=band_for(tuple(shape)), device=like.device)
        self.windows.append(g)
        return g.t

    def add(self, g):
        self.windows.append(g)
        return g

    def __enter__(self):
        from mcav import nn
        self._nn, self._saved = nn, nn.empty
        nn.empty = self._empty
        _ACTIVE.append(self)
        return self

    def __exit__(self, *exc):
        self._nn.empty = self._saved
        _ACTIVE.remove(self)
        return False

    def check(self):
        torch.cuda.synchronize()
        for g in self.windows:
            assert g.intact(), "a kernel wrote outside an output of shape %s (band of %d elements on each side)" % (tuple(g.t.shape), g.band)


def guarded_grad(param, fill=0.0):
    """param.grad becomes a guarded window: zero-filled (fill = 0.0, what an accumulating launch adds into), filled with another number, or
    left as sentinels (fill = None: a launch that overwrites must store every element).  The window is checked with the innermost open
    guard_allocations block, if there is one.  None for a parameter that is None (a convolution without bias)."""
    if param is None:
        return None
    g = Guarded(tuple(param.shape), F32, init=fill, band=band_for(tuple(param.shape)), device=param.device)
    param.grad = g.t
    param._guard = g
    if _ACTIVE:
        _ACTIVE[-1].add(g)
    return g


def guarded_spec(spec, fill=0.0):
    """both gradients of a ConvSpec (weight, and bias where it has one) as guarded windows -> spec"""
    guarded_grad(spec.weight, fill)
    guarded_grad(spec.bias, fill)
    return spec
