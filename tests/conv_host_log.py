"""A call log of the host layer, taken without a GPU (a helper module, not a conftest).

`recording(mode)` installs a proxy as mcav.lib._LIB.  The pure planner entries (they launch nothing and never dereference a descriptor's
pointers) go to the real library; every other entry is recorded and answered with 0, so the whole host layer -- mcav.nn, mcav.tape, the
networks' forward and backward engines -- runs on CPU tensors and leaves the list of launches it would have made, descriptors field by field.

  full mode      every distinct non-null pointer is renamed to the index of its first appearance in the case, so a log does not depend on
                 allocation addresses but still says which launch reads what another wrote.  For that no address may be used twice within
                 a case: every tensor torch allocates inside the block is kept alive until the block ends.
  sequence mode  pointers are reduced to null / non-null (whole networks, where holding every activation would defeat the allocator).

With profile=True mcav.nn.PROFILE is a list inside the block and its records and tags are kept with the log (profile_line)."""
import contextlib
import ctypes
import hashlib

import torch

FORWARDED = {"mcav_abi_version", "mcav_igemm_mtiles", "mcav_igemm_uses_bf16", "mcav_wgrad_uses_bf16", "mcav_wgrad_workspace_bytes",
             "mcav_igemm_route", "mcav_wgrad_route", "mcav_wgrad_reduce_plan", "mcav_pack_weights_blocks"}
TIMED = {"mcav_igemm", "mcav_wgrad", "mcav_wgrad_deferred"}
INTS = (ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_ulonglong)
FLOATS = (ctypes.c_float, ctypes.c_double)
ALLOCATORS = ("empty", "zeros", "empty_like", "zeros_like")


def forwarded(name):
    return name in FORWARDED or name.endswith("_workspace_bytes")


class CallLog:
    def __init__(self, real, signatures, mode):
        assert mode in ("full", "sequence")
        self.real, self.signatures, self.mode = real, signatures, mode
        self.lines, self.names, self.timed, self.held = [], {}, 0, []
        self.profile = []                                # (ProfileRec, tag) of the block, when it ran with mcav.nn.PROFILE a list

    def pointer(self, v):
        if isinstance(v, ctypes.c_void_p):
            v = v.value
        if not v:
            return "0"
        if self.mode == "sequence":
            return "p"
        return "p%d" % self.names.setdefault(int(v), len(self.names))

    def struct(self, s):
        out = []
        for name, typ in s._fields_:
            v = getattr(s, name)
            if typ in INTS:
                out.append("%s=%d" % (name, v))
            elif typ in FLOATS:
                out.append("%s=%s" % (name, float(v).hex()))
            elif typ is ctypes.c_void_p:
                out.append("%s=%s" % (name, self.pointer(v)))
            else:                                        # an array of pointers (x_planar)
                out.append("%s=[%s]" % (name, ",".join(self.pointer(e) for e in v)))
        return "%s{%s}" % (type(s).__name__, " ".join(out))

    def argument(self, typ, v):
        if typ in INTS:
            return "%d" % int(v)
        if typ in FLOATS:
            return float(v).hex()
        if v is None or isinstance(v, (int, ctypes.c_void_p)):
            return self.pointer(v)
        obj = getattr(v, "_obj", v)                      # ctypes.byref(x)
        if type(obj).__name__ in ("IgemmDesc", "WgradDesc"):
            return self.struct(obj)
        return "&" + type(obj).__name__                  # an out-parameter or a host-side table

    def record(self, name, args):
        types = self.signatures[name][1]
        assert len(types) == len(args), name
        self.lines.append("%s(%s)" % (name, ", ".join(self.argument(t, a) for t, a in zip(types, args))))
        self.timed += name in TIMED
        return 0

    def note(self, text):
        self.lines.append(text)

    def __getattr__(self, name):
        if not name.startswith("mcav_"):
            raise AttributeError(name)
        if name == "mcav_kernel_timer_count":
            return lambda: self.timed
        if forwarded(name):
            return getattr(self.real, name)
        return lambda *args: self.record(name, args)

    def text(self):
        return "\n".join(self.lines) + "\n"


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()


def _host_dev(t, name="tensor", dtype=torch.float32):
    """mcav.lib.dev without the `is_cuda` check."""
    from mcav import lib as L
    if t.dtype != dtype:
        raise L.MCAVError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise L.MCAVError("%s must be contiguous" % name)
    return t


@contextlib.contextmanager
def recording(mode, profile=False):
    """-> the CallLog.  Inside the block the host layer runs on CPU tensors; per-process caches that would carry one case into the next
    (workspaces, whose sizes are launch arguments) start empty."""
    from mcav import lib as L
    from mcav import nn as N
    import mcav.tape  # noqa: F401  (registers its entries' signatures)
    log = CallLog(L.lib(), L._SIGNATURES, mode)
    saved = (L._LIB, L.stream, L.dev, dict(L._WS), N.PROFILE, N.PROFILE_TAGS)
    allocs = {n: getattr(torch, n) for n in ALLOCATORS}

    def holding(fn):
        def alloc(*a, **kw):
            t = fn(*a, **kw)
            log.held.append(t)
            return t
        return alloc
    L._LIB, L.stream, L.dev = log, (lambda: ctypes.c_void_p(0)), _host_dev
    L._WS.clear()
    N.PROFILE, N.PROFILE_TAGS = ([], []) if profile else (None, None)
    if mode == "full":
        for n, fn in allocs.items():
            setattr(torch, n, holding(fn))
    try:
        yield log
        if profile:
            assert len(N.PROFILE) == len(N.PROFILE_TAGS)
            log.profile = list(zip(N.PROFILE, N.PROFILE_TAGS))
    finally:
        for n, fn in allocs.items():
            setattr(torch, n, fn)
        L._LIB, L.stream, L.dev = saved[:3]
        L._WS.clear()
        L._WS.update(saved[3])
        N.PROFILE, N.PROFILE_TAGS = saved[4:]
        N.flush_bn_counters()


def profile_line(rec, tag, executed=None):
    """One ProfileRec as a log line; executed: what stands in its place (the comparison of a corrected record leaves the figure out)."""
    executed = float(rec.executed).hex() if executed is None else executed
    return "profile kind=%s flops=%s i0=%d i1=%d executed=%s bf16_planes=%d abytes=%s tag=%r" % (
        rec.kind, float(rec.flops).hex(), rec.i0, rec.i1, executed, rec.bf16_planes, float(rec.abytes).hex(), tag)
