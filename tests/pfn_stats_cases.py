"""TEST INFRASTRUCTURE: the cases of the voxels' moments, their adjoint and the batch-statistics layer, shared by the CPU tests
(tests/test_pfn_stats_cpu.py) and the GPU tests (tests/test_pfn_stats_gpu.py).  Every case of tests/pfn_cases.py (N = 1, 5, 32 and 64,
C = 4 and 9, up to P = 3 985 at KITTI coordinate magnitudes, where mean^2 is largest against var) plus planted ones:

    no-pillars      capacity 6, B = 2, offsets all zero, the buffers full of NaNs: rows = 0, the running statistics are folded
    one-point       one pillar with one point under N = 1: rows = 1, the same fallback
    cut             wide-o128 under pfn_cases.cut_capacity: the capacity ends inside image 1 (NaN rows among the live ones)
    cut-finite      fullrow-o32 under the same cut: finite, for the layer
    clipped         mixed-N5-c9-o64 with num_points above N (the pillars that were full) and below 0 (the first partly filled ones)
    special-o32     as it is: NaN and infinities in used slots go in, NaN statistics come out
nan_filled(a, capacity): a copy whose unused slots and rows at and beyond P hold NaNs: the same bytes as the clean case must come out.
A case: dict(voxels [capacity, N, C], num_points, coords, offsets, nx, ny, capacity, weight [C_out, C]); references are computed once."""
import functools

import numpy as np

import pfn_cases as C
import pfn_ref as R
import pfn_stats_ref as SR

F = np.float32
PFN = C.CASES + [C.REAL_CASE]
PLANTED = ["no-pillars", "one-point", "cut", "cut-finite", "clipped"]
ALL = PFN + PLANTED
FALLBACK = ["no-pillars", "one-point"]                       # rows < 2
SLACK = 5                                                    # rows of the buffers behind the pillars


@functools.lru_cache(maxsize=None)
def build(name):
    if name in PFN:
        a = dict(C.build(name))
        a["capacity"] = len(a["voxels"]) + SLACK
    elif name == "no-pillars":
        w, _ = C.layer(32, 4, 77)
        a = dict(voxels=np.full((6, 3, 4), np.nan, F), coords=np.zeros((6, 4), np.int32), num_points=np.full(6, 2, np.int32),
                 offsets=np.zeros(3, np.int32), nx=7, ny=9, capacity=6, weight=w)
    elif name == "one-point":
        w, _ = C.layer(32, 4, 78)
        a = dict(voxels=np.array([[[1.5, -2.25, 0.5, 0.75]]], F), coords=np.array([[0, 0, 4, 2]], np.int32), num_points=np.ones(1, np.int32),
                 offsets=np.array([0, 1], np.int32), nx=7, ny=9, capacity=1, weight=w)
    elif name == "cut":
        a = dict(C.build("wide-o128"))
        a["capacity"] = C.cut_capacity("wide-o128")
    elif name == "cut-finite":
        a = dict(C.build("fullrow-o32"))
        a["capacity"] = C.cut_capacity("fullrow-o32")
    elif name == "clipped":
        a = dict(C.build("mixed-N5-c9-o64"))
        num, N = a["num_points"].copy(), a["voxels"].shape[1]
        full, partly = np.flatnonzero(num == N), np.flatnonzero(num < N)
        assert len(full) >= 2 and len(partly) >= 3
        num[full[:2]] = [N + 1000, 2 ** 31 - 1]
        num[partly[:2]] = [-3, -2 ** 31]
        a["num_points"], a["capacity"] = num, len(num) + SLACK
    else:
        raise KeyError(name)
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


def padded(a, fill):
    """-> voxels, coords, num_points of a["capacity"] rows: the case's rows below the capacity, `fill` (and counts of 1 << 20) behind"""
    cap, (_, N, Cc) = a["capacity"], a["voxels"].shape
    k = min(cap, len(a["voxels"]))
    vox, coords, num = np.full((cap, N, Cc), fill, F), np.full((cap, 4), 1 << 20, np.int32), np.full(cap, 1 << 20, np.int32)
    vox[:k], coords[:k], num[:k] = a["voxels"][:k], a["coords"][:k], a["num_points"][:k]
    return vox, coords, num


def nan_filled(a):
    """-> voxels [capacity, N, C] with NaNs in every slot the definition does not read"""
    vox, _, num = padded(a, np.nan)
    P = R.live_pillars(a["offsets"], a["capacity"])
    used, _ = SR.used_mask(num, P, vox.shape[1])
    vox[:P][~used] = np.nan
    return vox


@functools.lru_cache(maxsize=None)
def moments(name):
    a = build(name)
    out = SR.moments(a["voxels"], a["num_points"], a["offsets"], a["capacity"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def gradient(name, seed=0):
    """a seeded upstream gradient of the moments: float64 [2 + C + C C], H not symmetric"""
    Cc = build(name)["voxels"].shape[2]
    return np.random.RandomState(500 + seed + len(name)).standard_normal(SR.size(Cc))


@functools.lru_cache(maxsize=None)
def backward(name, seed=0):
    a = build(name)
    Cc = a["voxels"].shape[2]
    g = gradient(name, seed)
    return SR.moments_backward(a["voxels"], a["num_points"], a["offsets"], g[2:2 + Cc], g[2 + Cc:], a["capacity"])


def norm_parameters(c_out, seed):
    """gamma = |randn| + 0.5, beta = 0.3 randn, running_mean, running_var: float64 numpy"""
    rng = np.random.RandomState(seed)
    return np.abs(rng.randn(c_out)) + 0.5, 0.3 * rng.randn(c_out), 0.2 * rng.randn(c_out), rng.rand(c_out) + 0.1


def check_non_trivial():
    assert moments("no-pillars")["moments"][0] == 0 and moments("one-point")["moments"][0] == 1
    a = build("cut")
    assert int(a["offsets"][1]) < a["capacity"] < int(a["offsets"][2])
    c, m = build("clipped"), build("mixed-N5-c9-o64")
    assert (c["num_points"] > 5).sum() == 2 and (c["num_points"] < 0).sum() == 2
    assert moments("clipped")["moments"][1] < moments("mixed-N5-c9-o64")["moments"][1]      # the negative counts' points are gone
    assert np.isnan(moments("special-o32")["moments"][2:]).any() and np.isfinite(moments("special-o32")["moments"][:2]).all()
    assert {build(n)["voxels"].shape[1] for n in PFN} >= {1, 5, 32, 64} and {build(n)["voxels"].shape[2] for n in PFN} == {4, 9}
