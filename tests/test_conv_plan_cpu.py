"""No GPU: the convolution dispatch is planned in one place (csrc/conv_plan.h) and every entry answers from that plan.

Over the descriptor sweep of tests/conv_plan_cases.py (no tensors: the planner entries never dereference a pointer):
  * the library reproduces what the commit before the planner answered (tests/golden/conv_plan_parent.npz: mcav_igemm_mtiles,
    mcav_igemm_uses_bf16, mcav_wgrad_workspace_bytes, mcav_wgrad_uses_bf16), so no descriptor changed its route's observable plan;
  * the route queries agree with the older queries, and the bf16 tests agree with the route's family -- also on the copies of a descriptor
    whose stats / groups / w_stem are not settled yet, which is how the host package asks before it chooses the filter copy;
  * conv_plan.h compiles under plain g++ and, without the library around it, gives the library's answers; the same source as a program of
    its own under the address and undefined-behaviour sanitizers also survives degenerate descriptors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import conv_plan_cases as K
from conftest import PKG, REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "conv_plan_parent.npz")
SRC = os.path.join(REPO, "tests", "conv_plan_hostcheck", "conv_plan_hostcheck.cpp")
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc")]
E_INVALID = -1
IGEMM_FAMILIES, WGRAD_FAMILIES = range(8), range(5)


class Sweep:
    """The sweep and the library's answers, computed once for the module."""

    def __init__(self):
        from mcav import lib as L
        from mcav import nn as N
        self.N, self.h = N, L.lib()
        self.ig_names, self.ig = K.igemm_sweep(N)
        self.wg_names, self.wg = K.wgrad_sweep(N)
        h, ref = self.h, ctypes.byref
        self.ig_route, _ = self.routes(self.ig, h.mcav_igemm_route)
        self.wg_route, self.wg_ws = self.routes(self.wg, h.mcav_wgrad_route)
        self.ig_mtiles = np.array([h.mcav_igemm_mtiles(ref(d)) for d in self.ig], np.int32)
        self.ig_bf16 = np.array([h.mcav_igemm_uses_bf16(ref(d)) for d in self.ig], np.int8)
        self.wg_bytes = np.array([h.mcav_wgrad_workspace_bytes(ref(d)) for d in self.wg], np.int64)
        self.wg_bf16 = np.array([h.mcav_wgrad_uses_bf16(ref(d)) for d in self.wg], np.int8)

    def routes(self, descs, query):
        """-> ([n][9] = rc, family, variant, tile, mtiles, ntiles, workgroups, splits, 0 ; zeros behind a refusal), workspace bytes"""
        out, ws = np.zeros((len(descs), 9), np.int32), np.zeros(len(descs), np.int64)
        for i, d in enumerate(descs):
            r = self.N.ConvRoute()
            rc = query(ctypes.byref(d), ctypes.byref(r))
            out[i, 0] = rc
            if rc == 0:
                out[i, 1:8] = (r.family, r.variant, r.tile, r.mtiles, r.ntiles, r.workgroups, r.splits)
                ws[i] = r.workspace_bytes
            else:
                assert (r.family, r.variant, r.tile, r.mtiles, r.ntiles, r.workgroups, r.splits, r.workspace_bytes) == (0,) * 8
        return out, ws


@pytest.fixture(scope="module")
def sweep():
    return Sweep()


def test_sweep_covers_every_family_and_refusals(sweep):
    assert len(sweep.ig) >= 2000 and len(sweep.wg) >= 1000
    ig_ok, wg_ok = sweep.ig_route[:, 0] == 0, sweep.wg_route[:, 0] == 0
    ig_fam = np.bincount(sweep.ig_route[ig_ok, 1], minlength=len(IGEMM_FAMILIES))
    wg_fam = np.bincount(sweep.wg_route[wg_ok, 1], minlength=len(WGRAD_FAMILIES))
    print("igemm: %d cases, %d refused, per family %s" % (len(sweep.ig), int((~ig_ok).sum()), ig_fam.tolist()))
    print("wgrad: %d cases, %d refused, per family %s" % (len(sweep.wg), int((~wg_ok).sum()), wg_fam.tolist()))
    assert len(ig_fam) == len(IGEMM_FAMILIES) and len(wg_fam) == len(WGRAD_FAMILIES)
    assert ig_fam.min() >= 8, ig_fam
    assert wg_fam.min() >= 8, wg_fam
    assert (~ig_ok).sum() >= 50 and (~wg_ok).sum() >= 50
    assert set(np.unique(sweep.ig_route[~ig_ok, 0])) == {E_INVALID} and set(np.unique(sweep.wg_route[~wg_ok, 0])) == {E_INVALID}


def _first_difference(names, got, want):
    bad = np.flatnonzero(got != want)
    return "%d differ, first: %s (%s, recorded %s)" % (len(bad), names[bad[0]], got[bad[0]], want[bad[0]]) if len(bad) else ""


def test_library_reproduces_the_recorded_answers(sweep):
    g = np.load(GOLDEN)
    assert len(g["igemm_mtiles"]) == len(sweep.ig) and len(g["wgrad_workspace_bytes"]) == len(sweep.wg), "the sweep changed: record the golden again"
    for name, got, names in (("igemm_mtiles", sweep.ig_mtiles, sweep.ig_names), ("igemm_uses_bf16", sweep.ig_bf16, sweep.ig_names),
                             ("wgrad_workspace_bytes", sweep.wg_bytes, sweep.wg_names), ("wgrad_uses_bf16", sweep.wg_bf16, sweep.wg_names)):
        assert g[name].dtype.kind == "i"
        assert not _first_difference(names, got, g[name]), name + ": " + _first_difference(names, got, g[name])


def test_route_queries_agree_with_the_older_queries(sweep):
    ok = sweep.ig_route[:, 0] == 0
    assert (sweep.ig_mtiles[~ok] == E_INVALID).all()
    assert not _first_difference(sweep.ig_names, np.where(ok, sweep.ig_route[:, 4], E_INVALID), sweep.ig_mtiles)
    assert (sweep.ig_mtiles[ok] > 0).all() and (sweep.ig_route[ok, 5] > 0).all() and (sweep.ig_route[ok, 6] > 0).all()
    ok = sweep.wg_route[:, 0] == 0
    assert ((sweep.wg_bytes > 0) == ok).all()
    assert not _first_difference(sweep.wg_names, sweep.wg_ws, sweep.wg_bytes)
    assert (sweep.wg_route[ok, 7] > 0).all() and (sweep.wg_route[ok, 6] > 0).all()


def test_uses_bf16_is_the_route_family(sweep):
    N = sweep.N
    bf16 = (N.IGEMM_BF16_PATCH3, N.IGEMM_BF16_PATCH2, N.IGEMM_BF16_PATCH, N.IGEMM_BF16_TILE)
    ok = sweep.ig_route[:, 0] == 0
    assert not _first_difference(sweep.ig_names, np.isin(sweep.ig_route[:, 1], bf16) & ok, sweep.ig_bf16[:] * ok == 1)
    ok = sweep.wg_route[:, 0] == 0
    assert not _first_difference(sweep.wg_names, np.isin(sweep.wg_route[:, 1], (N.WGRAD_BF16_PATCH, N.WGRAD_BF16_TILE)) & ok, sweep.wg_bf16 == 1)


def test_uses_bf16_is_the_route_family_before_the_descriptor_is_settled(sweep):
    """mcav.nn._weights_for asks mcav_igemm_uses_bf16 before stats, groups and w_stem are final and then hands the bf16 filter over in d.w: on
    every such copy that the planner accepts, 'uses bf16' must be exactly 'a bf16 family runs it' (an fp32 kernel would read bf16 bytes)."""
    N, h = sweep.N, sweep.h
    bf16 = (N.IGEMM_BF16_PATCH3, N.IGEMM_BF16_PATCH2, N.IGEMM_BF16_PATCH, N.IGEMM_BF16_TILE)
    checked = 0
    for name, d in zip(sweep.ig_names, sweep.ig):
        if not d.mma:
            continue
        for c in K.unsettled_copies(d):
            r = N.ConvRoute()
            if h.mcav_igemm_route(ctypes.byref(c), ctypes.byref(r)) == 0:
                assert (r.family in bf16) == bool(h.mcav_igemm_uses_bf16(ctypes.byref(c))), (name, bool(c.stats), c.groups, bool(c.w_stem), r.family)
                checked += 1
    assert checked >= 8 * 1000


def _host_answers(lib, descs, fn):
    out, ws = np.zeros((len(descs), 9), np.int32), np.zeros(len(descs), np.int64)
    getattr(lib, fn)(K.as_array(descs), len(descs), out.ctypes.data_as(ctypes.c_void_p), ws.ctypes.data_as(ctypes.c_void_p))
    return out, ws


def test_header_under_plain_gxx_gives_the_library_answers(sweep, tmp_path):
    so = str(tmp_path / "libconv_plan_hostcheck.so")
    subprocess.check_call(GXX + ["-shared", "-fPIC", SRC, "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.conv_plan_hostcheck_sizes(0) == ctypes.sizeof(sweep.N.IgemmDesc) and lib.conv_plan_hostcheck_sizes(1) == ctypes.sizeof(sweep.N.WgradDesc)
    out, _ = _host_answers(lib, sweep.ig, "conv_plan_hostcheck_igemm")
    assert not _first_difference(sweep.ig_names, (out[:, :8] != sweep.ig_route[:, :8]).any(axis=1), np.zeros(len(sweep.ig), bool))
    assert not _first_difference(sweep.ig_names, out[:, 8], sweep.ig_bf16)
    out, ws = _host_answers(lib, sweep.wg, "conv_plan_hostcheck_wgrad")
    assert not _first_difference(sweep.wg_names, (out[:, :8] != sweep.wg_route[:, :8]).any(axis=1), np.zeros(len(sweep.wg), bool))
    assert not _first_difference(sweep.wg_names, out[:, 8], sweep.wg_bf16)
    assert not _first_difference(sweep.wg_names, ws, sweep.wg_bytes)


def test_stand_alone_program_under_the_sanitizers(sweep, tmp_path):
    """The same source with its own main(), built with -fsanitize=address,undefined and run as a program of its own over the sweep (it checks
    the library's answers, read from a file) and over degenerate descriptors: zeros, negative sizes, INT_MAX sizes, filters of up to 64 taps."""
    exe, data = str(tmp_path / "conv_plan_hostcheck_san"), str(tmp_path / "sweep.bin")
    cmd = GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCONV_PLAN_HOSTCHECK_MAIN", SRC, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("g++ has no sanitizer runtime here")
    assert build.returncode == 0, build.stderr
    with open(data, "wb") as f:
        for descs, route, ws, bf16 in ((sweep.ig, sweep.ig_route, np.zeros(len(sweep.ig), np.int64), sweep.ig_bf16),
                                       (sweep.wg, sweep.wg_route, sweep.wg_bytes, sweep.wg_bf16)):
            want = route.copy()
            want[:, 8] = bf16
            f.write(np.int32(len(descs)).tobytes())
            f.write(bytes(K.as_array(descs)))
            f.write(want.tobytes())
            f.write(ws.tobytes())
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0 and "conv_plan_hostcheck: ok" in run.stdout, (run.stdout, run.stderr)
