"""No GPU: the planner entries of the convolution ABI (mcav_igemm_mtiles, mcav_wgrad_workspace_bytes) refuse descriptors whose destination or
gradient window the kernels could not honour (include/mcav_conv.h: Cd / y_choff, the 2 GiB bound of the 32-bit output offsets, Cdy / dy_choff,
kh / kw, Cin_total / ci_offset) -- and keep accepting their neighbours.  Both entries only plan: they launch nothing and never dereference the
descriptor's pointers, so dummy non-null addresses stand in for device memory here; tests/test_conv_contract_gpu.py repeats every refusal
through the launch entries."""
import ctypes

import pytest

import conv_contract_cases as K

DUMMY = 0x10000          # a non-null address the planners only compare with NULL


def lib_and_nn():
    from mcav import lib as L
    from mcav import nn as N
    return L.lib(), N


@pytest.mark.parametrize("name", list(K.IGEMM_REFUSED))
def test_igemm_planner_refuses(name):
    h, N = lib_and_nn()
    d = K.igemm_base(N, DUMMY, DUMMY, DUMMY)
    assert h.mcav_igemm_mtiles(ctypes.byref(d)) > 0
    K.IGEMM_REFUSED[name](d)
    assert h.mcav_igemm_mtiles(ctypes.byref(d)) == K.E_INVALID


@pytest.mark.parametrize("name", list(K.IGEMM_ACCEPTED))
def test_igemm_planner_accepts(name):
    h, N = lib_and_nn()
    d = K.igemm_base(N, DUMMY, DUMMY, DUMMY)
    K.IGEMM_ACCEPTED[name](d)
    assert h.mcav_igemm_mtiles(ctypes.byref(d)) > 0


@pytest.mark.parametrize("name", list(K.WGRAD_REFUSED))
def test_wgrad_planner_refuses(name):
    h, N = lib_and_nn()
    d = K.wgrad_base(N, DUMMY, DUMMY, DUMMY)
    assert h.mcav_wgrad_workspace_bytes(ctypes.byref(d)) > 0
    K.WGRAD_REFUSED[name](d)
    assert h.mcav_wgrad_workspace_bytes(ctypes.byref(d)) == 0
    assert h.mcav_wgrad_uses_bf16(ctypes.byref(d)) == 0


@pytest.mark.parametrize("name", list(K.WGRAD_ACCEPTED))
def test_wgrad_planner_accepts(name):
    h, N = lib_and_nn()
    d = K.wgrad_base(N, DUMMY, DUMMY, DUMMY)
    K.WGRAD_ACCEPTED[name](d)
    assert h.mcav_wgrad_workspace_bytes(ctypes.byref(d)) > 0
