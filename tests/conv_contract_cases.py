"""Descriptors the planners of mcav_igemm / mcav_wgrad must refuse (include/mcav_conv.h), shared by tests/test_conv_contract_cpu.py (planner
entries only: they launch nothing and need no device memory) and tests/test_conv_contract_gpu.py (the launch entries, after the planner has
refused).  Every case starts from a descriptor the planner accepts and changes the named fields only."""
E_INVALID = -1


def igemm_base(N, x, w, y):
    """A 64 -> 64 3x3 stride-1 zero-padded convolution at 1 x 8 x 8 on the fp32 kernels; x, w, y: device addresses (never dereferenced by the planner)."""
    d = N.IgemmDesc()
    d.x1, d.B, d.Hs, d.Ws, d.C1 = x, 1, 8, 8, 64
    d.w, d.kh, d.kw, d.Np, d.Kp = w, 3, 3, 64, 64
    d.mode, d.stride, d.sign, d.offset, d.pad_mode = N.G_DIRECT, 1, 1, -1, N.PAD_ZERO
    d.y, d.Hd, d.Wd, d.Cd, d.n_begin, d.n_count, d.y_choff = y, 8, 8, 64, 0, 64, 0
    d.groups = 1
    return d


def _set(**kw):
    def change(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return change


BIG = dict(Hs=512, Ws=512, Hd=512, Wd=512)          # source 512 x 512 x 64 floats = 64 MiB: inside the planner's source bound

# name -> change: each makes the descriptor one mcav_igemm_mtiles must answer with MCAV_E_INVALID
IGEMM_REFUSED = {
    "Cd zero": _set(Cd=0),
    "Cd negative": _set(Cd=-64),
    "Cd below n_count": _set(Cd=48),
    "y_choff negative": _set(Cd=128, y_choff=-16),
    "y_choff + n_count past Cd": _set(Cd=64, y_choff=16),
    "y_choff + n_count past a wider Cd": _set(Cd=96, n_count=32, y_choff=80),
    "y_choff overflows with n_count": _set(Cd=96, n_count=32, y_choff=0x7fffffff),
    "output of 2 GiB": _set(Cd=2048, **BIG),                                     # 512 * 512 * 2048 * 4 bytes = 2^31
    "output of 2 GiB through the batch": _set(B=32, Hs=64, Ws=64, Hd=2048, Wd=128, Cd=64, stride=1),      # 32 * 2048 * 128 * 64 * 4 = 2^31, source 32 MiB
    "pooled output of 2 GiB": _set(Cd=8192, pool=1, mode=2, sign=-1, offset=1, **BIG),                     # (512 / 2)^2 * 8192 * 4 = 2^31
}
# ... and their neighbours the planner must keep accepting (mtiles > 0)
IGEMM_ACCEPTED = {
    "the base": _set(),
    "a sub-range at the end of a wider pixel": _set(Cd=96, n_count=32, n_begin=32, y_choff=64),
    "output just below 2 GiB": _set(Cd=2044, **BIG),
    "pooled: the pooled size counts": _set(Cd=2048, pool=1, mode=2, sign=-1, offset=1, **BIG),             # un-pooled it would be 2 GiB
}


def wgrad_base(N, x, dy, dw):
    """The weight gradient of a 64 -> 64 3x3 stride-1 zero-padded convolution at 1 x 8 x 8."""
    d = N.WgradDesc()
    d.x1, d.B, d.Hs, d.Ws, d.C1 = x, 1, 8, 8, 64
    d.kh, d.kw, d.Kp = 3, 3, 64
    d.mode, d.stride, d.sign, d.offset, d.pad_mode = N.G_DIRECT, 1, 1, -1, N.PAD_ZERO
    d.dy, d.Hd, d.Wd, d.Cdy, d.dy_choff = dy, 8, 8, 64, 0
    d.Cout, d.Cin = 64, 64
    d.dw_oihw, d.accumulate = dw, 1
    return d


# name -> change: each makes the descriptor one mcav_wgrad_workspace_bytes must answer with 0
WGRAD_REFUSED = {
    "dy_choff negative": _set(Cdy=128, dy_choff=-4),
    "dy_choff + Cout past Cdy": _set(dy_choff=4),
    "dy_choff + Cout past a wider Cdy": _set(Cdy=96, dy_choff=36),
    "Cdy zero": _set(Cdy=0),
    "Cdy below Cout": _set(Cdy=32),
    "kh zero": _set(kh=0),
    "kw negative": _set(kw=-3),
    "ci_offset negative": _set(Cin_total=96, ci_offset=-1),
    "ci_offset + Cin past Cin_total": _set(Cin_total=96, ci_offset=48),
    "ci_offset without Cin_total": _set(ci_offset=16),
    "dy_choff + Cout past Cdy on the bf16 planner": _set(mma=1, dy_choff=4),
    "ci_offset + Cin past Cin_total on the split planner": _set(mma=2, Cin_total=96, ci_offset=48),
}
WGRAD_ACCEPTED = {
    "the base": _set(),
    "channels at the end of a wider dy": _set(Cdy=96, dy_choff=32),
    "the last input-channel window": _set(Cin_total=96, ci_offset=32),
}
