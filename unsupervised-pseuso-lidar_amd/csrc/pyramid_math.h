// Per-pixel arithmetic of the depth pyramid (include/mcav_depth.h: mcav_depth_pyramid_fwd / _bwd): the bilinear taps of
// F.interpolate(align_corners=False), disp_to_depth and its slope, and the adjoint's window -- which outputs touch a given source index.
// Shared by the HIP kernels (depth_pyramid.hip, aux_ops.hip's standalone resize) and by the host-compiled check in
// tests/pyramid_hostcheck (never by the product).
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MCAV_PYR_HD __host__ __device__ __forceinline__
#else
#define MCAV_PYR_HD inline
#endif

namespace mcav {
namespace pyr {

// PyTorch's bilinear source index with align_corners = False: max(0, scale * (dst + 0.5) - 0.5)
MCAV_PYR_HD void bil_src(int o, float scale, int n_in, int& i0, int& i1, float& lam) {
    float s = scale * ((float)o + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    lam = s - (float)i0;
}

// disp_to_depth (pose_geometry.py:81-82) and dD/dd at that depth
MCAV_PYR_HD float depth_of(float d) { return 1.0f / (10.0f * d + 0.01f); }
MCAV_PYR_HD float depth_slope(float D) { return -10.0f * D * D; }

// weight of source index i in output o along one axis (both taps when they coincide at the last source)
MCAV_PYR_HD float tap_weight(int o, int i, float scale, int n_in) {
    int i0, i1;
    float lam;
    bil_src(o, scale, n_in, i0, i1, lam);
    float wgt = 0.f;
    if (i0 == i) wgt += 1.f - lam;
    if (i1 == i) wgt += lam;
    return wgt;
}

// The first output whose lower tap is >= i; n_out when there is none.  The lower tap never decreases with o (every float32 operation of
// bil_src is monotone), so a bisection over bil_src itself is exact: no inverse formula whose rounding would have to be argued about.
MCAV_PYR_HD int first_output_at(int i, float scale, int n_in, int n_out) {
    int lo = 0, hi = n_out;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        int i0, i1;
        float lam;
        bil_src(mid, scale, n_in, i0, i1, lam);
        if (i0 >= i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Outputs [lo, hi] whose taps touch source i: exactly those whose lower tap is i - 1 or i.  Source 0 collects the whole leading run that
// max(0, .) clamps onto it, the last source everything up to n_out - 1.  Empty (lo > hi) only if no output reaches i.
MCAV_PYR_HD void adjoint_window(int i, float scale, int n_in, int n_out, int& lo, int& hi) {
    lo = first_output_at(i - 1, scale, n_in, n_out);
    hi = first_output_at(i + 1, scale, n_in, n_out) - 1;
}

// One output of one level.  p: the level's [h, w] disparities of this sample.  Depth-first (the reference's order, losses.py:212-216): the
// four taps become depths, then blend; resize_then_depth (monodepth2): blend the disparities, then the depth.  The blend is
// resize_bilinear_fwd_kernel's expression.
MCAV_PYR_HD float fwd_value(const float* p, int w, int y0, int y1, float ly, int x0, int x1, float lx, bool resize_then_depth) {
    float p00 = p[(size_t)y0 * w + x0], p01 = p[(size_t)y0 * w + x1], p10 = p[(size_t)y1 * w + x0], p11 = p[(size_t)y1 * w + x1];
    if (!resize_then_depth) { p00 = depth_of(p00); p01 = depth_of(p01); p10 = depth_of(p10); p11 = depth_of(p11); }
    const float top = p00 * (1.f - lx) + p01 * lx;
    const float bot = p10 * (1.f - lx) + p11 * lx;
    const float v = top * (1.f - ly) + bot * ly;
    return resize_then_depth ? depth_of(v) : v;
}

}  // namespace pyr
}  // namespace mcav
