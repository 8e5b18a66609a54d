// Per-pixel arithmetic of the KITTI depth evaluation protocol (mcav_eval_depth, include/mcav_depth.h), shared by the HIP kernels
// (eval_depth.hip) and by the host-compiled check in tests/eval_hostcheck (never by the product).  The definition is
// tests/eval_protocol_ref.py:
//   up   = disp resized to the ground truth's (Hb, Wb): bilinear, half-pixel centres, edge clamping (F.interpolate, align_corners=False)
//   pred = 1 / (10 up + 0.01) * scale, float32, every operation rounded on its own (numpy float32, no fused multiply-add)
// and the order-preserving float -> uint32 key of the exact radix-select median.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MCAV_EV_HD __host__ __device__ __forceinline__
#else
#define MCAV_EV_HD inline
#endif

namespace mcav {
namespace ev {

// Rounded float32 operations: the device spells them out, the host build is compiled with -ffp-contract=off.
MCAV_EV_HD float mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
MCAV_EV_HD float add_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
MCAV_EV_HD float fma_rn(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return fmaf(a, b, c);
#endif
}
MCAV_EV_HD float div_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

MCAV_EV_HD uint32_t float_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
#endif
}
MCAV_EV_HD float bits_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float x;
    memcpy(&x, &u, 4);
    return x;
#endif
}

// Order-preserving key: a value with the sign bit clear (x >= +0, +inf) gets its sign bit set, one with the sign bit set (x <= -0, -inf)
// has every bit inverted.  a < b => key(a) < key(b); -0 sorts directly below +0.  The sign bit decides, not x >= 0, so -0 stays between
// the negatives and +0.  NaNs land beyond +-inf; the kernels flag them separately (a median over a NaN is NaN, as in numpy).
MCAV_EV_HD uint32_t float_key(float x) {
    const uint32_t u = float_bits(x);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
MCAV_EV_HD float key_float(uint32_t k) { return bits_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// The depth of one disparity: 1 / (10 d + 0.01), times the caller's scale (pred_depth_scale_factor; 1 leaves it exact).
MCAV_EV_HD float disp_depth(float d, float scale) { return mul_rn(div_rn(1.0f, add_rn(mul_rn(10.0f, d), 0.01f)), scale); }

// Source coordinate of output index i along an axis resized from n_in to n_out (upsample_bilinear2d, align_corners=False):
// s = (i + 0.5) * (n_in / n_out) - 0.5, negative values clamped to 0.  i0 = floor(s), i1 = min(i0 + 1, n_in - 1), l = s - i0.
// The multiply-add is fused, as torch's CPU kernel compiles it: with two roundings l differs by an ulp of s, which is hundreds of ulps of
// a small result.
MCAV_EV_HD void bilinear_axis(int i, int n_in, float scale, int& i0, int& i1, float& l) {
    float s = fma_rn(scale, add_rn((float)i, 0.5f), -0.5f);
    if (s < 0.0f) s = 0.0f;
    i0 = (int)s;
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 < n_in - 1 ? i0 + 1 : i0;
    l = add_rn(s, -(float)i0);
}

// disp [h, w] (one image, row stride w) sampled at ground-truth pixel (y, x) of an Hb x Wb image; sy = h / Hb, sx = w / Wb (float32).
// (1 - ly) * ((1 - lx) v00 + lx v01) + ly * ((1 - lx) v10 + lx v11), the inner sums fused: within 1 ulp of F.interpolate on the CPU.
MCAV_EV_HD float bilinear_sample(const float* disp, int h, int w, float sy, float sx, int y, int x) {
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_axis(y, h, sy, y0, y1, ly);
    bilinear_axis(x, w, sx, x0, x1, lx);
    const float hy = add_rn(1.0f, -ly), hx = add_rn(1.0f, -lx);
    const float* r0 = disp + (size_t)y0 * w;
    const float* r1 = disp + (size_t)y1 * w;
    const float t = fma_rn(hx, r0[x0], mul_rn(lx, r0[x1]));
    const float b = fma_rn(hx, r1[x0], mul_rn(lx, r1[x1]));
    return add_rn(mul_rn(hy, t), mul_rn(ly, b));
}

// The resize factor of one axis: n_in / n_out in float32 (area_pixel_compute_scale without a given scale factor)
MCAV_EV_HD float axis_scale(int n_in, int n_out) { return div_rn((float)n_in, (float)n_out); }

// np.median of float32 from the two middle order statistics: odd counts take the middle one, even counts the float32 mean of the two.
MCAV_EV_HD float median_of(float lo, float hi, uint32_t n) { return (n & 1u) ? lo : mul_rn(add_rn(lo, hi), 0.5f); }

// np.clip(p, lo, hi): a NaN stays NaN (fminf / fmaxf would drop it)
MCAV_EV_HD float clip(float p, float lo, float hi) { return p < lo ? lo : (p > hi ? hi : p); }

// Per-pixel metric terms, float32 per pixel as compute_errors, summed in float64 by the caller.
// sums: 0..2 d1..d3 counts, 3 (g-p)^2, 4 (ln g - ln p)^2, 5 |g-p|/g, 6 (g-p)^2/g, 7 e = ln p - ln g, 8 e^2, 9 |log10 p - log10 g|, 10 count
constexpr int NSUM = 11;
MCAV_EV_HD void pixel_terms(float g, float p, double (&s)[NSUM]) {
    const float t = fmaxf(div_rn(g, p), div_rn(p, g));
    s[0] += t < 1.25f ? 1.0 : 0.0;
    s[1] += t < 1.5625f ? 1.0 : 0.0;
    s[2] += t < 1.953125f ? 1.0 : 0.0;
    const float d = add_rn(g, -p);
    const float lg = logf(g), lp = logf(p);
    const float dl = add_rn(lg, -lp);
    s[3] += (double)mul_rn(d, d);
    s[4] += (double)mul_rn(dl, dl);
    s[5] += (double)div_rn(fabsf(d), g);
    s[6] += (double)div_rn(mul_rn(d, d), g);
    const float e = add_rn(lp, -lg);
    s[7] += (double)e;
    s[8] += (double)mul_rn(e, e);
    s[9] += (double)fabsf(add_rn(log10f(p), -log10f(g)));
    s[10] += 1.0;
}

// One image's row from its sums: the nine metrics in evaluate.KEYS order (silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3).
// No pixel: NaN.  A NaN among the sums (from the data) propagates.
MCAV_EV_HD void metrics_row(const double (&s)[NSUM], float (&m)[9]) {
    const double n = s[10];
    if (!(n > 0.0)) {
        for (int k = 0; k < 9; ++k) m[k] = NAN;
        return;
    }
    const double me = s[7] / n;
    double var = s[8] / n - me * me;
    if (var < 0.0) var = 0.0;                         // rounding only (a NaN stays)
    m[0] = (float)(sqrt(var) * 100.0);
    m[1] = (float)(s[5] / n);
    m[2] = (float)(s[9] / n);
    m[3] = (float)sqrt(s[3] / n);
    m[4] = (float)(s[6] / n);
    m[5] = (float)sqrt(s[4] / n);
    m[6] = (float)(s[0] / n);
    m[7] = (float)(s[1] / n);
    m[8] = (float)(s[2] / n);
}

}  // namespace ev
}  // namespace mcav
