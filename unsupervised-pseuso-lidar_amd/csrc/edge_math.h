// Per-pixel arithmetic of monodepth2's edge-aware smoothness on mean-normalised disparity, shared by the HIP kernels (edge_smooth.hip)
// and by the host-compiled check in tests/edge_hostcheck (never by the product).  The definition (include/mcav_depth.h,
// mcav_edge_smooth_fwd): for one sample, disparity d [h,w], image I_s = the f x f box average of the full-resolution image,
//   wx(y,x) = exp(-mean_c |I_s(c,y,x) - I_s(c,y,x+1)|),  wy likewise along y,
//   R = cx sum |d(y,x) - d(y,x+1)| wx  +  cy sum |d(y,x) - d(y+1,x)| wy,   cx = 1/(B h (w-1)),  cy = 1/(B (h-1) w),
//   E = R / (m + 1e-7),  m = mean of d,
//   dE/dd_i = dR/dd_i / (m + 1e-7)  -  R / ((m + 1e-7)^2 h w).
// A pixel's loss part is its right and lower pair; its gradient stencil is the four pairs it belongs to.  |.|' at 0 is 0 (torch's sign).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define MCAV_ES_HD __host__ __device__ __forceinline__
#else
#define MCAV_ES_HD inline
#endif

namespace mcav {
namespace es {

constexpr double EPS = 1e-7;      // monodepth2: disp / (mean_disp + 1e-7)

struct Rgb {
    float c[3];
};

MCAV_ES_HD float sign_of(float v) { return (float)((v > 0.0f) - (v < 0.0f)); }

// I_s(c, y, x) of one channel plane of the full-resolution image (row stride W): the f x f box average, rows then columns, in fp32
MCAV_ES_HD float box_tap(const float* plane, int W, int f, int y, int x) {
    if (f == 1) return plane[(size_t)y * W + x];
    float s = 0.f;
    for (int i = 0; i < f; ++i) {
        const float* row = plane + (size_t)(y * f + i) * W + (size_t)x * f;
        for (int j = 0; j < f; ++j) s += row[j];
    }
    return s / (float)(f * f);
}

// the three channels of I_s at (y, x); img points at the sample's first plane, hw_full = H * W
MCAV_ES_HD Rgb rgb_at(const float* img, size_t hw_full, int W, int f, int y, int x) {
    Rgb r;
    for (int c = 0; c < 3; ++c) r.c[c] = box_tap(img + c * hw_full, W, f, y, x);
    return r;
}

// exp(-(1/3) sum_c |a_c - b_c|): symmetric in its arguments, bit for bit
MCAV_ES_HD float edge_weight(const Rgb& a, const Rgb& b) {
    return expf(-((fabsf(a.c[0] - b.c[0]) + fabsf(a.c[1] - b.c[1])) + fabsf(a.c[2] - b.c[2])) / 3.0f);
}

// The pair factors of one sample: a direction without pairs (w == 1 or h == 1) gets 0.
MCAV_ES_HD void pair_scales(int B, int h, int w, float& cx, float& cy) {
    cx = w > 1 ? (float)(1.0 / ((double)B * h * (w - 1))) : 0.f;
    cy = h > 1 ? (float)(1.0 / ((double)B * (h - 1) * w)) : 0.f;
}

// Pixel (y, x)'s part of R: its pair to the right and its pair below.  D(y, x) -> disparity, C(y, x) -> Rgb of I_s.
// A neighbour beyond the last column / row is clamped onto the pixel itself: |d - d| = 0 and sign(0) = 0 add exactly +0, so the border
// needs no branch and the kernels issue every load of a pixel at once.
template <class Dv, class Cv>
MCAV_ES_HD float pixel_loss(Dv D, Cv C, int y, int x, int h, int w, float cx, float cy) {
    const int xr = x < w - 1 ? x + 1 : x, yd = y < h - 1 ? y + 1 : y;
    const float d0 = D(y, x);
    const Rgb c0 = C(y, x);
    return fabsf(d0 - D(y, xr)) * edge_weight(c0, C(y, xr)) * cx + fabsf(d0 - D(yd, x)) * edge_weight(c0, C(yd, x)) * cy;
}

// dR / dd at (y, x): the four pairs the pixel belongs to (clamped neighbours as in pixel_loss)
template <class Dv, class Cv>
MCAV_ES_HD float pixel_stencil(Dv D, Cv C, int y, int x, int h, int w, float cx, float cy) {
    const int xr = x < w - 1 ? x + 1 : x, xl = x > 0 ? x - 1 : x;
    const int yd = y < h - 1 ? y + 1 : y, yu = y > 0 ? y - 1 : y;
    const float d0 = D(y, x);
    const Rgb c0 = C(y, x);
    const float gx = sign_of(d0 - D(y, xr)) * edge_weight(c0, C(y, xr)) - sign_of(D(y, xl) - d0) * edge_weight(c0, C(y, xl));
    const float gy = sign_of(d0 - D(yd, x)) * edge_weight(c0, C(yd, x)) - sign_of(D(yu, x) - d0) * edge_weight(c0, C(yu, x));
    return gx * cx + gy * cy;
}

// The per-sample finish, from the sums over the sample's pixels: m = sum d / (h w), R = sum of pixel_loss.
MCAV_ES_HD double sample_loss(double m, double R) { return R / (m + EPS); }

// The two per-sample factors of the gradient: dE/dd_i = stencil_i * inv - k
MCAV_ES_HD void grad_factors(double m, double R, int h, int w, float& inv, float& k) {
    const double me = m + EPS;
    inv = (float)(1.0 / me);
    k = (float)(R / (me * me * ((double)h * w)));
}

MCAV_ES_HD float pixel_grad(float stencil, float inv, float k) { return stencil * inv - k; }

}  // namespace es
}  // namespace mcav
