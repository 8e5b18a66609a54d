// Per-pixel arithmetic of the ground-plane scale estimator (include/mcav_depth.h: mcav_ground_scale), shared by the HIP kernels
// (ground_scale.hip) and by the host-compiled check in tests/ground_hostcheck (never by the product on the host).  The definition is
// tests/ground_scale_ref.py: float32 with every operation rounded on its own, as numpy float32 arithmetic.  The device build switches
// contraction off below (pl_math.h tells why __fmul_rn / __fadd_rn alone do not keep a product and a sum apart), the host build is compiled
// with -ffp-contract=off; division and square root are the correctly rounded ones: `/` and sqrtf as hipcc compiles them by default (the
// compiler's __fsqrt_rn is NOT that here: without OCML_BASIC_ROUNDED_OPERATIONS it is the hardware's approximate square root).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eval_math.h"

#if defined(__HIPCC__)
#define MCAV_GS_HD __host__ __device__ __forceinline__
#else
#define MCAV_GS_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)           // the definition is numpy float32: keep mul / add separate as it does
#endif

namespace mcav {
namespace gs {

constexpr uint32_t NOT_GROUND = 0xffffffffu;             // the key of a pixel that is no ground pixel; a ground pixel's key is the bits of hgt

MCAV_GS_HD float mul(float a, float b) { return a * b; }
MCAV_GS_HD float add(float a, float b) { return a + b; }
MCAV_GS_HD float sub(float a, float b) { return a - b; }
MCAV_GS_HD float sqrt_rn(float a) { return sqrtf(a); }
MCAV_GS_HD bool finite_positive(float a) { return a > 0.0f && a <= 3.40282346638528859812e+38f; }      // a NaN fails

// xn[c] (or yn[r]): the ray of network pixel i of n_net along an axis of n_true native pixels, float64 in this order, rounded once
MCAV_GS_HD float ray(int i, int n_true, int n_net, double centre, double focal) {
    return (float)((((((double)i + 0.5) * (double)n_true) / (double)n_net - 0.5) - centre) / focal);
}

MCAV_GS_HD float depth_of(float v, bool input_depth) { return input_depth ? v : ev::div_rn(1.0f, add(mul(10.0f, v), 0.01f)); }

struct Box {
    int y0, y1, x0, x1;                  // half-open, inside [0, h] x [0, w]
};
// boxes[4] = (y0, y1, x0, x1) as the caller gave them, clamped; null: everything
MCAV_GS_HD Box clamp_box(const int* box, int h, int w) {
    Box r = {0, h, 0, w};
    if (!box) return r;
    r.y0 = box[0] < 0 ? 0 : (box[0] > h ? h : box[0]);
    r.y1 = box[1] < r.y0 ? r.y0 : (box[1] > h ? h : box[1]);
    r.x0 = box[2] < 0 ? 0 : (box[2] > w ? w : box[2]);
    r.x1 = box[3] < r.x0 ? r.x0 : (box[3] > w ? w : box[3]);
    return r;
}
MCAV_GS_HD bool in_box(const Box& b, int r, int c) { return r >= b.y0 && r < b.y1 && c >= b.x0 && c < b.x1; }

// The 3x3 neighbourhood of a pixel as points: index k = (dr + 1) * 3 + (dc + 1), the centre at 4
constexpr int CENTRE = 4;
// R D L U DR DL UL UR as neighbourhood indices, and the pairs whose cross products are taken, in the definition's order
#define MCAV_GS_NEIGHBOURS {5, 7, 3, 1, 8, 6, 0, 2}
#define MCAV_GS_PAIRS {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}}

// Ground test of one interior pixel from its neighbourhood; hgt is its height above the plane through the camera centre (defined whenever
// the normal is).  false: no ground pixel.
MCAV_GS_HD bool ground_pixel(const float (&X)[9], const float (&Y)[9], const float (&Z)[9], float cos_max, float& hgt) {
    const int nb[8] = MCAV_GS_NEIGHBOURS;
    const int pr[8][2] = MCAV_GS_PAIRS;
    float ex[8], ey[8], ez[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ex[k] = sub(X[nb[k]], X[CENTRE]);
        ey[k] = sub(Y[nb[k]], Y[CENTRE]);
        ez[k] = sub(Z[nb[k]], Z[CENTRE]);
    }
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int a = pr[k][0], b = pr[k][1];
        const float cx = sub(mul(ey[a], ez[b]), mul(ez[a], ey[b]));
        const float cy = sub(mul(ez[a], ex[b]), mul(ex[a], ez[b]));
        const float cz = sub(mul(ex[a], ey[b]), mul(ey[a], ex[b]));
        const float len = sqrt_rn(add(add(mul(cx, cx), mul(cy, cy)), mul(cz, cz)));
        ok = ok && finite_positive(len);
        ax = add(ax, ev::div_rn(cx, len));
        ay = add(ay, ev::div_rn(cy, len));
        az = add(az, ev::div_rn(cz, len));
    }
    const float L = sqrt_rn(add(add(mul(ax, ax), mul(ay, ay)), mul(az, az)));
    const float nx = ev::div_rn(ax, L), ny = ev::div_rn(ay, L), nz = ev::div_rn(az, L);
    hgt = add(add(mul(nx, X[CENTRE]), mul(ny, Y[CENTRE])), mul(nz, Z[CENTRE]));
    return ok && finite_positive(L) && ny >= cos_max && finite_positive(hgt);
}

MCAV_GS_HD uint32_t pixel_key(bool ground, float hgt) { return ground ? ev::float_bits(hgt) : NOT_GROUND; }

// rows[b] from the count and the two middle order statistics (ranks floor((n-1)/2) and n/2) of the ground pixels' heights
MCAV_GS_HD void image_row(uint32_t count, float lo, float hi, float camera_height, int min_ground, float fallback, float (&row)[4]) {
    const float med = count ? ev::median_of(lo, hi, count) : NAN;
    const bool valid = count >= (uint32_t)min_ground;
    row[0] = valid ? ev::div_rn(camera_height, med) : fallback;
    row[1] = med;
    row[2] = (float)count;
    row[3] = valid ? 1.0f : 0.0f;
}

// The arguments mcav_ground_scale refuses (sizes and pointers apart)
inline bool scalars_ok(float camera_height, float cos_max, int min_ground, int flags) {
    return finite_positive(camera_height) && cos_max > 0.0f && cos_max <= 1.0f && min_ground >= 1 && !(flags & ~1);
}

}  // namespace gs
}  // namespace mcav
