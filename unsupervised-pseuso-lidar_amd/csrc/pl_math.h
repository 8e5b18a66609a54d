// Per-pixel arithmetic of the pseudo-LiDAR projections (include/mcav_depth.h: mcav_pseudo_lidar_project, mcav_pl_batch_project), shared by
// the HIP kernels (post_ops.hip, pl_batch.hip) and by the host-compiled check in tests/pl_batch_hostcheck (never by the product on the
// host, apart from the calibration set-up of mcav_pseudo_lidar_project).  The definition of the batch form is tests/pl_batch_ref.py.
// Everything is float64 with every operation rounded on its own, as the reference's numpy arithmetic: the device build switches
// contraction off below, the host build is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eval_math.h"

#if defined(__HIPCC__)
#define MCAV_PL_HD __host__ __device__ __forceinline__
#else
#define MCAV_PL_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)           // the reference is numpy float64: keep mul / add separate as it does
#endif

namespace mcav {

struct PLCalib {
    double cu, cv, fu, fv, bx, by;       // from P_rect_02 (PseudoLiDAR.py:78-83)
    double ti[3][4];                     // rows 0..2 of inverse_rigid_trans(T) (PseudoLiDAR.py:39-46); its 4th row is zero
};

// T_velo_to_cam: 4x4 row-major (calib_velo_to_cam R|T); P_rect: 3x4 row-major (calib_cam_to_cam P_rect_02)
MCAV_PL_HD void pl_calib(const double* T, const double* P, PLCalib& c) {
    c.cu = P[2]; c.cv = P[4 + 2]; c.fu = P[0]; c.fv = P[4 + 1];
    c.bx = P[3] / (-c.fu); c.by = P[4 + 3] / (-c.fv);
    for (int i = 0; i < 3; ++i) {                         // inverse_rigid_trans: [R' | -R' t]
        for (int j = 0; j < 3; ++j) c.ti[i][j] = T[j * 4 + i];
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += -T[j * 4 + i] * T[j * 4 + 3];
        c.ti[i][3] = acc;
    }
}

// The velodyne-frame point of pixel (r, cc) at depth d
MCAV_PL_HD void pl_point_at(double d, int r, int cc, const PLCalib& c, double (&q)[3]) {
    const double x = (((double)cc - c.cu) * d) / c.fu + c.bx;
    const double y = (((double)r - c.cv) * d) / c.fv + c.by;
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = ((x * c.ti[j][0] + y * c.ti[j][1]) + d * c.ti[j][2]) + c.ti[j][3];
}

MCAV_PL_HD bool pl_point(const float* depth, int cols, const PLCalib& c, size_t i, double (&q)[3]) {
    const int r = (int)(i / cols), cc = (int)(i - (size_t)r * cols);
    pl_point_at((double)depth[i], r, cc, c, q);
    return q[0] >= 0.0 && q[2] < 1.0;
}

// ---------------------------------------------------------------------------------------------- the batch form (mcav_pl_batch_project)
namespace plb {

// float32 products and sums that stay apart on the device: compiled here, under contract(off), they carry no contraction flag.  The
// compiler's own __fmul_rn / __fadd_rn (eval_math.h's mul_rn / add_rn) are a plain * and + compiled where contraction is allowed, and a
// product of theirs that feeds a sum of theirs comes out of the backend as one fused multiply-add.
MCAV_PL_HD float mul(float a, float b) { return a * b; }
MCAV_PL_HD float add(float a, float b) { return a + b; }

// eval_math.h's bilinear_sample and disp_depth, operation for operation (its taps, weights, fused inner sums and division), with the
// products that feed a sum kept apart as the definition has them; on the host the two are the same function (tests/pl_batch_hostcheck).
MCAV_PL_HD float bilinear_sample(const float* plane, int h, int w, float sy, float sx, int y, int x) {
    int y0, y1, x0, x1;
    float ly, lx;
    ev::bilinear_axis(y, h, sy, y0, y1, ly);
    ev::bilinear_axis(x, w, sx, x0, x1, lx);
    const float hy = add(1.0f, -ly), hx = add(1.0f, -lx);
    const float* r0 = plane + (size_t)y0 * w;
    const float* r1 = plane + (size_t)y1 * w;
    const float t = ev::fma_rn(hx, r0[x0], mul(lx, r0[x1]));
    const float b = ev::fma_rn(hx, r1[x0], mul(lx, r1[x1]));
    return add(mul(hy, t), mul(ly, b));
}
MCAV_PL_HD float disp_depth(float d, float scale) { return mul(ev::div_rn(1.0f, add(mul(10.0f, d), 0.01f)), scale); }

// One plane [h, w] read at pixel (r, c) of an Hb x Wb image: the evaluation protocol's resize, or the value itself when the sizes agree
// (no taps: an infinite neighbour must not turn 0 * inf into NaN).
MCAV_PL_HD float sample(const float* plane, int h, int w, int Hb, int Wb, int r, int c) {
    if (h == Hb && w == Wb) return plane[(size_t)r * w + c];
    return bilinear_sample(plane, h, w, ev::axis_scale(h, Hb), ev::axis_scale(w, Wb), r, c);
}

// float32 depth of a sampled value: the evaluation protocol's 1 / (10 v + 0.01) * scale, or v * scale for a depth input
MCAV_PL_HD float depth_of(float v, float scale, bool input_depth) { return input_depth ? mul(v, scale) : disp_depth(v, scale); }

// dense-mode survivor; NaNs fail every comparison
MCAV_PL_HD bool keep(const double (&q)[3], float d, double max_height, double max_depth) {
    return q[0] >= 0.0 && q[2] < max_height && (double)d <= max_depth;
}

// k with tab[k] <= v < tab[k + 1] in a strictly increasing table of n + 1 edges; -1 outside it or for a NaN
MCAV_PL_HD int table_bin(const double* tab, int n, double v) {
    if (!(v >= tab[0]) || !(v < tab[n])) return -1;
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= tab[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

// The (beam, azimuth) cell of a survivor: s = q2 |q2| / (q0^2 + q1^2) against elev (tan e |tan e| at the beam edges), a = q1 / q0 against
// azim (tan phi at the azimuth edges).  false: in front of no cell.
MCAV_PL_HD bool beam_cell(const double (&q)[3], const double* elev, int nb, const double* azim, int na, int& beam, int& az) {
    if (!(q[0] > 0.0)) return false;
    const double s = (q[2] * fabs(q[2])) / (q[0] * q[0] + q[1] * q[1]);
    const double a = q[1] / q[0];
    beam = table_bin(elev, nb, s);
    az = table_bin(azim, na, a);
    return beam >= 0 && az >= 0;
}

// The squared range as float32 bits: non-negative, so the bits order it
MCAV_PL_HD uint32_t range_key(const double (&q)[3]) { return ev::float_bits((float)((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])); }

constexpr unsigned long long EMPTY_CELL = ~0ull;
MCAV_PL_HD unsigned long long cell_word(uint32_t key, uint32_t pixel) { return ((unsigned long long)key << 32) | pixel; }

// n + 1 finite, strictly increasing edges
inline bool table_ok(const double* tab, int n) {
    if (!tab || n < 1) return false;
    for (int k = 0; k <= n; ++k) {
        if (!(fabs(tab[k]) <= 1.79769313486231570815e+308)) return false;
        if (k > 0 && !(tab[k - 1] < tab[k])) return false;
    }
    return true;
}

}  // namespace plb
}  // namespace mcav
