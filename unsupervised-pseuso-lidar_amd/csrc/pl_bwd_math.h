// Arithmetic of the two backwards that carry a gradient from pillar voxels back to the network's plane (include/mcav_depth.h:
// mcav_pillarize_bwd, mcav_pl_batch_project_bwd), shared by the HIP kernels (pl_bwd.hip) and by the host-compiled check in
// tests/pl_bwd_hostcheck (never by the product on the host).  The definition is tests/pl_bwd_ref.py.  The selection (which pixel became
// which cloud row, which row which slot) is piecewise constant and is taken from the forwards' provenance; what is differentiated is the
// arithmetic behind it.  Sums and products are float64 with every operation rounded on its own and one rounding to float32 at the store:
// the device build switches contraction off below (as pl_math.h), the host build is compiled with -ffp-contract=off.
#pragma once
#include "pillar_math.h"
#include "pl_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcav {
namespace plg {

// ---------------------------------------------------------------------------------------------- voxels -> cloud rows
// float64 sum of one column of a pillar's gradient rows over its used slots, in slot order from +0 (what column_mean's derivative needs)
MCAV_PIL_HD double column_sum(const float* rows, int stride, int count) {
    double acc = 0.0;
    for (int k = 0; k < count; ++k) acc += (double)rows[(size_t)k * stride];
    return acc;
}

// Column `col` (0..3) of the gradient of the cloud row held by one used slot.  g: the slot's C gradient columns; S: column_sum of column
// 4 + col of the pillar (col < 3, decorated only).  Decorated: x collects its own column, its offset from the mean (which also pulls on
// every other slot through the mean: - S / count) and its offset from the cell's centre, a constant; z has no centre column.
MCAV_PIL_HD float point_grad(const float* g, int C, int col, double S, int count) {
    if (C == pil::COLS_PLAIN || col == 3) return g[col];
    double own = (double)g[col] + (double)g[4 + col];
    if (col < 2) own = own + (double)g[7 + col];
    return (float)(own - S / (double)count);
}

// ---------------------------------------------------------------------------------------------- cloud rows -> the resized plane G
// The scale of image b as the forward forms it (pl_batch.hip image_scale); false: the image kept no pixel
MCAV_PL_HD bool image_scale(float scale, const float* scales, int b, float& s) {
    s = scale;
    if (!scales) return true;
    s = plb::mul(scale, scales[b]);
    return s > 0.0f && s <= 3.40282346638528859812e+38f;
}

// d(q . g) / dv at pixel (r, c): g holds the row's three gradient columns, v is the sampled plane value, s the image's scale.  The point
// is linear in the depth d, q_j = a_j d + const with a_j below; d = s / (10 v + 0.01) or s v.  The cloud's float32 rounding of q has
// derivative 1.
MCAV_PL_HD float plane_grad(const float* g, float v, float s, bool input_depth, int r, int c, const PLCalib& k) {
    const double xn = ((double)c - k.cu) / k.fu, yn = ((double)r - k.cv) / k.fv;
    double a[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = (xn * k.ti[j][0] + yn * k.ti[j][1]) + k.ti[j][2];
    const double gd = ((double)g[0] * a[0] + (double)g[1] * a[1]) + (double)g[2] * a[2];
    double slope = (double)s;
    if (!input_depth) {
        const double u = 1.0 / (10.0 * (double)v + 0.01);
        slope = ((-10.0 * (double)s) * u) * u;
    }
    return (float)(gd * slope);
}

// ---------------------------------------------------------------------------------------------- G -> the network's plane (resize adjoint)
// The first output whose lower tap is >= i; n_out when there is none.  ev::bilinear_axis' lower tap never decreases with the output index
// (every float32 operation of it is monotone), so the bisection over the function itself is exact (as pyramid_math.h first_output_at).
MCAV_PL_HD int first_output_at(int i, int n_in, float scale, int n_out) {
    int lo = 0, hi = n_out;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        int i0, i1;
        float l;
        ev::bilinear_axis(mid, n_in, scale, i0, i1, l);
        if (i0 >= i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Outputs [lo, hi] whose taps touch source i: those whose lower tap is i - 1 or i
MCAV_PL_HD void adjoint_window(int i, int n_in, float scale, int n_out, int& lo, int& hi) {
    lo = first_output_at(i - 1, n_in, scale, n_out);
    hi = first_output_at(i + 1, n_in, scale, n_out) - 1;
}

// The forward's float32 weight of source i in output o along one axis: 1 - l at the lower tap, l at the upper, both added (in float32)
// when they coincide at the last source
MCAV_PL_HD float tap_weight(int o, int i, int n_in, float scale) {
    int i0, i1;
    float l;
    ev::bilinear_axis(o, n_in, scale, i0, i1, l);
    float wgt = 0.0f;
    if (i0 == i) wgt = plb::add(wgt, plb::add(1.0f, -l));
    if (i1 == i) wgt = plb::add(wgt, l);
    return wgt;
}

// d_m[y][x] of an image: G [.., Wg] is its plane of the padded grid, (Hb, Wb) its true size.  The float64 sum over the outputs (r, c) whose
// taps touch (y, x), r ascending and c ascending inside, of (wy wx) G, rounded once; G itself when the sizes agree.
MCAV_PL_HD float resize_adjoint(const float* G, int Wg, int h, int w, int Hb, int Wb, int y, int x) {
    if (h == Hb && w == Wb) return G[(size_t)y * Wg + x];
    const float sy = ev::axis_scale(h, Hb), sx = ev::axis_scale(w, Wb);
    int r0, r1, c0, c1;
    adjoint_window(y, h, sy, Hb, r0, r1);
    adjoint_window(x, w, sx, Wb, c0, c1);
    double acc = 0.0;
    for (int r = r0; r <= r1; ++r) {
        const double wy = (double)tap_weight(r, y, h, sy);
        for (int c = c0; c <= c1; ++c) acc += (wy * (double)tap_weight(c, x, w, sx)) * (double)G[(size_t)r * Wg + c];
    }
    return (float)acc;
}

}  // namespace plg
}  // namespace mcav
