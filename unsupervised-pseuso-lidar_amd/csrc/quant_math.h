// Arithmetic of the soft-occupancy grid (include/mcav_depth.h: mcav_cloud_occupancy, mcav_cloud_occupancy_bwd): End-to-End Pseudo-LiDAR's
// soft quantisation of a cloud batch into a dense [B, nz, ny, nx] canvas for detectors that read voxel occupancy (PIXOR).  Shared by the
// HIP kernels (quant.hip) and by the host-compiled check in tests/quant_hostcheck (never by the product on the host, apart from the
// argument checks and the workspace layout).  The definition is tests/quant_ref.py.  float32 with every operation rounded on its own and
// fmaf where the definition says fmaf; float64 where it says float64: the device build switches contraction off below (as pl_math.h),
// the host build is compiled with -ffp-contract=off.
#pragma once
#include "pillar_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcav {
namespace qnt {

constexpr int MAX_NZ = 64;               // z bins of a canvas: a tile of 64 bins of 64-bit sums is 128 KB of the 160 KB of LDS
constexpr int TILE_X = 64, TILE_Y = 4;   // BEV columns of one workgroup of the count and canvas kernels
constexpr int SCAN_TILE = 1024;          // column counters per workgroup of the scan passes
constexpr int REFUSED = -1, SHORT_WORKSPACE = -2;      // MCAV_E_INVALID, MCAV_E_WORKSPACE

struct Grid {
    float x0, y0, z0, vx, vy, vz;
    int nx, ny, nz;
};

// what mcav_cloud_occupancy accepts as a grid and as a width
MCAV_PIL_HD bool grid_ok(const Grid& g) {
    return g.nx >= 1 && g.ny >= 1 && g.nz >= 1 && g.nz <= MAX_NZ && pil::finite(g.vx) && g.vx > 0.0f && pil::finite(g.vy) && g.vy > 0.0f &&
           pil::finite(g.vz) && g.vz > 0.0f && pil::finite(g.x0) && pil::finite(g.y0) && pil::finite(g.z0);
}
MCAV_PIL_HD bool sigma2_ok(float sigma2) { return pil::finite(sigma2) && sigma2 > 0.0f; }

// pillar_math.h's rule on all three axes: the point is kept iff every floorf((v - origin) / size) names a cell, compared as floats
MCAV_PIL_HD bool cell_of(const Grid& g, float x, float y, float z, int& ix, int& iy, int& iz) {
    return pil::axis_cell(x, g.x0, g.vx, g.nx, ix) && pil::axis_cell(y, g.y0, g.vy, g.ny, iy) && pil::axis_cell(z, g.z0, g.vz, g.nz, iz);
}

// ---------------------------------------------------------------------------------------------- quant_exp
// exp(t) in float32 for t <= 0 from fmaf, float32 sums and integer exponent arithmetic alone, so that the host and the device give the same
// bits.  t < QEXP_CUT (and a NaN) gives +0: every result that is not zero is a normal number.  k = the nearest integer to t log2(e) (the
// 1.5 * 2^23 trick: the sum's rounding does it), r = (t - k LN2_HI) - k LN2_LO (Cody-Waite: k LN2_HI is exact, it has 8 + 11 bits), the
// Taylor polynomial of degree 7 in r by Horner's rule, then k added to the exponent field.
// QEXP_MAX_ULP bounds |quant_exp(t) - exp(t)| in units of the last place of exp(t), over EVERY float32 t in [QEXP_CUT, -0] and +0
// (1 118 699 522 arguments), measured against the float64 exponential by tests/quant_hostcheck (`quant_hostcheck --exp-ulp`): the maximum
// found is 0.937081 ulp, at t = -0x1.79082cp+2.
constexpr float QEXP_CUT = -87.0f;       // exp(-87) = 1.65e-38 > FLT_MIN = 1.18e-38
constexpr float QEXP_MAX_ULP = 0.9375f;
constexpr float QEXP_LOG2E = 1.44269504088896341f;
constexpr float QEXP_LN2_HI = 0.693359375f, QEXP_LN2_LO = -2.12194440e-4f;
constexpr float QEXP_ROUND = 12582912.0f;

MCAV_PIL_HD float quant_exp(float t) {
    if (!(t >= QEXP_CUT)) return 0.0f;
    const float kf = ev::add_rn(ev::fma_rn(t, QEXP_LOG2E, QEXP_ROUND), -QEXP_ROUND);
    float r = ev::fma_rn(kf, -QEXP_LN2_HI, t);
    r = ev::fma_rn(kf, -QEXP_LN2_LO, r);
    float p = 1.0f / 5040.0f;
    p = ev::fma_rn(p, r, 1.0f / 720.0f);
    p = ev::fma_rn(p, r, 1.0f / 120.0f);
    p = ev::fma_rn(p, r, 1.0f / 24.0f);
    p = ev::fma_rn(p, r, 1.0f / 6.0f);
    p = ev::fma_rn(p, r, 0.5f);
    p = ev::fma_rn(p, r, 1.0f);
    p = ev::fma_rn(p, r, 1.0f);
    const int k = (int)kf;                                  // in [-126, 0]
    return ev::bits_float(ev::float_bits(p) + ((uint32_t)k << 23));
}

// ---------------------------------------------------------------------------------------------- one term
// e = quant_exp(-(|p - c|^2 / sigma2)) of a point against a cell's centre; d[3] = p - c, as the backward needs it
MCAV_PIL_HD float term(float x, float y, float z, float cx, float cy, float cz, float sigma2, float (&d)[3]) {
    d[0] = x - cx;
    d[1] = y - cy;
    d[2] = z - cz;
    float d2 = d[0] * d[0];
    d2 = ev::fma_rn(d[1], d[1], d2);
    d2 = ev::fma_rn(d[2], d[2], d2);
    return quant_exp(-ev::div_rn(d2, sigma2));
}

// The term in 2^-40 units, over the points of its cell (and the 26 neighbours when it lands on one): sums of these are integers and do
// not depend on their order.  A cell's own terms add up to at most 2^40 and every neighbour's to 2^40 / 26: no sum passes 2^41.
constexpr double FIXED_ONE = 1099511627776.0;               // 2^40
MCAV_PIL_HD long long to_fixed(float e, int count, bool own) {
    const long long den = (long long)count * (own ? 1 : 26);
    return llrint(((double)e * FIXED_ONE) / (double)den);
}
MCAV_PIL_HD float from_fixed(long long s) { return (float)((double)s * (1.0 / FIXED_ONE)); }

// ---------------------------------------------------------------------------------------------- backward
// d_points[i][0..2] of a kept point in cell (ix, iy, iz) with `count` points: the derivative of the unrounded expression, every factor
// promoted to float64, the 27 terms added in ascending (dz, dy, dx) order from +0 and rounded once.  d_canvas: the image's [nz, ny, nx]
// block; neighbours outside the grid have no term.
MCAV_PIL_HD void point_grad(const Grid& g, float sigma2, const float* d_canvas, float x, float y, float z, int ix, int iy, int iz, int count,
                            float (&out)[3]) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (int oz = -1; oz <= 1; ++oz)
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const int jx = ix + ox, jy = iy + oy, jz = iz + oz;
                if (jx < 0 || jx >= g.nx || jy < 0 || jy >= g.ny || jz < 0 || jz >= g.nz) continue;
                float d[3];
                const float e = term(x, y, z, pil::cell_centre(jx, g.x0, g.vx), pil::cell_centre(jy, g.y0, g.vy),
                                     pil::cell_centre(jz, g.z0, g.vz), sigma2, d);
                const double w = (ox | oy | oz) ? 1.0 / 26.0 : 1.0;
                const double c = ((double)d_canvas[((size_t)jz * g.ny + jy) * g.nx + jx] * (w / (double)count)) * (double)e;
                for (int a = 0; a < 3; ++a) acc[a] += c * ((-2.0 * (double)d[a]) / (double)sigma2);
            }
    for (int a = 0; a < 3; ++a) out[a] = (float)acc[a];
}

// ---------------------------------------------------------------------------------------------- the calls' arguments (host)
// Workspace of mcav_cloud_occupancy: the per-column counters (+ the total), their tile sums, and per row the (column, slot) pair, the
// sorted row index and the sorted rows' cell counts; each piece rounded up to 256 bytes.
struct Layout {
    size_t cells, tile_sums, rec, index, cnt, total;
    unsigned M, ntiles;
};

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline bool layout(int B, long long n_max, int nz, int ny, int nx, Layout& l) {
    if (B <= 0 || B > 65535 || n_max < 0 || n_max > 0x7fffffffll || nx < 1 || ny < 1 || nz < 1 || nz > MAX_NZ) return false;
    const unsigned long long M = (unsigned long long)B * (unsigned long long)ny * (unsigned long long)nx;
    if (M > 0x7fffffffull || M * (unsigned long long)nz > 0x7fffffffull) return false;       // int32 canvas elements
    l.M = (unsigned)M;
    l.ntiles = (unsigned)((M + SCAN_TILE - 1) / SCAN_TILE);
    l.cells = 0;
    l.tile_sums = l.cells + round_up(sizeof(unsigned) * ((size_t)M + 1), 256);
    l.rec = l.tile_sums + round_up(sizeof(unsigned) * l.ntiles, 256);
    l.index = l.rec + round_up(8 * (size_t)n_max, 256);
    l.cnt = l.index + round_up(sizeof(int) * (size_t)n_max, 256);
    l.total = l.cnt + round_up(sizeof(int) * (size_t)n_max, 256);
    return true;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// 0, or the code mcav_cloud_occupancy returns without launching anything
inline int forward_refusal(const float* points, const int* offsets, int B, long long n_max, const Grid& g, float sigma2, const float* canvas,
                           const int* point_count, const void* workspace, size_t workspace_bytes) {
    Layout l;
    if (!points || !offsets || !canvas || !workspace) return REFUSED;
    if (!grid_ok(g) || !sigma2_ok(sigma2) || !layout(B, n_max, g.nz, g.ny, g.nx, l)) return REFUSED;
    if (!aligned(points, 16) || !aligned(canvas, 16) || !aligned(workspace, 16) || !aligned(offsets, 4) || !aligned(point_count, 4)) return REFUSED;
    return workspace_bytes < l.total ? SHORT_WORKSPACE : 0;
}

inline int backward_refusal(const float* points, const int* offsets, const int* point_count, const float* d_canvas, int B, long long n_max,
                            const Grid& g, float sigma2, const float* d_points) {
    Layout l;
    if (!points || !offsets || !point_count || !d_canvas || !d_points) return REFUSED;
    if (!grid_ok(g) || !sigma2_ok(sigma2) || !layout(B, n_max, g.nz, g.ny, g.nx, l)) return REFUSED;
    if (!aligned(points, 16) || !aligned(d_points, 16) || !aligned(d_canvas, 4) || !aligned(offsets, 4) || !aligned(point_count, 4)) return REFUSED;
    return 0;
}

}  // namespace qnt
}  // namespace mcav
