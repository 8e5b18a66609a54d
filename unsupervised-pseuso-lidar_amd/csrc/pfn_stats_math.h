// Arithmetic of the voxel moments and their adjoint (include/mcav_depth.h: mcav_pillar_moments, mcav_pillar_moments_bwd), shared by the HIP
// kernels (pfn_stats.hip) and by the host-compiled check in tests/pfn_stats_hostcheck (never by the product on the host, apart from the
// argument checks).  The definition is tests/pfn_stats_ref.py.  A term of a moment is the float64 product of two float32 values, which is
// exact, so fma(a, b, acc) is the float64 sum of the term and acc with one rounding; which order the terms come in is the kernel's.
#pragma once
#include "pfn_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcav {
namespace pfn {

constexpr int STATS_ROWS = 64;           // consecutive rows a wavefront takes at a time: one lane reads one row's count
constexpr int STATS_WAVES = 4;           // wavefronts of a workgroup
constexpr int STATS_GRID = 512;          // workgroups at most: the columns of the slab; group i of rows belongs to wavefront i % (4 grid)

MCAV_PFN_HD int stats_grid(long long capacity) {
    const long long per = (long long)STATS_ROWS * STATS_WAVES, c = (capacity + per - 1) / per;
    return c < 1 ? 1 : (c < STATS_GRID ? (int)c : STATS_GRID);
}

// what a lane accumulates: used, s[C], the upper triangle of M by rows
MCAV_PFN_HD constexpr int stats_triangle(int C) { return C * (C + 1) / 2; }
MCAV_PFN_HD constexpr int stats_sums(int C) { return 1 + C + stats_triangle(C); }
// what comes out: rows, used, s[C], M[C][C]
MCAV_PFN_HD constexpr int stats_moments(int C) { return 2 + C + C * C; }
// where M[c][d], c <= d, lies in the triangle
MCAV_PFN_HD constexpr int stats_at(int C, int c, int d) { return c * C - c * (c - 1) / 2 + (d - c); }

// one used slot x[C] into s[C] and the triangle tri[C (C + 1) / 2]
template <int C>
MCAV_PFN_HD void moments_add(const float* x, double* s, double* tri) {
    double v[C];
    for (int c = 0; c < C; ++c) v[c] = (double)x[c];
    int q = 0;
    for (int c = 0; c < C; ++c) {
        s[c] += v[c];
        for (int d = c; d < C; ++d, ++q) tri[q] = fma(v[c], v[d], tri[q]);
    }
}

// the adjoint's matrix: G[c][d] = H[c][d] + H[d][c] (the same bits on both sides of the diagonal)
MCAV_PFN_HD double adjoint_entry(const double* H, int C, int c, int d) { return H[c * C + d] + H[d * C + c]; }

// d_voxels[p, k, c] of a used slot x[C]: g[c], then one fma per column in ascending order, rounded once to float32.  G: row c of the
// adjoint's matrix
template <class Row, class X>
MCAV_PFN_HD float moments_bwd_value(double g, const Row& G, const X& x, int C) {
    double acc = g;
    for (int d = 0; d < C; ++d) acc = fma(G[d], (double)x[d], acc);
    return (float)acc;
}

}  // namespace pfn
}  // namespace mcav
