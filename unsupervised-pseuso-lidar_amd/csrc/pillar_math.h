// Per-point and per-pillar arithmetic of the pillar voxeliser (include/mcav_depth.h: mcav_pillarize), shared by the HIP kernels
// (pillarize.hip) and by the host-compiled check in tests/pillar_hostcheck (never by the product on the host, apart from the argument
// checks).  The definition is tests/pillar_ref.py.  float32 with every operation rounded on its own: the device build switches
// contraction off below (as pl_math.h), the host build is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eval_math.h"

#if defined(__HIPCC__)
#define MCAV_PIL_HD __host__ __device__ __forceinline__
#else
#define MCAV_PIL_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)           // v * 0.5 + x0 and ix * v + c stay a product and a sum
#endif

namespace mcav {
namespace pil {

constexpr int MAX_POINTS = 64;           // one wavefront holds a pillar's slots
constexpr int COLS_PLAIN = 4, COLS_DECORATED = 9;
constexpr float F32_MAX = 3.40282346638528859812e+38f;

struct Grid {
    float x0, y0, z0, z1, vx, vy;
    int nx, ny;
};

MCAV_PIL_HD bool finite(float v) { return fabsf(v) <= F32_MAX; }          // false for a NaN

// what mcav_pillarize accepts as a grid
MCAV_PIL_HD bool grid_ok(const Grid& g) {
    return g.nx >= 1 && g.ny >= 1 && finite(g.vx) && g.vx > 0.0f && finite(g.vy) && g.vy > 0.0f && finite(g.x0) && finite(g.y0) &&
           g.z1 > g.z0;
}

// The image that owns row i of a cloud batch: the b with offsets[b] <= i < offsets[b + 1] (offsets ascending, i < offsets[B]); images
// without rows are stepped over.  Always in [0, B - 1], whatever the table holds.
MCAV_PIL_HD int image_of(const int* offsets, int B, int i) {
    int lo = 0, hi = B;                                    // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// One axis: floor((v - origin) / size) as a float, and whether it names a cell.  Compared as floats: a NaN or an infinity fails, -0.0
// passes as cell 0.  The conversion to int happens only after the test.
MCAV_PIL_HD bool axis_cell(float v, float origin, float size, int n, int& cell) {
    const float f = floorf(ev::div_rn(v - origin, size));
    if (!(f >= 0.0f && f < (float)n)) return false;
    cell = (int)f;
    return cell < n;                                       // (float)n rounds up above 2^24: never past the grid
}

MCAV_PIL_HD bool cell_of(const Grid& g, float x, float y, float z, int& ix, int& iy) {
    return axis_cell(x, g.x0, g.vx, g.nx, ix) && axis_cell(y, g.y0, g.vy, g.ny, iy) && z >= g.z0 && z < g.z1;
}

// centre of cell i along an axis: (float)i * size + (size * 0.5 + origin)
MCAV_PIL_HD float cell_centre(int i, float origin, float size) { return (float)i * size + (size * 0.5f + origin); }

// mean of one column over a pillar's kept slots: the float64 sum in slot order from +0, over the count, rounded once to float32
MCAV_PIL_HD float column_mean(const float* rows, int stride, int count) {
    double acc = 0.0;
    for (int k = 0; k < count; ++k) acc += (double)rows[(size_t)k * stride];
    return (float)(acc / (double)count);
}

// columns 4..8 of a decorated slot from its x, y, z: offsets from the pillar's mean and from the cell's centre
MCAV_PIL_HD void decorate(float x, float y, float z, float mx, float my, float mz, float cx, float cy, float* out5) {
    out5[0] = x - mx;
    out5[1] = y - my;
    out5[2] = z - mz;
    out5[3] = x - cx;
    out5[4] = y - cy;
}

// One step of the ordered selection.  `kept` holds k point indices, `chunk` c more (all distinct); an entry's rank among the k + c is the
// number of entries below it, and the entries of rank < limit form the new kept set, in ascending order, in `next`.  One caller per
// entry: `mine` is that entry; the return value is its rank.
MCAV_PIL_HD int rank_among(int mine, const int* kept, int k, const int* chunk, int c) {
    int r = 0;
    for (int j = 0; j < k; ++j) r += kept[j] < mine ? 1 : 0;
    for (int j = 0; j < c; ++j) r += chunk[j] < mine ? 1 : 0;
    return r;
}

}  // namespace pil
}  // namespace mcav
