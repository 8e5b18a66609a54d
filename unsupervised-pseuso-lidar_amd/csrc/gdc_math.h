// Per-pixel arithmetic of the graph-based depth correction (include/mcav_depth.h: mcav_gdc_graph, mcav_gdc_solve), shared by the HIP
// kernels (gdc.hip) and by the host-compiled check in tests/gdc_hostcheck (never by the product on the host, apart from the argument
// checks).  The definition is tests/gdc_ref.py.  float32 with every operation rounded on its own: the device build switches contraction
// off below (as pillar_math.h), the host build is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eval_math.h"

#if defined(__HIPCC__)
#define MCAV_GDC_HD __host__ __device__ __forceinline__
#else
#define MCAV_GDC_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)           // (u - cx) / fx * z, dx dx + dy dy and 1 - d t stay separate operations
#endif

namespace mcav {
namespace gdc {

constexpr int MAX_K = 16, MAX_RADIUS = 7;
constexpr unsigned char IN_GRAPH = 1, KNOWN = 2;
constexpr float F32_INF = __builtin_huge_valf();

struct Params {
    float reg, min_depth, max_depth;
    int k, radius;
};

// what mcav_gdc_graph accepts
MCAV_GDC_HD bool params_ok(const Params& p) {
    return p.k >= 1 && p.k <= MAX_K && p.radius >= 1 && p.radius <= MAX_RADIUS && p.reg > 0.0f && p.reg < F32_INF && p.min_depth >= 0.0f &&
           p.max_depth > p.min_depth;
}

// min_depth < z <= max_depth, compared as floats: a NaN or an infinity fails
MCAV_GDC_HD bool in_range(float z, float min_depth, float max_depth) { return z > min_depth && z <= max_depth; }

struct Point {
    float x, y, z;
};

// X = ((u - cx) / fx * z, (v - cy) / fy * z, z): IEEE division, then the product
MCAV_GDC_HD Point back_project(int u, int v, float z, float fx, float fy, float cx, float cy) {
    Point p;
    p.x = ev::div_rn((float)u - cx, fx) * z;
    p.y = ev::div_rn((float)v - cy, fy) * z;
    p.z = z;
    return p;
}

MCAV_GDC_HD float dist2(const Point& a, const Point& b) {
    const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// The K best of a stream of candidates offered in ascending index order: `d`, `id` ascending by (distance, index), +inf / -1 in the free
// slots.  A candidate goes in front of the first entry it is strictly below, so equal distances keep the earlier (lower) index; a distance
// that is not below +inf (an overflow, a NaN) is never taken.  Every index is a compile-time constant: the lists stay in registers.
template <int K>
MCAV_GDC_HD void best_init(float (&d)[K], int (&id)[K]) {
#pragma unroll
    for (int s = 0; s < K; ++s) { d[s] = F32_INF; id[s] = -1; }
}

template <int K>
MCAV_GDC_HD void best_insert(float (&d)[K], int (&id)[K], float cd, int cid) {
#pragma unroll
    for (int s = K - 1; s >= 0; --s) {
        const bool here = cd < d[s];
        if (s > 0) {
            const bool before = cd < d[s - 1];
            id[s] = before ? id[s - 1] : (here ? cid : id[s]);
            d[s] = before ? d[s - 1] : (here ? cd : d[s]);
        } else {
            id[s] = here ? cid : id[s];
            d[s] = here ? cd : d[s];
        }
    }
}

// The locally-linear-embedding weights of one pixel on its neighbours' depths (sklearn.manifold.barycenter_weights with a scalar
// feature; C = d d^T + lam I is rank one plus a ridge, so Sherman-Morrison gives w_j ~ 1 - d_j s / (lam + q)).  dz[s] = z_j - z_i for the
// m used slots, in neighbour order; w[s] for s >= m is +0.0.  Only the first k slots of the K are looked at.
template <int K>
MCAV_GDC_HD void lle_weights(const float (&dz)[K], int m, int k, float reg, float (&w)[K]) {
    float s = 0.0f, q = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k && j < m) { s = s + dz[j]; q = q + dz[j] * dz[j]; }
    const float lam = q > 0.0f ? reg * q : reg;
    const float t = ev::div_rn(s, lam + q);
    float tot = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        w[j] = 0.0f;
        if (j < k && j < m) { w[j] = 1.0f - dz[j] * t; tot = tot + w[j]; }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k && j < m) w[j] = ev::div_rn(w[j], tot);
}

}  // namespace gdc
}  // namespace mcav
