// TEST INFRASTRUCTURE (CPU): drives the per-point math of csrc/velo_math.h -- the functions the projection kernel (csrc/velo_depth.hip)
// calls -- with a plain host loop.  Built by tests/test_velodyne_cpu.py with g++ -ffp-contract=off; never loaded by the product.
#include <cstddef>
#include <cstdint>

#include "velo_math.h"

using namespace mcav;

// For every point of pts [n,4]: landed[i], u[i], v[i] (-1 when it does not land) and key[i] (0 when it does not land)
extern "C" void vd_project(const float* pts, int n, const double* P, int H, int W, int depth_from_x, uint8_t* landed, int32_t* u,
                           int32_t* v, uint32_t* key) {
    for (int i = 0; i < n; ++i) {
        int uu = -1, vv = -1;
        uint32_t k = 0;
        landed[i] = vd::project_point(pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], P, H, W, depth_from_x != 0, uu, vv, k) ? 1 : 0;
        u[i] = landed[i] ? uu : -1;
        v[i] = landed[i] ? vv : -1;
        key[i] = landed[i] ? k : 0u;
    }
}

// The whole map of one image on the host: key minimum per pixel, then key_depth
extern "C" void vd_map(const float* pts, int n, const double* P, int H, int W, int flip, int depth_from_x, float* out) {
    uint32_t* keys = reinterpret_cast<uint32_t*>(out);
    for (size_t i = 0; i < (size_t)H * W; ++i) keys[i] = vd::EMPTY_KEY;
    for (int i = 0; i < n; ++i) {
        int uu, vv;
        uint32_t k;
        if (!vd::project_point(pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], P, H, W, depth_from_x != 0, uu, vv, k)) continue;
        uint32_t& slot = keys[(size_t)vv * W + (flip ? W - 1 - uu : uu)];
        if (k < slot) slot = k;
    }
    for (size_t i = 0; i < (size_t)H * W; ++i) out[i] = vd::key_depth(keys[i]);
}
