// Velodyne scans -> sparse depth maps, KITTI Eigen ground truth (monodepth2 generate_depth_map): mcav_velo_depth_map (include/mcav_depth.h).
// Definition: tests/velo_ref.py.  Per-point math: velo_math.h.
//
// Launches, all on the caller's stream, no host synchronisation, allocation or copy (the call can be captured in a hipGraph):
//   init      every element of out = EMPTY_KEY (the keys live in out itself: no workspace)
//   scatter   one pass over each image's points (16 B each, consecutive lanes on consecutive points): project, and for a point that lands,
//             one integer atomicMin of its order-preserving depth key on its pixel.  ~15 k of an HDL-64E scan's ~120 k points land, on
//             ~470 k pixels, so the atomics rarely meet; integer minima are exact and order-independent: the map is bit-reproducible.
//   finalize  every element: key -> float32 depth, +0.0 for EMPTY_KEY (no point, and all of the padding) and for a negative minimum.
// No float atomics anywhere.
#include <hip/hip_runtime.h>

#include "kernel_timer.h"
#include "mcav_common.h"
#include "velo_math.h"

namespace mcav {

constexpr int VD_THREADS = 256;
constexpr int VD_PPT = 4;                              // scatter: points per thread, VD_THREADS apart
constexpr int VD_TILE = VD_THREADS * VD_PPT;           // points per workgroup and step
constexpr int VD_MAX_SCATTER_GROUPS = 4096;            // per image; larger scans loop
constexpr int VD_EPT = 4;                              // init / finalize: elements per thread, VD_THREADS apart
constexpr int VD_MAX_MAP_GROUPS = 65536;               // larger maps loop

struct VDArgs {
    const float* points;       // [N,4]
    const long long* offsets;  // [B+1]
    const double* P;           // [B,12]
    const int* sizes;          // [B,2]
    const unsigned char* flip; // [B] or null
    int Hg, Wg;
    long long max_points;
    int flags;
    uint32_t* keys;            // out, [B,Hg,Wg]
};

__global__ __launch_bounds__(VD_THREADS) void velo_init_kernel(uint32_t* keys, size_t total) {
    const size_t step = (size_t)gridDim.x * (VD_THREADS * VD_EPT);
    for (size_t base = (size_t)blockIdx.x * (VD_THREADS * VD_EPT) + threadIdx.x; base < total; base += step) {
#pragma unroll
        for (int k = 0; k < VD_EPT; ++k) {
            const size_t i = base + (size_t)k * VD_THREADS;
            if (i < total) keys[i] = vd::EMPTY_KEY;
        }
    }
}

__global__ __launch_bounds__(VD_THREADS) void velo_scatter_kernel(VDArgs a) {
    const int b = blockIdx.y;
    const long long first = max(a.offsets[b], 0ll);
    const long long n = min(max(a.offsets[b + 1] - first, 0ll), a.max_points);
    const int Hb = min(max(a.sizes[2 * b], 0), a.Hg), Wb = min(max(a.sizes[2 * b + 1], 0), a.Wg);
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = a.P[(size_t)b * 12 + k];
    const bool flip = a.flip && a.flip[b];
    const bool from_x = (a.flags & MCAV_VELO_DEPTH_FROM_X) != 0;
    const float* pts = a.points + (size_t)first * 4;
    uint32_t* kb = a.keys + (size_t)b * a.Hg * a.Wg;
    const long long step = (long long)gridDim.x * VD_TILE;
    for (long long base = (long long)blockIdx.x * VD_TILE + threadIdx.x; base < n; base += step) {
        float x[VD_PPT], y[VD_PPT], z[VD_PPT];
#pragma unroll
        for (int k = 0; k < VD_PPT; ++k) {             // all loads first
            const long long i = base + (long long)k * VD_THREADS;
            const float* p = pts + (size_t)(i < n ? i : 0) * 4;
            x[k] = i < n ? p[0] : -1.0f;                // (-1 is dropped by the x test)
            y[k] = p[1];
            z[k] = p[2];
        }
#pragma unroll
        for (int k = 0; k < VD_PPT; ++k) {
            int u, v;
            uint32_t key;
            if (vd::project_point(x[k], y[k], z[k], P, Hb, Wb, from_x, u, v, key)) {
                const int col = flip ? Wb - 1 - u : u;
                atomicMin(&kb[(size_t)v * a.Wg + col], key);
            }
        }
    }
}

__global__ __launch_bounds__(VD_THREADS) void velo_finalize_kernel(uint32_t* keys, size_t total) {
    float* out = reinterpret_cast<float*>(keys);
    const size_t step = (size_t)gridDim.x * (VD_THREADS * VD_EPT);
    for (size_t base = (size_t)blockIdx.x * (VD_THREADS * VD_EPT) + threadIdx.x; base < total; base += step) {
#pragma unroll
        for (int k = 0; k < VD_EPT; ++k) {
            const size_t i = base + (size_t)k * VD_THREADS;
            if (i < total) out[i] = vd::key_depth(keys[i]);
        }
    }
}

}  // namespace mcav

using namespace mcav;

MCAV_EXPORT int mcav_velo_depth_map(const float* points, const long long* offsets, const double* P, const int* sizes,
                                    const unsigned char* flip, int B, int Hg, int Wg, long long max_points, int flags, float* out,
                                    void* stream) {
    if (!points || !offsets || !P || !sizes || !out) return MCAV_E_INVALID;
    if (B <= 0 || Hg <= 0 || Wg <= 0 || max_points < 0) return MCAV_E_INVALID;
    if (B > 65535) return MCAV_E_INVALID;                                          // grid y
    if (flags & ~MCAV_VELO_DEPTH_FROM_X) return MCAV_E_INVALID;
    if ((unsigned long long)Hg * (unsigned long long)Wg > (1ull << 62) / 4 / (unsigned long long)B) return MCAV_E_INVALID;   // 64-bit byte offsets
    const size_t total = (size_t)B * Hg * Wg;
    VDArgs a = {};
    a.points = points; a.offsets = offsets; a.P = P; a.sizes = sizes; a.flip = flip;
    a.Hg = Hg; a.Wg = Wg; a.max_points = max_points; a.flags = flags;
    a.keys = reinterpret_cast<uint32_t*>(out);
    hipStream_t s = as_stream(stream);
    const size_t mg = (total + VD_THREADS * VD_EPT - 1) / (VD_THREADS * VD_EPT);
    const int map_groups = (int)(mg < (size_t)VD_MAX_MAP_GROUPS ? mg : (size_t)VD_MAX_MAP_GROUPS);
    const long long sg = (max_points + VD_TILE - 1) / VD_TILE;
    const int scatter_groups = (int)(sg < VD_MAX_SCATTER_GROUPS ? (sg > 0 ? sg : 1) : VD_MAX_SCATTER_GROUPS);
    timed_launch(velo_init_kernel, dim3(map_groups), dim3(VD_THREADS), 0, s, a.keys, total);
    timed_launch(velo_scatter_kernel, dim3(scatter_groups, B), dim3(VD_THREADS), 0, s, a);
    timed_launch(velo_finalize_kernel, dim3(map_groups), dim3(VD_THREADS), 0, s, a.keys, total);
    return launch_status();
}
