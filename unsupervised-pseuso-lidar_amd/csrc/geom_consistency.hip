// Depth geometry-consistency term (SC-SfMLearner): mcav_geom_consistency_fwd / _bwd (include/mcav_depth.h).  Per-pixel math: geom_math.h.
//
// Two directions (0: tgt -> ref0 with pose[:,0]; 1: ref0 -> tgt with its inverse), each a pass over the pixels of frame a that projects
// them into frame b and compares the projected depth with b's own depth at the landing point.
//   forward:  one launch, grid (tiles, B, 2).  A workgroup owns a 32 x 32 tile of a (four pixels per thread) and leaves the sum of diff,
//             the number of valid pixels (an integer) and the 12 raw dP sums in the slab; the last workgroup of a (sample, direction) -- a
//             ticket, mcav_common.h's hand-off -- adds its slab entries in float64 in a fixed order; the workgroup that finishes the last
//             of them (a second ticket) forms n_d, E_d and loss_accum += weight * 0.5 (E_0 + E_1).  n_d, sum diff and the dP sums stay on
//             the device, in `saved`.  The tickets are cleared by a memset node in front of the launch: no call depends on an earlier one.
//   backward: memset of the scatter accumulators; the scatter launch (same grid, same per-pixel code) writes d diff / d D_a of each pixel
//             and adds each bilinear tap's w_tap * d diff / d D_samp to its destination in D_b as a 64-bit fixed-point integer (integer
//             adds commute: the sums do not depend on the order of arrival, results are bit-identical from run to run); the combine launch
//             scales both by upstream * weight * 0.5 / n_d, adds them, chains to the disparities and turns the dP sums into d_poses.
// The scatter has two forms with bit-identical results (integer sums): four global 64-bit atomics per pixel, or, with MCAV_GC_LDS_TILE in the
// backward's flags, adds into an LDS copy of b's tile (+ halo) that is flushed with one global atomic per non-zero destination, taps
// outside the halo going straight to global memory.
#include <hip/hip_runtime.h>

#include "geom_math.h"
#include "kernel_timer.h"
#include "block_ops.h"

namespace mcav {

constexpr int GC_THREADS = 256;
constexpr int GC_TW = 32, GC_TH = 32, GC_SUB = 4, GC_ROWS = GC_TH / GC_SUB;      // tile of a; rows GC_ROWS apart per thread
constexpr int GC_HALO = 8, GC_LW = GC_TW + 2 * GC_HALO, GC_LH = GC_TH + 2 * GC_HALO;      // the LDS form's tile of b
constexpr int GC_MAX_B = 4095;                     // samples per launch (grid and ticket capacity)
constexpr int GC_NRED = 13;                        // sum of diff, 12 dP sums
constexpr int GC_RED_LD = GC_THREADS + 8;          // one pad float per 32 threads

struct GCArgs {
    const float *disp_t, *disp_r0, *poses;
    const void* K;
    int B, H, W, ntx, G;                           // G = tiles (workgroups) per (sample, direction)
    unsigned flags;
    int min_valid;
    float weight;
    double* saved;                                 // [4 + 24 B]: n_0, n_1, S_0, S_1, then dP[b][d][12]
    float* loss_accum;
    float* diff_out;                               // [B,2,H,W] or nullptr
    unsigned* tickets;                             // [2B + 1]
    double* slab;                                  // [2B][G][GC_NRED]
    unsigned* slab_n;                              // [2B][G]
    double* dir_s;                                 // [2B]
    double* dir_n;                                 // [2B] (integers)
    long long* acc;                                // [2][B][H*W] fixed-point scatter sums, index = direction that scattered
    float* direct;                                 // [2][B][H*W] d diff / d D_a, index = direction
};

__device__ __forceinline__ float gc_uniform(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// The direction's constants: one thread forms them (geom_math.h: the fused loss kernel's sequence), every wavefront lifts them into
// scalar registers.
__device__ __forceinline__ void gc_prepare(const GCArgs& a, int b, int d, gc::Dir* s_dir, WarpFast& wf, float* Kinv) {
    if (threadIdx.x == 0) {
        double Kd[9];
        if (a.flags & MCAV_WL_K_F64) {
            const double* p = reinterpret_cast<const double*>(a.K) + (size_t)b * 9;
            for (int i = 0; i < 9; ++i) Kd[i] = p[i];
        } else {
            const float* p = reinterpret_cast<const float*>(a.K) + (size_t)b * 9;
            for (int i = 0; i < 9; ++i) Kd[i] = (double)p[i];
        }
        gc::make_dir(Kd, a.poses + (size_t)b * 12, d == 1, *s_dir);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 9; ++i) { wf.Q[i] = gc_uniform(s_dir->wf.Q[i]); Kinv[i] = gc_uniform(s_dir->Kinv[i]); }
#pragma unroll
    for (int i = 0; i < 3; ++i) wf.p3[i] = gc_uniform(s_dir->wf.p3[i]);
}

struct GCTile {
    int x, y0;         // this thread's column and first row
    bool xin;
};
__device__ __forceinline__ GCTile gc_tile(const GCArgs& a) {
    const int tyi = (int)blockIdx.x / a.ntx, txi = (int)blockIdx.x - tyi * a.ntx;
    GCTile t;
    t.x = txi * GC_TW + ((int)threadIdx.x & 31);
    t.y0 = tyi * GC_TH + ((int)threadIdx.x >> 5);
    t.xin = t.x < a.W;
    return t;
}

__global__ __launch_bounds__(GC_THREADS) void geom_consistency_fwd_kernel(GCArgs a) {
    __shared__ gc::Dir s_dir;
    __shared__ float s_red[GC_NRED][GC_RED_LD];
    __shared__ double s_d[4];
    __shared__ unsigned s_cnt[4];
    __shared__ int s_flag;
    const int d = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    const bool in_depth = (a.flags & MCAV_WL_INPUT_DEPTH) != 0;
    WarpFast wf;
    float Kinv[9];
    gc_prepare(a, b, d, &s_dir, wf, Kinv);
    const float* const Da = (d == 0 ? a.disp_t : a.disp_r0) + (size_t)b * plane;
    const float* const Db = (d == 0 ? a.disp_r0 : a.disp_t) + (size_t)b * plane;
    float* const dout = a.diff_out ? a.diff_out + ((size_t)b * 2 + d) * plane : nullptr;
    auto texel = [&](int i) { return gc::depth_of(Db[i], in_depth); };
    const GCTile t = gc_tile(a);
    float acc[GC_NRED];
#pragma unroll
    for (int k = 0; k < GC_NRED; ++k) acc[k] = 0.f;
    unsigned cnt = 0;
#pragma unroll
    for (int k = 0; k < GC_SUB; ++k) {
        const int y = t.y0 + k * GC_ROWS;
        const bool live = t.xin && y < H;
        const int q = live ? y * W + t.x : 0;              // past the image: pixel 0's load, nothing kept
        const float D = gc::depth_of(Da[q], in_depth);
        const gc::Result r = gc::pixel(wf, t.x, y, D, H, W, live, texel);
        const bool v = r.p.valid;
        acc[0] += v ? r.e.diff : 0.f;
        cnt += v ? 1u : 0u;
        float X[3];
        gc::camera_point(Kinv, (float)t.x, (float)y, D, X);
        if (!v) { X[0] = 0.f; X[1] = 0.f; X[2] = 0.f; }    // (an invalid pixel's dc is 0; its X may be NaN)
        apply_dc(r.dc, 1.0f, X, acc + 1);
        if (dout && live) dout[q] = v ? r.e.diff : -1.0f;
    }
    // the workgroup's sums in a fixed order: each value's 256 addends through LDS, 8 lanes take 32 each in float64, three xor-shuffles
#pragma unroll
    for (int k = 0; k < GC_NRED; ++k) s_red[k][tid + (tid >> 5)] = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    const size_t slot = ((size_t)b * 2 + d) * a.G + blockIdx.x;
    {
        const int k = tid >> 3, part = tid & 7;
        double s = 0.0;
        if (k < GC_NRED) {
#pragma unroll
            for (int j = 0; j < 32; ++j) s += (double)s_red[k][part * 33 + j];
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (k < GC_NRED && part == 0) handoff_store(a.slab + slot * GC_NRED + k, s);
        if (tid == GC_THREADS - 1) handoff_store(a.slab_n + slot, (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]));
    }
    const int bd = b * 2 + d;
    if (!handoff_last([&] { return &a.tickets[bd]; }, a.G, &s_flag)) return;
    // the last workgroup of (sample, direction): its slab entries in a fixed order (8 lanes per value, entries part, part + 8, ...)
    {
        const int k = tid >> 3, part = tid & 7;
        const double* sl = a.slab + (size_t)bd * a.G * GC_NRED;
        double s = 0.0;
        if (k < GC_NRED)
            for (int i = part; i < a.G; i += 8) s += handoff_load(sl + (size_t)i * GC_NRED + k);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (k == 0 && part == 0) handoff_store(a.dir_s + bd, s);
        if (k >= 1 && k < GC_NRED && part == 0) a.saved[4 + (size_t)bd * 12 + (k - 1)] = s;      // read by the backward: another launch
        unsigned long long n = 0;
        for (int i = tid; i < a.G; i += GC_THREADS) n += handoff_load(a.slab_n + (size_t)bd * a.G + i);
        const double nn = block_sum<double, GC_THREADS / 64>((double)n, s_d);    // (integers below 2^53: exact in any order)
        if (tid == 0) handoff_store(a.dir_n + bd, nn);
    }
    if (!handoff_last([&] { return &a.tickets[2 * a.B]; }, 2 * a.B, &s_flag)) return;
    // the last (sample, direction): both directions' sums over the samples, in a fixed order
    double ns[2], ss[2];
#pragma unroll
    for (int dd = 0; dd < 2; ++dd) {
        double n = 0.0, s = 0.0;
        for (int i = tid; i < a.B; i += GC_THREADS) {
            n += handoff_load(a.dir_n + i * 2 + dd);
            s += handoff_load(a.dir_s + i * 2 + dd);
        }
        ns[dd] = block_sum<double, GC_THREADS / 64>(n, s_d);
        ss[dd] = block_sum<double, GC_THREADS / 64>(s, s_d);
    }
    if (tid == 0) {
        a.saved[0] = ns[0]; a.saved[1] = ns[1]; a.saved[2] = ss[0]; a.saved[3] = ss[1];
        const double e = 0.5 * (gc::direction_loss(ns[0], ss[0], a.min_valid) + gc::direction_loss(ns[1], ss[1], a.min_valid));
        a.loss_accum[0] += (float)((double)a.weight * e);
    }
}

// The backward's pass over the pixels of a: d diff / d D_a to `direct`, the four taps' contributions to `acc` (fixed point).
template <bool LDS_TILE>
__global__ __launch_bounds__(GC_THREADS) void geom_consistency_scatter_kernel(GCArgs a) {
    __shared__ gc::Dir s_dir;
    __shared__ long long s_tile[LDS_TILE ? GC_LH * GC_LW : 1];
    const int d = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    const bool in_depth = (a.flags & MCAV_WL_INPUT_DEPTH) != 0;
    WarpFast wf;
    float Kinv[9];
    if constexpr (LDS_TILE) {
        for (int i = tid; i < GC_LH * GC_LW; i += GC_THREADS) s_tile[i] = 0;
    }
    gc_prepare(a, b, d, &s_dir, wf, Kinv);                 // (its barrier also covers the tile's zero-fill)
    const float* const Da = (d == 0 ? a.disp_t : a.disp_r0) + (size_t)b * plane;
    const float* const Db = (d == 0 ? a.disp_r0 : a.disp_t) + (size_t)b * plane;
    float* const direct = a.direct + ((size_t)d * a.B + b) * plane;
    long long* const dst = a.acc + ((size_t)d * a.B + b) * plane;
    auto texel = [&](int i) { return gc::depth_of(Db[i], in_depth); };
    const GCTile t = gc_tile(a);
    const int tyi = (int)blockIdx.x / a.ntx, txi = (int)blockIdx.x - tyi * a.ntx;
    const int ox = txi * GC_TW - GC_HALO, oy = tyi * GC_TH - GC_HALO;      // origin of the LDS tile in b
#pragma unroll
    for (int k = 0; k < GC_SUB; ++k) {
        const int y = t.y0 + k * GC_ROWS;
        const bool live = t.xin && y < H;
        const int q = live ? y * W + t.x : 0;
        const float D = gc::depth_of(Da[q], in_depth);
        const gc::Result r = gc::pixel(wf, t.x, y, D, H, W, live, texel);
        if (live) direct[q] = r.dD;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long f = gc::to_fixed(r.tap[j]);
            if (f == 0) continue;                          // (invalid pixel, tap outside the image, or a contribution below 2^-37)
            // r.tap[j] != 0 only for a tap inside the image: 0 <= r.idx[j] < H * W
            if constexpr (LDS_TILE) {
                const int lx = r.p.t.x0 + (j & 1) - ox, ly = r.p.t.y0 + (j >> 1) - oy;
                if ((unsigned)lx < (unsigned)GC_LW && (unsigned)ly < (unsigned)GC_LH) {
                    __hip_atomic_fetch_add(&s_tile[ly * GC_LW + lx], f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    continue;
                }
            }
            __hip_atomic_fetch_add(dst + r.idx[j], f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (LDS_TILE) {
        __syncthreads();
        for (int i = tid; i < GC_LH * GC_LW; i += GC_THREADS) {
            const long long f = s_tile[i];
            if (f == 0) continue;
            const int ly = i / GC_LW, lx = i - ly * GC_LW;
            const int gx = ox + lx, gy = oy + ly;
            if ((unsigned)gx < (unsigned)W && (unsigned)gy < (unsigned)H)      // (always: only taps inside the image were added)
                __hip_atomic_fetch_add(dst + (size_t)gy * W + gx, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// d_disp_t = k_0 direct_0 + k_1 scattered_1,  d_disp_r0 = k_1 direct_1 + k_0 scattered_0,  k_d = upstream * weight * 0.5 / n_d (0 when
// n_d <= min_valid), chained through D = 1 / (10 d + 0.01) unless the inputs are depths; block (0, b, 0) also turns the dP sums into d_poses.
__global__ __launch_bounds__(GC_THREADS) void geom_consistency_combine_kernel(GCArgs a, const float* upstream, float* d_disp_t, float* d_disp_r0,
                                                                               float* d_poses, int accumulate) {
    __shared__ double s_g[2][6];
    const int m = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
    const size_t plane = (size_t)a.H * a.W;
    const bool in_depth = (a.flags & MCAV_WL_INPUT_DEPTH) != 0;
    const double up = (double)(upstream ? upstream[0] : 1.0f) * (double)a.weight;
    const double kd[2] = {up * gc::direction_scale(a.saved[0], a.min_valid), up * gc::direction_scale(a.saved[1], a.min_valid)};
    const bool on[2] = {a.saved[0] > (double)a.min_valid, a.saved[1] > (double)a.min_valid};
    const size_t i = (size_t)blockIdx.x * GC_THREADS + tid;
    if (i < plane) {
        const float kdir = (float)kd[m], ksc = (float)kd[1 - m];
        const float dv = a.direct[((size_t)m * a.B + b) * plane + i];
        const float sv = (float)((double)a.acc[((size_t)(1 - m) * a.B + b) * plane + i] * gc::FIX_INV);
        float g = (on[m] ? kdir * dv : 0.f) + (on[1 - m] ? ksc * sv : 0.f);
        if (!in_depth) {
            const float D = gc::depth_of((m == 0 ? a.disp_t : a.disp_r0)[(size_t)b * plane + i], false);
            g *= -10.0f * D * D;
        }
        float* out = (m == 0 ? d_disp_t : d_disp_r0) + (size_t)b * plane + i;
        *out = accumulate ? *out + g : g;
    }
    if (blockIdx.x != 0 || m != 0) return;
    if (tid < 2) {
        const int d = tid;
        double Kd[9];
        if (a.flags & MCAV_WL_K_F64) {
            const double* p = reinterpret_cast<const double*>(a.K) + (size_t)b * 9;
            for (int k = 0; k < 9; ++k) Kd[k] = p[k];
        } else {
            const float* p = reinterpret_cast<const float*>(a.K) + (size_t)b * 9;
            for (int k = 0; k < 9; ++k) Kd[k] = (double)p[k];
        }
        float Kf[9];
        for (int k = 0; k < 9; ++k) Kf[k] = (float)Kd[k];
        double dP[12];
        for (int k = 0; k < 12; ++k) dP[k] = on[d] ? kd[d] * a.saved[4 + ((size_t)b * 2 + d) * 12 + k] : 0.0;
        pose_grad_from_dP(dP, Kf, a.poses + (size_t)b * 12, d == 1, s_g[d]);
    }
    __syncthreads();
    if (tid < 12) {
        float* out = d_poses + (size_t)b * 12 + tid;
        const float g = tid < 6 ? (float)(s_g[0][tid] + s_g[1][tid]) : 0.f;      // pose[:,1] takes no part
        *out = accumulate ? *out + g : g;
    }
}

struct GCLayout {
    size_t tick_off, slab_off, slab_n_off, dir_s_off, dir_n_off, acc_off, direct_off, total;
    int ntx, G;
};

inline GCLayout gc_layout(int B, int H, int W) {
    GCLayout l;
    l.ntx = (W + GC_TW - 1) / GC_TW;
    l.G = l.ntx * ((H + GC_TH - 1) / GC_TH);
    const size_t plane = (size_t)H * W, bd = 2 * (size_t)B;
    size_t o = 0;
    l.tick_off = o;   o = align_up(o + sizeof(unsigned) * (2 * (size_t)GC_MAX_B + 1), 256);      // a fixed place and size, whatever the shape
    l.slab_off = o;   o = align_up(o + sizeof(double) * bd * l.G * GC_NRED, 256);
    l.slab_n_off = o; o = align_up(o + sizeof(unsigned) * bd * l.G, 256);
    l.dir_s_off = o;  o = align_up(o + sizeof(double) * bd, 256);
    l.dir_n_off = o;  o = align_up(o + sizeof(double) * bd, 256);
    l.acc_off = o;    o = align_up(o + sizeof(long long) * bd * plane, 256);
    l.direct_off = o; o = align_up(o + sizeof(float) * bd * plane, 256);
    l.total = o;
    return l;
}

inline bool gc_shape_ok(int B, int H, int W) {
    return B > 0 && B <= GC_MAX_B && H >= 2 && W >= 2 && (size_t)H * W <= ((size_t)1 << 24);
}

inline GCArgs gc_args(const float* disp_t, const float* disp_r0, const float* poses, const void* K, int B, int H, int W, unsigned flags,
                      int min_valid, float weight, double* saved, void* workspace, const GCLayout& l) {
    char* ws = reinterpret_cast<char*>(workspace);
    GCArgs a = {};
    a.disp_t = disp_t; a.disp_r0 = disp_r0; a.poses = poses; a.K = K;
    a.B = B; a.H = H; a.W = W; a.ntx = l.ntx; a.G = l.G;
    a.flags = flags; a.min_valid = min_valid; a.weight = weight; a.saved = saved;
    a.tickets = reinterpret_cast<unsigned*>(ws + l.tick_off);
    a.slab = reinterpret_cast<double*>(ws + l.slab_off);
    a.slab_n = reinterpret_cast<unsigned*>(ws + l.slab_n_off);
    a.dir_s = reinterpret_cast<double*>(ws + l.dir_s_off);
    a.dir_n = reinterpret_cast<double*>(ws + l.dir_n_off);
    a.acc = reinterpret_cast<long long*>(ws + l.acc_off);
    a.direct = reinterpret_cast<float*>(ws + l.direct_off);
    return a;
}

}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_geom_consistency_workspace_bytes(int B, int H, int W) {
    if (!gc_shape_ok(B, H, W)) return 0;
    return gc_layout(B, H, W).total;
}

MCAV_EXPORT int mcav_geom_consistency_fwd(const float* disp_t, const float* disp_r0, const float* poses, const void* K, int B, int H, int W,
                                          unsigned flags, int min_valid, float weight, double* saved, float* loss_accum, float* diff_out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!disp_t || !disp_r0 || !poses || !K || !saved || !loss_accum || !workspace) return MCAV_E_INVALID;
    if ((flags & ~(MCAV_WL_K_F64 | MCAV_WL_INPUT_DEPTH | MCAV_GC_LDS_TILE)) != 0 || min_valid < 0 || !gc_shape_ok(B, H, W)) return MCAV_E_INVALID;
    const GCLayout l = gc_layout(B, H, W);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    GCArgs a = gc_args(disp_t, disp_r0, poses, K, B, H, W, flags, min_valid, weight, saved, workspace, l);
    a.loss_accum = loss_accum;
    a.diff_out = diff_out;
    if (hipMemsetAsync(a.tickets, 0, sizeof(unsigned) * (2 * (size_t)B + 1), as_stream(stream)) != hipSuccess) return MCAV_E_LAUNCH;
    timed_launch(geom_consistency_fwd_kernel, dim3(l.G, B, 2), dim3(GC_THREADS), 0, as_stream(stream), a);
    return launch_status();
}

MCAV_EXPORT int mcav_geom_consistency_bwd(const float* disp_t, const float* disp_r0, const float* poses, const void* K, int B, int H, int W,
                                          unsigned flags, int min_valid, float weight, const double* saved, const float* upstream,
                                          float* d_disp_t, float* d_disp_r0, float* d_poses, int accumulate, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    if (!disp_t || !disp_r0 || !poses || !K || !saved || !d_disp_t || !d_disp_r0 || !d_poses || !workspace) return MCAV_E_INVALID;
    if ((flags & ~(MCAV_WL_K_F64 | MCAV_WL_INPUT_DEPTH | MCAV_GC_LDS_TILE)) != 0 || min_valid < 0 || !gc_shape_ok(B, H, W)) return MCAV_E_INVALID;
    const GCLayout l = gc_layout(B, H, W);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    GCArgs a = gc_args(disp_t, disp_r0, poses, K, B, H, W, flags, min_valid, weight, const_cast<double*>(saved), workspace, l);
    const size_t plane = (size_t)H * W;
    if (hipMemsetAsync(a.acc, 0, sizeof(long long) * 2 * (size_t)B * plane, as_stream(stream)) != hipSuccess) return MCAV_E_LAUNCH;
    if (flags & MCAV_GC_LDS_TILE) timed_launch(geom_consistency_scatter_kernel<true>, dim3(l.G, B, 2), dim3(GC_THREADS), 0, as_stream(stream), a);
    else timed_launch(geom_consistency_scatter_kernel<false>, dim3(l.G, B, 2), dim3(GC_THREADS), 0, as_stream(stream), a);
    if (launch_status() != MCAV_OK) return MCAV_E_LAUNCH;
    timed_launch(geom_consistency_combine_kernel, dim3((unsigned)((plane + GC_THREADS - 1) / GC_THREADS), B, 2), dim3(GC_THREADS), 0,
                 as_stream(stream), a, upstream, d_disp_t, d_disp_r0, d_poses, accumulate);
    return launch_status();
}
