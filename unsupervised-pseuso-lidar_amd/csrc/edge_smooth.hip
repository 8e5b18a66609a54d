// Edge-aware smoothness on mean-normalised disparity (monodepth2's get_smooth_loss(disp / (mean_disp + 1e-7), color)), one scale per
// launch: mcav_edge_smooth_fwd / mcav_edge_smooth_bwd (include/mcav_depth.h).  Per-pixel math: edge_math.h.
//
// The mean normalisation makes every pixel's gradient depend on two per-sample sums, m_b (mean disparity) and R_b (the weighted |delta d|
// sum), so the term is two launches:
//   forward:  every workgroup sums d and its pixels' parts of R over a tile of ES_TILE pixels and leaves the two sums in the slab; the last
//             workgroup of a sample (a ticket) adds that sample's slab entries in float64 in a fixed order, writes m_b, R_b to the caller's
//             saved buffer and E_b to the per-sample slot; the workgroup that finishes the last sample (a second ticket) adds the E_b in a
//             fixed order and does loss_accum += weight * sum.  The hand-off is mcav_common.h's protocol (tests/test_edge_smooth_cpu.py
//             reads it in the ISA); no workgroup waits for another, and the tickets are left at zero.
//   backward: one pass over the pixels with the saved sums: d_disp = upstream * weight * (stencil / (m_b + eps) - R_b / ((m_b + eps)^2 h w)).
// The image taps of a coarse scale are box averages of the full-resolution image formed on the fly (f = H / h; f = 1 reads the image).
#include <hip/hip_runtime.h>

#include "edge_math.h"
#include "kernel_timer.h"
#include "block_ops.h"

namespace mcav {

constexpr int ES_THREADS = 256;
constexpr int ES_PPT = 4;                              // pixels per thread, ES_THREADS apart (coalesced)
constexpr int ES_TILE = ES_THREADS * ES_PPT;           // pixels per workgroup
constexpr int ES_MAX_B = 4095;                         // samples per launch (ticket capacity)

struct ESArgs {
    const float* disp;         // [B,1,h,w]
    const float* img;          // [B,3,H,W]
    int B, H, W, h, w, f;
    int G;                     // workgroups per sample
    float weight, cx, cy;
    double* saved;             // [2B]: m_b, then R_b
    float* loss_accum;         // [1], += weight * E
    unsigned* tickets;         // [ES_MAX_B + 1], zero between launches
    double* slab_m;            // [B][G]
    double* slab_r;            // [B][G]
    double* sample_e;          // [B]
};

// UNIT: f == 1, the image taps are plain loads
template <bool UNIT>
__global__ __launch_bounds__(ES_THREADS) void edge_smooth_fwd_kernel(ESArgs a) {
    __shared__ double s_red[4];
    __shared__ int s_flag;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int h = a.h, w = a.w, n = h * w, f = UNIT ? 1 : a.f;
    const size_t hw_full = (size_t)a.H * a.W;
    const float* dp = a.disp + (size_t)b * n;
    const float* ip = a.img + (size_t)b * 3 * hw_full;
    auto D = [&](int y, int x) { return dp[(size_t)y * w + x]; };
    auto C = [&](int y, int x) { return es::rgb_at(ip, hw_full, a.W, f, y, x); };
    float sd = 0.f, sr = 0.f;
#pragma unroll
    for (int k = 0; k < ES_PPT; ++k) {
        const int p = blockIdx.x * ES_TILE + k * ES_THREADS + tid;
        const int q = p < n ? p : n - 1;              // past the end: a real pixel's loads, its sums dropped (no branch around the loads)
        const int y = q / w, x = q - y * w;
        const float v = es::pixel_loss(D, C, y, x, h, w, a.cx, a.cy);
        const float dq = dp[q];
        sd += p < n ? dq : 0.f;
        sr += p < n ? v : 0.f;
    }
    const double bm = block_sum<double, ES_THREADS / 64>((double)sd, s_red);
    const double br = block_sum<double, ES_THREADS / 64>((double)sr, s_red);
    const size_t slot = (size_t)b * a.G + blockIdx.x;
    if (tid == 0) {
        handoff_store(a.slab_m + slot, bm);
        handoff_store(a.slab_r + slot, br);
    }
    if (!handoff_last([&] { return &a.tickets[b]; }, a.G, &s_flag)) return;
    // the last workgroup of sample b: its slab entries in a fixed order (thread t takes entries t, t + 256, ...)
    double tm = 0.0, tr = 0.0;
    for (int i = tid; i < a.G; i += ES_THREADS) {
        tm += handoff_load(a.slab_m + (size_t)b * a.G + i);
        tr += handoff_load(a.slab_r + (size_t)b * a.G + i);
    }
    const double m = block_sum<double, ES_THREADS / 64>(tm, s_red) / (double)n;
    const double R = block_sum<double, ES_THREADS / 64>(tr, s_red);
    if (tid == 0) {
        handoff_store(a.saved + b, m);
        handoff_store(a.saved + a.B + b, R);
        handoff_store(a.sample_e + b, es::sample_loss(m, R));
        handoff_store(&a.tickets[b], 0u);
    }
    if (!handoff_last([&] { return &a.tickets[a.B]; }, a.B, &s_flag)) return;
    // the last sample: every E_b, added in a fixed order (thread t takes samples t, t + 256, ...)
    double e = 0.0;
    for (int i = tid; i < a.B; i += ES_THREADS) e += handoff_load(a.sample_e + i);
    e = block_sum<double, ES_THREADS / 64>(e, s_red);
    if (tid == 0) {
        a.loss_accum[0] += (float)((double)a.weight * e);
        handoff_store(&a.tickets[a.B], 0u);
    }
}

template <bool UNIT>
__global__ __launch_bounds__(ES_THREADS) void edge_smooth_bwd_kernel(ESArgs a, const float* upstream, float* d_disp, int accumulate) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int h = a.h, w = a.w, n = h * w, f = UNIT ? 1 : a.f;
    const size_t hw_full = (size_t)a.H * a.W;
    const float* dp = a.disp + (size_t)b * n;
    const float* ip = a.img + (size_t)b * 3 * hw_full;
    auto D = [&](int y, int x) { return dp[(size_t)y * w + x]; };
    auto C = [&](int y, int x) { return es::rgb_at(ip, hw_full, a.W, f, y, x); };
    float inv, kk;
    es::grad_factors(a.saved[b], a.saved[a.B + b], h, w, inv, kk);
    const float g = (upstream ? upstream[0] : 1.0f) * a.weight;
    float v[ES_PPT];
#pragma unroll
    for (int k = 0; k < ES_PPT; ++k) {                 // every pixel's loads before the first store (to the compiler a store may alias them)
        const int p = blockIdx.x * ES_TILE + k * ES_THREADS + tid;
        const int q = p < n ? p : n - 1;
        const int y = q / w, x = q - y * w;
        v[k] = g * es::pixel_grad(es::pixel_stencil(D, C, y, x, h, w, a.cx, a.cy), inv, kk);
    }
    float* out = d_disp + (size_t)b * n;
#pragma unroll
    for (int k = 0; k < ES_PPT; ++k) {
        const int p = blockIdx.x * ES_TILE + k * ES_THREADS + tid;
        if (p < n) out[p] = accumulate ? out[p] + v[k] : v[k];
    }
}

struct ESLayout {
    size_t tick_off, slab_m_off, slab_r_off, e_off, total;
    int G;
};

// The tickets sit at a fixed place and size, whatever the shape: a cached workspace serves every scale, and a ticket word that another
// shape's slab had used would not be zero.
inline ESLayout es_layout(int B, int h, int w) {
    ESLayout l;
    l.G = (int)(((size_t)h * w + ES_TILE - 1) / ES_TILE);
    size_t o = 0;
    l.tick_off = o;   o = align_up(o + sizeof(unsigned) * ((size_t)ES_MAX_B + 1), 256);
    l.slab_m_off = o; o = align_up(o + sizeof(double) * (size_t)B * l.G, 256);
    l.slab_r_off = o; o = align_up(o + sizeof(double) * (size_t)B * l.G, 256);
    l.e_off = o;      o = align_up(o + sizeof(double) * (size_t)B, 256);
    l.total = o;
    return l;
}

// shape checks shared by both entries: -> f, or 0 when the shape is rejected
inline int es_factor(int B, int H, int W, int h, int w) {
    if (B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || B > ES_MAX_B) return 0;
    if (H % h != 0 || W % w != 0 || H / h != W / w) return 0;
    if ((size_t)h * w > (size_t)0x7fffffff - ES_TILE) return 0;
    return H / h;
}

inline ESArgs es_args(const float* disp, const float* img, int B, int H, int W, int h, int w, int f, float weight, double* saved) {
    ESArgs a = {};
    a.disp = disp; a.img = img;
    a.B = B; a.H = H; a.W = W; a.h = h; a.w = w; a.f = f;
    a.G = (int)(((size_t)h * w + ES_TILE - 1) / ES_TILE);
    a.weight = weight;
    es::pair_scales(B, h, w, a.cx, a.cy);
    a.saved = saved;
    return a;
}

}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_edge_smooth_workspace_bytes(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    return es_layout(B, h, w).total;
}

MCAV_EXPORT int mcav_edge_smooth_fwd(const float* disp, const float* img, int B, int H, int W, int h, int w, float weight, double* saved,
                                     float* loss_accum, void* workspace, size_t workspace_bytes, void* stream) {
    if (!disp || !img || !saved || !loss_accum || !workspace) return MCAV_E_INVALID;
    const int f = es_factor(B, H, W, h, w);
    if (f == 0) return MCAV_E_INVALID;
    const ESLayout l = es_layout(B, h, w);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    ESArgs a = es_args(disp, img, B, H, W, h, w, f, weight, saved);
    a.loss_accum = loss_accum;
    a.tickets = reinterpret_cast<unsigned*>(ws + l.tick_off);
    a.slab_m = reinterpret_cast<double*>(ws + l.slab_m_off);
    a.slab_r = reinterpret_cast<double*>(ws + l.slab_r_off);
    a.sample_e = reinterpret_cast<double*>(ws + l.e_off);
    if (f == 1) timed_launch(edge_smooth_fwd_kernel<true>, dim3(a.G, B), dim3(ES_THREADS), 0, as_stream(stream), a);
    else timed_launch(edge_smooth_fwd_kernel<false>, dim3(a.G, B), dim3(ES_THREADS), 0, as_stream(stream), a);
    return launch_status();
}

MCAV_EXPORT int mcav_edge_smooth_bwd(const float* disp, const float* img, int B, int H, int W, int h, int w, float weight,
                                     const double* saved, const float* upstream, float* d_disp, int accumulate, void* stream) {
    if (!disp || !img || !saved || !d_disp) return MCAV_E_INVALID;
    const int f = es_factor(B, H, W, h, w);
    if (f == 0) return MCAV_E_INVALID;
    ESArgs a = es_args(disp, img, B, H, W, h, w, f, weight, const_cast<double*>(saved));
    if (f == 1) timed_launch(edge_smooth_bwd_kernel<true>, dim3(a.G, B), dim3(ES_THREADS), 0, as_stream(stream), a, upstream, d_disp, accumulate);
    else timed_launch(edge_smooth_bwd_kernel<false>, dim3(a.G, B), dim3(ES_THREADS), 0, as_stream(stream), a, upstream, d_disp, accumulate);
    return launch_status();
}
