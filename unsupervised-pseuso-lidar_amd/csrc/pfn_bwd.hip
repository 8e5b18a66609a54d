// The backward of pillars -> pillar features -> BEV pseudo-image (include/mcav_depth.h: mcav_pillar_pseudo_image_bwd; the definition is
// tests/pfn_bwd_ref.py, the arithmetic csrc/pfn_bwd_math.h): from the canvas gradient (and / or a gradient of the feature rows) to the
// gradients of the weight, the bias, the padding bias and, when asked for, the voxels.  Nothing of the forward is kept: the layer is
// recomputed with pfn_math.h's fmaf chain, so the slot that won a channel's maximum is the forward's.
//   A workgroup owns chunks of BWD_CHUNK consecutive rows, chunk i going to workgroup i % grid on a grid that depends on the capacity
//   alone.  It first stages the chunk's upstream gradient in LDS.  Rows are in ascending (b, iy, ix) order, so with the lane indexing the
//   row a wavefront's loads of one channel of an NCHW canvas gradient fall into the few cache lines of a canvas row, where one lane per
//   channel would touch 64 lines a pillar; NHWC is one run of c_out floats a row.  Then a wavefront takes every fourth row of the chunk:
//   the pillar's used slots go through LDS as in the forward, one lane per channel (two at c_out > 64) finds the winner, adds its terms
//   of the three sums to float64 accumulators in registers and leaves (g, slot) in LDS; for d_voxels the lanes turn to the pillar's
//   elements (k, c) and walk the channels in ascending order.  The next row's slots are fetched into registers while this one is
//   computed.  d_voxels behind the last pillar is one run of zeros that all workgroups fill in 16-byte stores.
//   At the end the workgroup adds its wavefronts' accumulators in wavefront order and writes them to its column of the slab
//   [c_out (C + 2)][grid]; a second launch, one wavefront per sum, adds a slab row (lane l takes columns l, l + 64, ..., then the
//   butterfly) and rounds once.  The assignment of rows to accumulators is fixed, so two runs give the same bytes.
// No atomics, nothing returns to the host, no allocation: the call can be captured.  2 launches.
#include "block_ops.h"
#include "pfn_bwd_math.h"

namespace mcav {
namespace pfn {

constexpr int BWD_THREADS = 256;
constexpr int BWD_WAVES = BWD_THREADS / 64;
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int BWD_RED = 2 * (BWD_WAVES - 1) * 64;        // floats of LDS under the cross-wavefront sum: (WAVES - 1) x 64 doubles

struct BwdArgs {
    const float* voxels;
    const int* coords;
    const int* num_points;
    const int* pillar_offsets;
    const float* weight;
    const float* bias;
    const float* bias_pad;
    const float* d_canvas;
    const float* d_features;
    float* d_voxels;
    double* slab;
    long long capacity;
    int B, N, nx, ny, c_out;
    int stage;                                   // floats of LDS a wavefront stages a pillar in
};

__device__ __forceinline__ void bwd_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

inline size_t bwd_lds_floats(int c_out, int C, int stage) {
    return (size_t)BWD_RED + (size_t)BWD_CHUNK * (c_out + 1) + (size_t)c_out * C + (size_t)BWD_WAVES * (stage + 2 * c_out);
}

template <int C, int CPL, bool NHWC>
__global__ __launch_bounds__(BWD_THREADS) void pfn_bwd_kernel(const BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c_out = a.c_out, pitch = c_out + 1;            // a row of the staged gradient: odd, so 64 rows of one channel spread over the banks
    double* red = reinterpret_cast<double*>(lds);
    float* gbuf = lds + BWD_RED;                              // [BWD_CHUNK][pitch]
    float* wts = gbuf + BWD_CHUNK * pitch;                    // [c_out][C]
    float* stage = wts + c_out * C + wave * (a.stage + 2 * c_out);
    float* gw = stage + a.stage;                              // [c_out] g of the wavefront's pillar
    int* kw = reinterpret_cast<int*>(gw + c_out);             // [c_out] win_slot
    for (int e = threadIdx.x; e < c_out * C; e += BWD_THREADS) wts[e] = a.weight[e];

    float w[CPL][C], bias[CPL], pad[CPL];
    int ch[CPL];
    bool live[CPL];
    double dW[CPL][C], dB[CPL], dP[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        ch[j] = lane + 64 * j;
        live[j] = ch[j] < c_out;
        const int src = live[j] ? ch[j] : c_out - 1;
#pragma unroll
        for (int c = 0; c < C; ++c) { w[j][c] = a.weight[src * C + c]; dW[j][c] = 0.0; }
        bias[j] = a.bias[src];
        pad[j] = a.bias_pad[src];
        dB[j] = 0.0;
        dP[j] = 0.0;
    }
    const long long P = live_pillars(a.pillar_offsets, a.B, a.capacity);
    const int NC = a.N * C;
    // the wavefront's next row on its way in: its used slots as floats lane, lane + 64, ... (N * C <= 64 * C), fetched while the row
    // before it is computed
    float block[C];
    int n_next = 0;
    auto fetch = [&](long long r) {
        n_next = __builtin_amdgcn_readfirstlane(used_slots(a.num_points[r], a.N));
        const float* src = a.voxels + (size_t)r * (size_t)NC;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int f = lane + 64 * j;
            block[j] = f < n_next * C ? src[f] : 0.0f;
        }
    };

    for (long long r0 = (long long)blockIdx.x * BWD_CHUNK; r0 < P; r0 += (long long)gridDim.x * BWD_CHUNK) {
        if (r0 + wave < P) fetch(r0 + wave);                  // in flight under the staging of the gradient
        __syncthreads();                                      // the chunk before has been read (and wts written)
        if (a.d_canvas) {
            if constexpr (NHWC) {
                for (int e = threadIdx.x; e < BWD_CHUNK * c_out; e += BWD_THREADS) {
                    const int i = e / c_out, o = e - i * c_out;
                    const long long r = r0 + i;
                    float v = 0.0f;
                    if (r < P && cell_inside(a.coords, r, a.B, a.ny, a.nx))
                        v = a.d_canvas[canvas_index(true, a.coords[4 * r], o, a.coords[4 * r + 2], a.coords[4 * r + 3], c_out, a.ny, a.nx)];
                    gbuf[i * pitch + o] = v;
                }
            } else {
                const long long r = r0 + lane;                // the lane's row; its wavefront takes channels wave, wave + WAVES, ...
                const bool in = r < P && cell_inside(a.coords, r, a.B, a.ny, a.nx);
                const size_t plane = (size_t)a.ny * (size_t)a.nx;
                const size_t at = in ? canvas_index(false, a.coords[4 * r], 0, a.coords[4 * r + 2], a.coords[4 * r + 3], c_out, a.ny, a.nx) : 0;
                for (int o = wave; o < c_out; o += BWD_WAVES) gbuf[lane * pitch + o] = in ? a.d_canvas[at + (size_t)o * plane] : 0.0f;
            }
        }
        __syncthreads();
        for (int i = wave; i < BWD_CHUNK; i += BWD_WAVES) {
            const long long r = r0 + i;                       // the same in every lane
            if (r >= P) break;
            float* out = a.d_voxels ? a.d_voxels + (size_t)r * (size_t)NC : nullptr;
            const int n = n_next;
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const int f = lane + 64 * j;
                if (f < n * C) stage[f] = block[j];
            }
            bwd_wave_lds_sync();
            if (i + BWD_WAVES < BWD_CHUNK && r + BWD_WAVES < P) fetch(r + BWD_WAVES);
            Winner win[CPL];
#pragma unroll
            for (int j = 0; j < CPL; ++j) win[j] = win_start(n < a.N, pad[j]);
#pragma unroll 2
            for (int k = 0; k < n; ++k) {
                float x[C];
#pragma unroll
                for (int c = 0; c < C; ++c) x[c] = stage[k * C + c];
#pragma unroll
                for (int j = 0; j < CPL; ++j) win_join(win[j], act(pre(x, w[j], C, bias[j])), k);
            }
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                if (!live[j]) continue;
                const float part = a.d_canvas ? gbuf[i * pitch + ch[j]] : 0.0f;
                const float g = upstream(part, a.d_features != nullptr, a.d_features ? a.d_features[(size_t)r * (size_t)c_out + ch[j]] : 0.0f);
                const int slot = win_slot(win[j]);
                if (slot >= 0) {                              // slot < n: its row is in the stage
                    dB[j] += (double)g;
#pragma unroll
                    for (int c = 0; c < C; ++c) dW[j][c] += (double)g * (double)stage[slot * C + c];
                } else if (slot == PADDING) {
                    dP[j] += (double)g;
                }
                if (out) {
                    gw[ch[j]] = g;
                    kw[ch[j]] = slot;
                }
            }
            if (out) {
                bwd_wave_lds_sync();
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const int e = lane + 64 * j;
                    if (e >= NC) continue;
                    float v = 0.0f;
                    if (64 * j < n * C) {                     // the same in every lane: elements of unused slots get no channel
                        const int k = e / C, c = e - k * C;
                        v = d_voxel(gw, kw, wts, c_out, C, k, c);
                    }
                    out[e] = v;
                }
            }
            bwd_wave_lds_sync();                              // the stage, gw and kw are free again
        }
    }
    // ---- d_voxels behind the last pillar: one run of zeros up to the capacity, in 16-byte stores between its unaligned ends
    if (a.d_voxels) {
        const size_t begin = (size_t)P * (size_t)NC, end = (size_t)a.capacity * (size_t)NC;
        const size_t past = ((reinterpret_cast<uintptr_t>(a.d_voxels) >> 2) + begin) & 3;      // floats behind a 16-byte boundary
        const size_t body = begin + (past ? 4 - past : 0) < end ? begin + (past ? 4 - past : 0) : end;
        const size_t groups = (end - body) / 4, tail = body + 4 * groups;
        const size_t t = (size_t)blockIdx.x * BWD_THREADS + threadIdx.x, threads = (size_t)gridDim.x * BWD_THREADS;
        if (t < body - begin) a.d_voxels[begin + t] = 0.0f;
        f32x4* wide = reinterpret_cast<f32x4*>(a.d_voxels + body);
        for (size_t g = t; g < groups; g += threads) wide[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (t < end - tail) a.d_voxels[tail + t] = 0.0f;
    }
    // ---- the workgroup's sums: wavefront 0's accumulators, then 1's, 2's, 3's, into column blockIdx.x of the slab
    const int S = bwd_sums(C);
    auto leave = [&](double v, int j, int q) {
        __syncthreads();
        if (wave > 0) red[(wave - 1) * 64 + lane] = v;
        __syncthreads();
        if (wave == 0 && live[j]) {
#pragma unroll
            for (int u = 0; u < BWD_WAVES - 1; ++u) v += red[u * 64 + lane];
            a.slab[((size_t)ch[j] * S + q) * gridDim.x + blockIdx.x] = v;
        }
    };
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
#pragma unroll
        for (int c = 0; c < C; ++c) leave(dW[j][c], j, c);
        leave(dB[j], j, C);
        leave(dP[j], j, C + 1);
    }
}

// one wavefront per sum: the slab's row in a fixed order, rounded once
__global__ __launch_bounds__(BWD_THREADS) void pfn_bwd_reduce_kernel(const double* slab, int G, int c_out, int C, float* d_weight, float* d_bias,
                                                                      float* d_bias_pad) {
    const int lane = threadIdx.x & 63, S = bwd_sums(C);
    const int i = blockIdx.x * BWD_WAVES + (int)(threadIdx.x >> 6);
    if (i >= c_out * S) return;
    const double* row = slab + (size_t)i * G;
    double v = 0.0;
    for (int g = lane; g < G; g += 64) v += row[g];
    v = wave_sum(v);
    if (lane != 0) return;
    const int o = i / S, q = i - o * S;
    if (q < C) d_weight[o * C + q] = (float)v;
    else if (q == C) d_bias[o] = (float)v;
    else d_bias_pad[o] = (float)v;
}

template <int C, int CPL>
int bwd_launch(const BwdArgs& a, bool nhwc, int G, float* d_weight, float* d_bias, float* d_bias_pad, hipStream_t s) {
    const size_t lds = sizeof(float) * bwd_lds_floats(a.c_out, C, a.stage);
    if (nhwc) pfn_bwd_kernel<C, CPL, true><<<G, BWD_THREADS, lds, s>>>(a);
    else pfn_bwd_kernel<C, CPL, false><<<G, BWD_THREADS, lds, s>>>(a);
    const int sums = a.c_out * bwd_sums(C);
    pfn_bwd_reduce_kernel<<<(sums + BWD_WAVES - 1) / BWD_WAVES, BWD_THREADS, 0, s>>>(a.slab, G, a.c_out, C, d_weight, d_bias, d_bias_pad);
    return launch_status();
}

inline bool bwd_sizes_ok(long long capacity, int columns, int c_out) { return capacity >= 0 && columns_ok(columns) && c_out_ok(c_out); }

}  // namespace pfn
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_pillar_pseudo_image_bwd_workspace_bytes(long long capacity, int columns, int c_out) {
    if (!pfn::bwd_sizes_ok(capacity, columns, c_out)) return 0;
    return align_up(sizeof(double) * (size_t)c_out * pfn::bwd_sums(columns) * pfn::bwd_grid(capacity), 256);
}

MCAV_EXPORT int mcav_pillar_pseudo_image_bwd(const float* voxels, const int* coords, const int* num_points, const int* pillar_offsets, int B,
                                             long long capacity, int max_points, int columns, int nx, int ny, const float* weight,
                                             const float* bias, const float* bias_pad, int c_out, int flags, const float* d_canvas,
                                             const float* d_features, float* d_weight, float* d_bias, float* d_bias_pad, float* d_voxels,
                                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!voxels || !coords || !num_points || !pillar_offsets || !weight || !bias || !bias_pad || (!d_canvas && !d_features)) return MCAV_E_INVALID;
    if (!d_weight || !d_bias || !d_bias_pad || !workspace) return MCAV_E_INVALID;
    if (B <= 0 || B > 65535 || capacity < 0 || nx < 1 || ny < 1 || max_points < 1 || max_points > pfn::MAX_POINTS) return MCAV_E_INVALID;
    if ((unsigned long long)B * (unsigned long long)ny * (unsigned long long)nx > 0x7fffffffull) return MCAV_E_INVALID;
    if (!pfn::columns_ok(columns) || !pfn::c_out_ok(c_out) || (flags & ~MCAV_PFN_NHWC)) return MCAV_E_INVALID;
    uintptr_t bits = 0;
    for (const void* p : {(const void*)voxels, (const void*)coords, (const void*)num_points, (const void*)pillar_offsets, (const void*)weight,
                          (const void*)bias, (const void*)bias_pad, (const void*)d_canvas, (const void*)d_features, (const void*)d_weight,
                          (const void*)d_bias, (const void*)d_bias_pad, (const void*)d_voxels})
        bits |= reinterpret_cast<uintptr_t>(p);
    if ((bits & 3) || (reinterpret_cast<uintptr_t>(workspace) & 7)) return MCAV_E_INVALID;
    if (workspace_bytes < mcav_pillar_pseudo_image_bwd_workspace_bytes(capacity, columns, c_out)) return MCAV_E_WORKSPACE;
    pfn::BwdArgs a{voxels, coords, num_points, pillar_offsets, weight, bias, bias_pad, d_canvas, d_features, d_voxels,
                   reinterpret_cast<double*>(workspace), capacity, B, max_points, nx, ny, c_out, (max_points * columns + 3) & ~3};
    const int G = pfn::bwd_grid(capacity);
    const bool nhwc = (flags & MCAV_PFN_NHWC) != 0, two = c_out > 64;
    hipStream_t s = as_stream(stream);
    if (columns == 4) return two ? pfn::bwd_launch<4, 2>(a, nhwc, G, d_weight, d_bias, d_bias_pad, s) : pfn::bwd_launch<4, 1>(a, nhwc, G, d_weight, d_bias, d_bias_pad, s);
    return two ? pfn::bwd_launch<9, 2>(a, nhwc, G, d_weight, d_bias, d_bias_pad, s) : pfn::bwd_launch<9, 1>(a, nhwc, G, d_weight, d_bias, d_bias_pad, s);
}
