// The moments of a PillarBatch's used voxel slots and their adjoint (include/mcav_depth.h: mcav_pillar_moments, mcav_pillar_moments_bwd; the
// definition is tests/pfn_stats_ref.py, the arithmetic csrc/pfn_stats_math.h): what training-mode BatchNorm statistics behind a linear layer
// without bias follow from -- the count, the columns' sums s and their second-moment matrix M -- in one pass over the used slots.
//   A wavefront owns groups of STATS_ROWS consecutive rows, group i going to wavefront i % (4 grid) on a grid that depends on the capacity
//   alone.  A lane reads one row's count; the counts are scanned over the wavefront and every used slot of the group gets an entry
//   (row, slot) in a table in LDS, so the lanes then take the group's used slots 64 at a time whatever the rows' fill: a lane per slot of
//   the [N] a row has would idle 29 of 32 lanes on beam clouds, 24 on dense ones.  A lane keeps s and the upper triangle of M in float64
//   registers: C + C (C + 1) / 2 = 54 doubles at C = 9, 108 of the kernel's 156 VGPRs, which leaves three wavefronts a SIMD (93 VGPRs and
//   four at C = 4); the grid's 512 workgroups are two a CU.  A term is the exact float64 product of two float32 values.
//   At the end the workgroup adds its lanes' accumulators (block_sum: the butterfly, then the wavefronts from left to right) and writes
//   them to its column of the slab [sums][grid]; a second launch, one wavefront per sum, adds a slab row (lane l takes columns l, l + 64,
//   ..., then the butterfly) and writes both halves of M from the one value.  The assignment of slots to accumulators is fixed, so two
//   runs give the same bytes.
//   The adjoint is one launch: a wavefront per row as pfn_bwd.hip writes d_voxels, 4-byte coalesced stores inside the live rows, 16-byte
//   stores behind them.
// No atomics, nothing returns to the host, no allocation: both calls can be captured.
#include "block_ops.h"
#include "pfn_stats_math.h"

namespace mcav {
namespace pfn {

constexpr int STATS_THREADS = STATS_WAVES * 64;
constexpr int STATS_BWD_GRID = 4096;     // workgroups of the adjoint at most
typedef float stats_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void stats_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int C>
__global__ __launch_bounds__(STATS_THREADS) void pfn_moments_kernel(const float* __restrict__ voxels, const int* __restrict__ num_points,
                                                                    const int* __restrict__ pillar_offsets, int B, long long capacity, int N,
                                                                    double* __restrict__ slab) {
    __shared__ unsigned short table[STATS_WAVES][STATS_ROWS * MAX_POINTS];      // (slot << 6) | row of the group, one entry a used slot
    __shared__ double red[STATS_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned short* mine = table[wave];
    constexpr int T = stats_triangle(C);
    double s[C], tri[T], used = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0.0;
#pragma unroll
    for (int q = 0; q < T; ++q) tri[q] = 0.0;
    const long long P = live_pillars(pillar_offsets, B, capacity);
    const long long first = ((long long)blockIdx.x * STATS_WAVES + wave) * STATS_ROWS, step = (long long)gridDim.x * STATS_WAVES * STATS_ROWS;
    for (long long r0 = first; r0 < P; r0 += step) {
        const long long r = r0 + lane;
        const int n = r < P ? used_slots(num_points[r], N) : 0;
        int inc = n;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int a = __shfl_up(inc, off, 64);
            if (lane >= off) inc += a;
        }
        const int total = __shfl(inc, 63, 64);                // <= STATS_ROWS * MAX_POINTS: the table holds them
        for (int k = 0; k < n; ++k) mine[inc - n + k] = (unsigned short)((k << 6) | lane);
        used += (double)n;
        stats_wave_lds_sync();
        for (int j = lane; j < total; j += 64) {
            const int e = mine[j];
            const float* x = voxels + ((size_t)(r0 + (e & 63)) * (size_t)N + (size_t)(e >> 6)) * C;
            float v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = x[c];
            moments_add<C>(v, s, tri);
        }
        stats_wave_lds_sync();                                // the table is free again
    }
    const int G = gridDim.x;
    auto leave = [&](double v, int q) {
        v = block_sum<double, STATS_WAVES>(v, red);
        if (threadIdx.x == 0) slab[(size_t)q * G + blockIdx.x] = v;
    };
    leave(used, 0);
#pragma unroll
    for (int c = 0; c < C; ++c) leave(s[c], 1 + c);
#pragma unroll
    for (int q = 0; q < T; ++q) leave(tri[q], 1 + C + q);
}

// one wavefront per sum: the slab's row in a fixed order; an entry of the triangle goes to both halves of M
__global__ __launch_bounds__(STATS_THREADS) void pfn_moments_reduce_kernel(const double* __restrict__ slab, int G, int C,
                                                                           const int* __restrict__ pillar_offsets, int B, long long capacity, int N,
                                                                           double* __restrict__ moments) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * STATS_WAVES + (int)(threadIdx.x >> 6);
    if (q >= stats_sums(C)) return;
    const double* row = slab + (size_t)q * G;
    double v = 0.0;
    for (int g = lane; g < G; g += 64) v += row[g];
    v = wave_sum(v);
    if (lane != 0) return;
    if (q == 0) {
        moments[0] = (double)(live_pillars(pillar_offsets, B, capacity) * N);
        moments[1] = v;
    } else if (q <= C) {
        moments[1 + q] = v;
    } else {
        int c = 0, t = q - 1 - C;                            // the triangle's row c holds C - c entries
        while (t >= C - c) { t -= C - c; ++c; }
        const int d = c + t;
        double* M = moments + 2 + C;
        M[c * C + d] = v;
        M[d * C + c] = v;
    }
}

template <int C>
__global__ __launch_bounds__(STATS_THREADS) void pfn_moments_bwd_kernel(const float* __restrict__ voxels, const int* __restrict__ num_points,
                                                                        const int* __restrict__ pillar_offsets, int B, long long capacity, int N,
                                                                        const double* __restrict__ g, const double* __restrict__ H,
                                                                        float* __restrict__ d_voxels) {
    __shared__ double Gs[C * C], gs[C];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (threadIdx.x < C * C) Gs[threadIdx.x] = adjoint_entry(H, C, (int)threadIdx.x / C, (int)threadIdx.x % C);
    if (threadIdx.x < C) gs[threadIdx.x] = g[threadIdx.x];
    __syncthreads();
    const long long P = live_pillars(pillar_offsets, B, capacity);
    const int NC = N * C;
    for (long long r = (long long)blockIdx.x * STATS_WAVES + wave; r < P; r += (long long)gridDim.x * STATS_WAVES) {
        const int n = __builtin_amdgcn_readfirstlane(used_slots(num_points[r], N));
        const float* x = voxels + (size_t)r * (size_t)NC;
        float* out = d_voxels + (size_t)r * (size_t)NC;
        for (int e = lane; e < NC; e += 64) {
            float v = 0.0f;
            if (e < n * C) {                                  // a used slot: unused ones are never read
                const int k = e / C, c = e - k * C;
                v = moments_bwd_value(gs[c], Gs + c * C, x + k * C, C);
            }
            out[e] = v;
        }
    }
    // ---- behind the last pillar: one run of zeros up to the capacity, in 16-byte stores between its unaligned ends
    const size_t begin = (size_t)P * (size_t)NC, end = (size_t)capacity * (size_t)NC;
    const size_t past = ((reinterpret_cast<uintptr_t>(d_voxels) >> 2) + begin) & 3;          // floats behind a 16-byte boundary
    const size_t body = begin + (past ? 4 - past : 0) < end ? begin + (past ? 4 - past : 0) : end;
    const size_t groups = (end - body) / 4, tail = body + 4 * groups;
    const size_t t = (size_t)blockIdx.x * STATS_THREADS + threadIdx.x, threads = (size_t)gridDim.x * STATS_THREADS;
    if (t < body - begin) d_voxels[begin + t] = 0.0f;
    stats_f32x4* wide = reinterpret_cast<stats_f32x4*>(d_voxels + body);
    for (size_t i = t; i < groups; i += threads) wide[i] = stats_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (t < end - tail) d_voxels[tail + t] = 0.0f;
}

inline bool stats_sizes_ok(long long capacity, int max_points, int columns) {
    return capacity >= 0 && max_points >= 1 && max_points <= MAX_POINTS && columns_ok(columns);
}

inline int stats_bwd_grid(long long capacity) {
    const long long c = (capacity + 4 * STATS_WAVES - 1) / (4 * STATS_WAVES);
    return c < 1 ? 1 : (c < STATS_BWD_GRID ? (int)c : STATS_BWD_GRID);
}

}  // namespace pfn
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_pillar_moments_workspace_bytes(long long capacity, int max_points, int columns) {
    if (!pfn::stats_sizes_ok(capacity, max_points, columns)) return 0;
    return align_up(sizeof(double) * (size_t)pfn::stats_sums(columns) * pfn::stats_grid(capacity), 256);
}

MCAV_EXPORT int mcav_pillar_moments(const float* voxels, const int* num_points, const int* pillar_offsets, int B, long long capacity,
                                    int max_points, int columns, double* moments, void* workspace, size_t workspace_bytes, void* stream) {
    if (!voxels || !num_points || !pillar_offsets || !moments || !workspace) return MCAV_E_INVALID;
    if (B <= 0 || B > 65535 || !pfn::stats_sizes_ok(capacity, max_points, columns)) return MCAV_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(voxels) | reinterpret_cast<uintptr_t>(num_points) | reinterpret_cast<uintptr_t>(pillar_offsets)) & 3)
        return MCAV_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(moments) | reinterpret_cast<uintptr_t>(workspace)) & 7) return MCAV_E_INVALID;
    if (workspace_bytes < mcav_pillar_moments_workspace_bytes(capacity, max_points, columns)) return MCAV_E_WORKSPACE;
    const int G = pfn::stats_grid(capacity), S = pfn::stats_sums(columns);
    double* slab = reinterpret_cast<double*>(workspace);
    hipStream_t s = as_stream(stream);
    if (columns == 4) pfn::pfn_moments_kernel<4><<<G, pfn::STATS_THREADS, 0, s>>>(voxels, num_points, pillar_offsets, B, capacity, max_points, slab);
    else pfn::pfn_moments_kernel<9><<<G, pfn::STATS_THREADS, 0, s>>>(voxels, num_points, pillar_offsets, B, capacity, max_points, slab);
    pfn::pfn_moments_reduce_kernel<<<(S + pfn::STATS_WAVES - 1) / pfn::STATS_WAVES, pfn::STATS_THREADS, 0, s>>>(slab, G, columns, pillar_offsets, B,
                                                                                                              capacity, max_points, moments);
    return launch_status();
}

MCAV_EXPORT int mcav_pillar_moments_bwd(const float* voxels, const int* num_points, const int* pillar_offsets, int B, long long capacity,
                                        int max_points, int columns, const double* g, const double* H, float* d_voxels, void* stream) {
    if (!voxels || !num_points || !pillar_offsets || !g || !H || !d_voxels) return MCAV_E_INVALID;
    if (B <= 0 || B > 65535 || !pfn::stats_sizes_ok(capacity, max_points, columns)) return MCAV_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(voxels) | reinterpret_cast<uintptr_t>(num_points) | reinterpret_cast<uintptr_t>(pillar_offsets) |
         reinterpret_cast<uintptr_t>(d_voxels)) & 3)
        return MCAV_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(H)) & 7) return MCAV_E_INVALID;
    const int G = pfn::stats_bwd_grid(capacity);
    hipStream_t s = as_stream(stream);
    if (columns == 4) pfn::pfn_moments_bwd_kernel<4><<<G, pfn::STATS_THREADS, 0, s>>>(voxels, num_points, pillar_offsets, B, capacity, max_points, g, H, d_voxels);
    else pfn::pfn_moments_bwd_kernel<9><<<G, pfn::STATS_THREADS, 0, s>>>(voxels, num_points, pillar_offsets, B, capacity, max_points, g, H, d_voxels);
    return launch_status();
}
