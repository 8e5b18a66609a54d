// Pillars -> pillar features -> BEV pseudo-image in one launch (include/mcav_depth.h: mcav_pillar_pseudo_image; the definition is
// tests/pfn_ref.py, the arithmetic csrc/pfn_math.h).  PointPillars' PillarVFE (Linear + folded BatchNorm + ReLU + max over the pillar's
// points) and PointPillarScatter, without the [P, N, C_out] intermediate, the memset of the canvas or the strided scatter into it.
//   A workgroup owns one canvas row (b, iy) and walks it in tiles of TILE columns.  mcav_pillarize leaves the pillars in ascending
//   (b, iy, ix) order, so the row's pillars are one run of rows: every wavefront finds its first row inside pillar_offsets[b] ..
//   pillar_offsets[b + 1] with 64 probes a round (three dependent loads for 2^18 rows where a bisection takes eighteen), once per canvas
//   row; a tile's pillars lie in the TILE rows from there on, tested one per lane with two ballots, and the next tile's follow them.
//   The tile's image [C_out][TILE] (NHWC: [TILE][C_out]) starts as zeros in LDS.  A wavefront takes every WAVES-th pillar of the window: its N x C block comes in with one coalesced load per lane and
//   64 floats (the next pillar's while this one is computed), is staged in the wavefront's corner of LDS and read back as broadcasts, one
//   lane per output channel (two at C_out > 64) with that channel's weights in registers; the maximum goes into the pillar's column of
//   the image, and the image goes out in full-width stores.  The canvas is written once, never read.
// The layer is VALU fmaf, which is the definition; an MFMA form was not tried.  No atomics, nothing
// returns to the host, no allocation, no workspace: the call can be captured, and two runs give the same bytes.
#include "mcav_common.h"
#include "pfn_math.h"

namespace mcav {
namespace pfn {

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / 64;
constexpr int TILE = 128;                        // columns per workgroup: two ballots cover a tile's rows
constexpr int GROUPS = TILE / 4;                 // 16-byte groups of a tile row
constexpr unsigned MAX_BLOCKS = 1u << 22;        // the tiles beyond are reached by the grid's stride
constexpr int FEATURE_THREADS = 256, FEATURE_WAVES = FEATURE_THREADS / 64, FEATURE_BLOCKS = 8192;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Args {
    const float* voxels;
    const int* coords;
    const int* num_points;
    const int* pillar_offsets;
    const float* weight;
    const float* bias;
    const float* bias_pad;
    float* canvas;
    float* features;
    long long capacity;
    int B, N, nx, ny, c_out, tiles_x;
    int stage;                                   // floats of LDS a wavefront stages a pillar in: N * C rounded up to a multiple of 4
    bool wide;                                   // 16-byte stores: every run of the canvas starts on 16 bytes
};

inline int stage_floats(int N, int C) { return (N * C + 3) & ~3; }

// stores to LDS by some lanes of a wavefront, loads by others: LDS serves a wavefront's instructions in order, the compiler must keep them so
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The lane's channels (lane, lane + 64) with their weights, held for the life of the workgroup, and the wavefront's way through a pillar.
// A lane without a channel takes the last channel's and writes nothing.
template <int C, int CPL>
struct Lane {
    float w[CPL][C], bias[CPL], pad[CPL];
    int o[CPL];
    bool live[CPL];
    float block[C];                              // floats lane, lane + 64, ... of the pillar on its way in (N * C <= 64 * C)
    int n;                                       // and its used slots
    __device__ __forceinline__ void load(const Args& a, int lane) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            o[j] = lane + 64 * j;
            live[j] = o[j] < a.c_out;
            const int src = live[j] ? o[j] : a.c_out - 1;
#pragma unroll
            for (int c = 0; c < C; ++c) w[j][c] = a.weight[src * C + c];
            bias[j] = a.bias[src];
            pad[j] = a.bias_pad[src];
        }
    }
    // row r's used slots into registers, 256 bytes per load (r is the same in every lane)
    __device__ __forceinline__ void fetch(const Args& a, long long r, int lane) {
        n = used_slots(a.num_points[r], a.N);
        const float* rows = a.voxels + (size_t)r * (size_t)(a.N * C);
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int f = lane + 64 * j;
            block[j] = f < n * C ? rows[f] : 0.0f;
        }
    }
    // the fetched pillar into `stage`, then feat[r, o] of pfn_ref.py for the lane's channels; returns with the stage free again
    __device__ __forceinline__ void put(float* stage, int lane) const {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int f = lane + 64 * j;
            if (f < n * C) stage[f] = block[j];
        }
        wave_lds_sync();
    }
    __device__ __forceinline__ void features(const Args& a, const float* stage, int slots, float (&feat)[CPL]) const {
        Max m[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) m[j] = max_start(slots < a.N, pad[j]);
#pragma unroll 2
        for (int k = 0; k < slots; ++k) {
            float x[C];
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = stage[k * C + c];           // one address in every lane: a broadcast
#pragma unroll
            for (int j = 0; j < CPL; ++j) max_join(m[j], act(pre(x, w[j], C, bias[j])));
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) feat[j] = max_value(m[j]);
        wave_lds_sync();
    }
};

// where (channel o, column col) of the tile lives in LDS.  NCHW: rows of TILE columns, the 16-byte groups of row o XORed with o % 16, so
// that a wavefront's 64 channels of one column spread over 16 banks instead of one and a group is still read in one piece.
template <bool NHWC>
__device__ __forceinline__ int lds_index(int o, int col, int c_out) {
    if constexpr (NHWC) return col * c_out + o;
    else return o * TILE + ((((col >> 2) ^ (o & 15)) << 2) | (col & 3));
}

// first_at_or_after of pfn_math.h with the wavefront's lanes as the probes
__device__ __forceinline__ long long wave_first_at_or_after(const int* coords, long long lo, long long hi, int y, int x, int lane) {
    while (lo < hi) {
        const long long step = search_step(lo, hi), r = lo + lane * step;
        const int below = __popcll(__ballot(r < hi && row_below(coords, r, y, x)));
        search_narrow(lo, hi, step, below);
    }
    return lo;
}

template <int C, int CPL, bool NHWC>
__global__ __launch_bounds__(THREADS) void pfn_image_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];            // the image, c_out * TILE floats, then WAVES stages
    float* image = lds;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* stage = lds + a.c_out * TILE + wave * a.stage;
    Lane<C, CPL> ch;
    ch.load(a, lane);
    const long long P = live_pillars(a.pillar_offsets, a.B, a.capacity);
    const unsigned rows = (unsigned)a.B * (unsigned)a.ny;                            // below 2^31: B ny nx is
    const int cells = a.c_out * TILE;
    long long lo = 0, hi = 0, first = 0;
    for (unsigned row = blockIdx.x; row < rows; row += gridDim.x)
    for (int tx = 0; tx < a.tiles_x; ++tx) {                                          // a canvas row's tiles, left to right
        const int iy = (int)(row % (unsigned)a.ny), b = (int)(row / (unsigned)a.ny);
        const int x0 = tx * TILE, w = min(TILE, a.nx - x0);
        for (int e = threadIdx.x * 4; e < cells; e += THREADS * 4) *reinterpret_cast<f32x4*>(image + e) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // ---- the tile's rows: members of the TILE rows from `first` on, as two masks (the same in every wavefront).  One search per
        // canvas row: its rows are in ascending ix, so a tile's members are the rows from `first` on and the next tile's follow them.
        if (tx == 0) {
            image_rows(a.pillar_offsets, b, P, lo, hi);
            first = wave_first_at_or_after(a.coords, lo, hi, iy, 0, lane);
        }
        unsigned long long member[2];
        int column[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long r = first + 64 * h + lane;
            const bool in = r < hi && in_tile(a.coords, r, b, iy, x0, w);             // unsorted input: never outside the tile
            column[h] = in ? a.coords[4 * r + 3] - x0 : 0;
            member[h] = __ballot(in);
        }
        __syncthreads();
        // ---- every WAVES-th member is this wavefront's, the next one fetched while this one is computed
        int half = 0, seen = 0;
        unsigned long long left = member[0];
        auto next = [&]() -> int {                                                    // the window index of the wavefront's next row, -1 at the end
            for (;;) {
                if (left == 0) {
                    if (half == 1) return -1;
                    half = 1;
                    left = member[1];
                    continue;
                }
                const int bit = __builtin_ctzll(left);
                left &= left - 1;
                if (seen++ % WAVES == wave) return 64 * half + bit;
            }
        };
        int cur = next();
        if (cur >= 0) ch.fetch(a, first + cur, lane);
        while (cur >= 0) {
            const int slots = ch.n;
            ch.put(stage, lane);
            const int nxt = next();
            if (nxt >= 0) ch.fetch(a, first + nxt, lane);
            float feat[CPL];
            ch.features(a, stage, slots, feat);
            const long long r = first + cur;
            const int col = __shfl(cur < 64 ? column[0] : column[1], cur & 63, 64);
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                if (!ch.live[j]) continue;
                image[lds_index<NHWC>(ch.o[j], col, a.c_out)] = feat[j];
                if (a.features) a.features[(size_t)r * (size_t)a.c_out + ch.o[j]] = feat[j];
            }
            cur = nxt;
        }
        __syncthreads();
        if constexpr (NHWC) {                                                   // the tile is w * c_out floats in one piece
            float* out = a.canvas + ((size_t)row * (size_t)a.nx + (size_t)x0) * (size_t)a.c_out;
            const int count = w * a.c_out;
            if (a.wide) {
                for (int e = threadIdx.x * 4; e < count; e += THREADS * 4) *reinterpret_cast<f32x4*>(out + e) = *reinterpret_cast<const f32x4*>(image + e);
            } else {
                for (int e = threadIdx.x; e < count; e += THREADS) out[e] = image[e];
            }
        } else {                                                                // c_out runs of w floats
            const size_t plane = (size_t)a.ny * (size_t)a.nx;
            float* out = a.canvas + (size_t)b * (size_t)a.c_out * plane + (size_t)iy * (size_t)a.nx + (size_t)x0;
            if (a.wide) {                                                       // nx is a multiple of 4, and so is w
                for (int e = threadIdx.x; e < a.c_out * GROUPS; e += THREADS) {
                    const int o = e / GROUPS, g = e % GROUPS;
                    if (4 * g < w) *reinterpret_cast<f32x4*>(out + (size_t)o * plane + 4 * g) = *reinterpret_cast<const f32x4*>(image + o * TILE + ((g ^ (o & 15)) << 2));
                }
            } else {
                for (int e = threadIdx.x; e < cells; e += THREADS) {
                    const int o = e / TILE, col = e % TILE;
                    if (col < w) out[(size_t)o * plane + col] = image[lds_index<false>(o, col, a.c_out)];
                }
            }
        }
        __syncthreads();                                                        // the next tile zeroes the image
        first += __popcll(member[0]) + __popcll(member[1]);                     // at most hi: members lie below it
    }
}

// features alone (canvas == NULL): one wavefront per pillar, every row below P whatever its coords hold
template <int C, int CPL>
__global__ __launch_bounds__(FEATURE_THREADS) void pfn_features_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];            // FEATURE_WAVES stages
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* stage = lds + wave * a.stage;
    Lane<C, CPL> ch;
    ch.load(a, lane);
    const long long P = live_pillars(a.pillar_offsets, a.B, a.capacity);
    const long long stride = (long long)gridDim.x * FEATURE_WAVES;
    long long r = (long long)blockIdx.x * FEATURE_WAVES + wave;
    if (r < P) ch.fetch(a, r, lane);
    for (; r < P; r += stride) {
        const int slots = ch.n;
        ch.put(stage, lane);
        if (r + stride < P) ch.fetch(a, r + stride, lane);
        float feat[CPL];
        ch.features(a, stage, slots, feat);
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (ch.live[j]) a.features[(size_t)r * (size_t)a.c_out + ch.o[j]] = feat[j];
    }
}

// more than 64 KiB of dynamic LDS has to be allowed once per kernel
template <class K>
bool allow_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

constexpr size_t MAX_LDS = sizeof(float) * ((size_t)MAX_OUT * TILE + (size_t)WAVES * ((MAX_POINTS * MAX_COLUMNS + 3) & ~3));      // 82 KiB

template <int C, int CPL>
int launch(const Args& a, bool nhwc, hipStream_t s) {
    if (!a.canvas) {
        const long long groups = (a.capacity + FEATURE_WAVES - 1) / FEATURE_WAVES;
        const size_t lds = sizeof(float) * (size_t)FEATURE_WAVES * a.stage;
        if (groups > 0) pfn_features_kernel<C, CPL><<<(unsigned)(groups < FEATURE_BLOCKS ? groups : FEATURE_BLOCKS), FEATURE_THREADS, lds, s>>>(a);
        return launch_status();
    }
    static const bool allowed = allow_lds(pfn_image_kernel<C, CPL, true>, MAX_LDS) && allow_lds(pfn_image_kernel<C, CPL, false>, MAX_LDS);
    if (!allowed) return MCAV_E_LAUNCH;
    const unsigned long long rows = (unsigned long long)a.B * (unsigned long long)a.ny;
    const unsigned blocks = (unsigned)(rows < MAX_BLOCKS ? rows : MAX_BLOCKS);
    const size_t lds = sizeof(float) * ((size_t)a.c_out * TILE + (size_t)WAVES * a.stage);
    if (nhwc) pfn_image_kernel<C, CPL, true><<<blocks, THREADS, lds, s>>>(a);
    else pfn_image_kernel<C, CPL, false><<<blocks, THREADS, lds, s>>>(a);
    return launch_status();
}

}  // namespace pfn
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT int mcav_pillar_pseudo_image(const float* voxels, const int* coords, const int* num_points, const int* pillar_offsets, int B,
                                         long long capacity, int max_points, int columns, int nx, int ny, const float* weight,
                                         const float* bias, const float* bias_pad, int c_out, int flags, float* canvas, float* features,
                                         void* stream) {
    if (!voxels || !coords || !num_points || !pillar_offsets || !weight || !bias || !bias_pad || (!canvas && !features)) return MCAV_E_INVALID;
    if (B <= 0 || B > 65535 || capacity < 0 || nx < 1 || ny < 1 || max_points < 1 || max_points > pfn::MAX_POINTS) return MCAV_E_INVALID;
    if ((unsigned long long)B * (unsigned long long)ny * (unsigned long long)nx > 0x7fffffffull) return MCAV_E_INVALID;
    if (!pfn::columns_ok(columns) || !pfn::c_out_ok(c_out) || (flags & ~MCAV_PFN_NHWC)) return MCAV_E_INVALID;
    uintptr_t bits = 0;
    for (const void* p : {(const void*)voxels, (const void*)coords, (const void*)num_points, (const void*)pillar_offsets, (const void*)weight,
                          (const void*)bias, (const void*)bias_pad, (const void*)canvas, (const void*)features})
        bits |= reinterpret_cast<uintptr_t>(p);
    if (bits & 3) return MCAV_E_INVALID;
    const bool nhwc = (flags & MCAV_PFN_NHWC) != 0;
    pfn::Args a{voxels, coords, num_points, pillar_offsets, weight, bias, bias_pad, canvas, features, capacity,
                B, max_points, nx, ny, c_out, (nx + pfn::TILE - 1) / pfn::TILE, pfn::stage_floats(max_points, columns),
                (reinterpret_cast<uintptr_t>(canvas) & 15) == 0 && (nhwc || nx % 4 == 0)};
    hipStream_t s = as_stream(stream);
    const bool two = c_out > 64;
    if (columns == 4) return two ? pfn::launch<4, 2>(a, nhwc, s) : pfn::launch<4, 1>(a, nhwc, s);
    return two ? pfn::launch<9, 2>(a, nhwc, s) : pfn::launch<9, 1>(a, nhwc, s);
}
