// Cloud batch -> pillars for a LiDAR 3-D detector (include/mcav_depth.h: mcav_pillarize; the definition is tests/pillar_ref.py, the
// arithmetic csrc/pillar_math.h).  A counting sort of the points by cell, then one wavefront per pillar:
//   memset  : the per-cell counters
//   point   : image by bisection over offsets, cell, one integer atomicAdd on the cell's counter; (cell, returned slot) kept per point.
//             The slot only places the point inside its cell's segment -- in arrival order, which nothing below depends on.
//   reduce / scan / apply : an exclusive scan over the B * ny * nx counters in tiles of 1024 (the grid is flat: no tile knows of ny * nx),
//             giving every cell's segment start, every non-empty cell's pillar rank, the list of pillar cells and pillar_offsets
//   fill    : point indices into the segments
//   gather  : per pillar, the max_points smallest indices of its segment in ascending order (64 at a time, each entry ranked among the
//             kept set and the chunk), the points, the float64 means in slot order, the row block through LDS with 16-byte stores
// Integer atomics only, nothing returns to the host, no allocation: the call can be captured, and two runs give the same bytes.
// mcav_pillarize_indexed is the same sequence with one more store in the gather: the cloud row in every slot (-1 in the padding), which is
// all the backward (pl_bwd.hip) needs to know of the selection.
#include <limits.h>

#include "block_ops.h"
#include "pillar_math.h"

namespace mcav {
namespace pil {

constexpr int THREADS = 256;
constexpr int PER_THREAD = 4;
constexpr int TILE = THREADS * PER_THREAD;       // cells per block of the scan passes
constexpr int GATHER_BLOCKS = 8192;              // 32 single-wave blocks per CU; the pillars beyond are reached by the grid's stride

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// The scans carry two counters at once, points in the low word of a Pair and pillars (non-empty cells) in the high word: both totals are
// below 2^31 (the caller's checks), so nothing carries from one into the other.
typedef unsigned long long Pair;
__device__ __forceinline__ Pair pair_of(unsigned points, unsigned pillars) { return (Pair)points | (Pair)pillars << 32; }
__device__ __forceinline__ unsigned points_of(Pair p) { return (unsigned)p; }
__device__ __forceinline__ unsigned pillars_of(Pair p) { return (unsigned)(p >> 32); }

// the four counters of a thread; beyond the grid they read as empty cells
__device__ __forceinline__ void load_cells(const unsigned* cells, unsigned M, unsigned j, unsigned (&c)[PER_THREAD]) {
    if (j + PER_THREAD <= M) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(cells + j);
        c[0] = v[0]; c[1] = v[1]; c[2] = v[2]; c[3] = v[3];
    } else {
#pragma unroll
        for (int e = 0; e < PER_THREAD; ++e) c[e] = j + e < M ? cells[j + e] : 0u;
    }
}

__device__ __forceinline__ Pair cells_sum(const unsigned (&c)[PER_THREAD]) {
    Pair v = 0;
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e) v += pair_of(c[e], c[e] ? 1u : 0u);
    return v;
}

__device__ __forceinline__ int live_points(const int* offsets, int B, int n_max) { return min(offsets[B], n_max); }

__global__ __launch_bounds__(THREADS) void pil_point_kernel(const f32x4* points, const int* offsets, int B, int n_max, Grid g, unsigned* cells,
                                                            int2* rec) {
    const unsigned i = blockIdx.x * (unsigned)THREADS + threadIdx.x;
    if (i >= (unsigned)n_max || (int)i >= live_points(offsets, B, n_max)) return;
    const f32x4 p = points[i];
    int2 r = make_int2(-1, 0);
    int ix, iy;
    if (cell_of(g, p[0], p[1], p[2], ix, iy)) {
        const int b = image_of(offsets, B, (int)i);
        r.x = (b * g.ny + iy) * g.nx + ix;                 // below 2^31: checked by the caller
        r.y = (int)atomicAdd(cells + r.x, 1u);
    }
    rec[i] = r;
}

__global__ __launch_bounds__(THREADS) void pil_reduce_kernel(const unsigned* cells, unsigned M, unsigned* tile_points, unsigned* tile_pillars) {
    __shared__ Pair wsum[THREADS / 64];
    unsigned c[PER_THREAD];
    load_cells(cells, M, blockIdx.x * (unsigned)TILE + threadIdx.x * PER_THREAD, c);
    const Pair total = block_sum<Pair, THREADS / 64>(cells_sum(c), wsum);
    if (threadIdx.x == 0) { tile_points[blockIdx.x] = points_of(total); tile_pillars[blockIdx.x] = pillars_of(total); }
}

// exclusive scan of the tiles' sums in one block, 1024 per pass; the totals go to cells[M] (the end of the last segment) and pillar_offsets[B]
__global__ __launch_bounds__(1024) void pil_scan_kernel(unsigned* tile_points, unsigned* tile_pillars, unsigned ntiles, unsigned* cells, unsigned M,
                                                        int* pillar_offsets, int B) {
    __shared__ Pair wsum[16];
    const Pair total = chunked_scan<Pair, 16>((int)ntiles, wsum, [&](int i) { return pair_of(tile_points[i], tile_pillars[i]); },
                                              [&](int i, Pair v) { tile_points[i] = points_of(v); tile_pillars[i] = pillars_of(v); });
    if (threadIdx.x == 0) { cells[M] = points_of(total); pillar_offsets[B] = (int)pillars_of(total); }
}

// counters -> segment starts (in place: a thread rewrites the four it read); the rank and the cell of every pillar; pillar_offsets[b] at
// the first cell of image b
__global__ __launch_bounds__(THREADS) void pil_apply_kernel(unsigned* cells, unsigned M, unsigned per_image, const unsigned* tile_points,
                                                            const unsigned* tile_pillars, int* pillar_cell, int* pillar_offsets) {
    __shared__ Pair wsum[THREADS / 64];
    const unsigned j = blockIdx.x * (unsigned)TILE + threadIdx.x * PER_THREAD;
    unsigned c[PER_THREAD];
    load_cells(cells, M, j, c);
    Pair total;
    const Pair ex = block_scan<Pair, THREADS / 64>(cells_sum(c), wsum, total);
    unsigned start = tile_points[blockIdx.x] + points_of(ex), rank = tile_pillars[blockIdx.x] + pillars_of(ex);
    unsigned s[PER_THREAD];
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e) {
        s[e] = start;
        if (j + e < M) {
            if ((j + e) % per_image == 0) pillar_offsets[(j + e) / per_image] = (int)rank;
            if (c[e]) pillar_cell[rank++] = (int)(j + e);
        }
        start += c[e];
    }
    if (j + PER_THREAD <= M) {
        u32x4 o;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
        *reinterpret_cast<u32x4*>(cells + j) = o;
    } else {
#pragma unroll
        for (int e = 0; e < PER_THREAD; ++e)
            if (j + e < M) cells[j + e] = s[e];
    }
}

__global__ __launch_bounds__(THREADS) void pil_fill_kernel(const int2* rec, const int* offsets, int B, int n_max, const unsigned* cells, int* index) {
    const unsigned i = blockIdx.x * (unsigned)THREADS + threadIdx.x;
    if (i >= (unsigned)n_max || (int)i >= live_points(offsets, B, n_max)) return;
    const int2 r = rec[i];
    if (r.x >= 0) index[cells[r.x] + (unsigned)r.y] = (int)i;
}

// One wavefront (a block of its own: its barriers cost nothing and order its LDS traffic) per pillar.
template <bool DECORATE>
__global__ __launch_bounds__(64) void pil_gather_kernel(const f32x4* points, const unsigned* cells, const int* index, const int* pillar_cell,
                                                        const int* pillar_offsets, int B, Grid g, unsigned per_image, int N, float* voxels,
                                                        int4* coords, int* num_points, size_t capacity, int* slot_points) {
    constexpr int C = DECORATE ? COLS_DECORATED : COLS_PLAIN;
    __shared__ int kept[2][MAX_POINTS];
    __shared__ int chunk[64];
    __shared__ __attribute__((aligned(16))) float tile[MAX_POINTS * C];
    const int lane = threadIdx.x;
    const size_t total_pillars = (size_t)max(pillar_offsets[B], 0);
    const size_t P = total_pillars < capacity ? total_pillars : capacity;
    for (size_t r = blockIdx.x; r < P; r += gridDim.x) {
        const unsigned cell = (unsigned)pillar_cell[r];
        const unsigned start = cells[cell], count = cells[cell + 1] - start;
        // ---- the N smallest indices of the segment, ascending, in kept[cur][0 .. k)
        int k = 0, cur = 0;
        for (unsigned done = 0; done < count; done += 64u) {
            const int c = (int)min(64u, count - done);
            const int mine_c = lane < c ? index[start + done + lane] : INT_MAX;
            chunk[lane] = mine_c;
            __syncthreads();
            if (lane < k) {
                const int mine_k = kept[cur][lane];
                const int rk = rank_among(mine_k, kept[cur], k, chunk, c);
                if (rk < N) kept[cur ^ 1][rk] = mine_k;
            }
            if (lane < c) {
                const int rc = rank_among(mine_c, kept[cur], k, chunk, c);
                if (rc < N) kept[cur ^ 1][rc] = mine_c;
            }
            k = min(k + c, N);
            cur ^= 1;
            __syncthreads();
        }
        // ---- the slots: the points, zero rows behind them
        f32x4 p = {0.0f, 0.0f, 0.0f, 0.0f};
        if (lane < k) p = points[kept[cur][lane]];
        if (lane < N) {
            float* row = tile + lane * C;
            row[0] = p[0]; row[1] = p[1]; row[2] = p[2]; row[3] = p[3];
            if constexpr (DECORATE) { row[4] = 0.0f; row[5] = 0.0f; row[6] = 0.0f; row[7] = 0.0f; row[8] = 0.0f; }
        }
        const int b = (int)(cell / per_image);
        const unsigned in_image = cell - (unsigned)b * per_image;
        const int iy = (int)(in_image / (unsigned)g.nx), ix = (int)(in_image - (unsigned)iy * (unsigned)g.nx);
        if constexpr (DECORATE) {
            __syncthreads();
            const float mx = column_mean(tile + 0, C, k), my = column_mean(tile + 1, C, k), mz = column_mean(tile + 2, C, k);
            if (lane < k) decorate(p[0], p[1], p[2], mx, my, mz, cell_centre(ix, g.x0, g.vx), cell_centre(iy, g.y0, g.vy), tile + lane * C + 4);
        }
        __syncthreads();
        // ---- the N x C block, contiguous in the output
        const int total = N * C;
        float* out = voxels + r * (size_t)total;
        if ((total & 3) == 0) {                            // C = 4, or C = 9 with N a multiple of 4: the block starts on 16 bytes
            for (int e = lane * 4; e < total; e += 256) *reinterpret_cast<f32x4*>(out + e) = *reinterpret_cast<const f32x4*>(tile + e);
        } else {
            for (int e = lane; e < total; e += 64) out[e] = tile[e];
        }
        if (slot_points && lane < N) slot_points[r * (size_t)N + lane] = lane < k ? kept[cur][lane] : -1;       // mcav_pillarize_indexed
        if (lane == 0) {
            coords[r] = make_int4(b, 0, iy, ix);
            num_points[r] = k;
        }
        __syncthreads();                                   // the next pillar reuses kept, chunk and tile
    }
}

struct Layout {
    size_t cells, tile_points, tile_pillars, rec, index, pillar_cell, total;
    unsigned M, ntiles;
    size_t max_pillars;
};

inline bool layout(int B, long long n_max, int ny, int nx, Layout& l) {
    if (B <= 0 || B > 65535 || n_max < 0 || n_max > 0x7fffffffll || nx < 1 || ny < 1) return false;
    const unsigned long long M = (unsigned long long)B * (unsigned long long)ny * (unsigned long long)nx;
    if (M > 0x7fffffffull) return false;                   // int32 cell ids, one grid dimension
    l.M = (unsigned)M;
    l.ntiles = (unsigned)((M + TILE - 1) / TILE);
    l.max_pillars = (size_t)((unsigned long long)n_max < M ? (unsigned long long)n_max : M);
    l.cells = 0;
    l.tile_points = l.cells + align_up(sizeof(unsigned) * ((size_t)M + 1), 256);
    l.tile_pillars = l.tile_points + align_up(sizeof(unsigned) * l.ntiles, 256);
    l.rec = l.tile_pillars + align_up(sizeof(unsigned) * l.ntiles, 256);
    l.index = l.rec + align_up(sizeof(int2) * (size_t)n_max, 256);
    l.pillar_cell = l.index + align_up(sizeof(int) * (size_t)n_max, 256);
    l.total = l.pillar_cell + align_up(sizeof(int) * l.max_pillars, 256);
    return true;
}

}  // namespace pil
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_pillarize_workspace_bytes(int B, long long n_max, int ny, int nx) {
    pil::Layout l;
    return pil::layout(B, n_max, ny, nx, l) ? l.total : 0;
}

// both entries' body; slot_points: null, or device int [capacity, max_points]
static int pillarize(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float z1, float vx, float vy,
                     int nx, int ny, int max_points, int flags, float* voxels, int* coords, int* num_points, long long capacity,
                     int* pillar_offsets, int* slot_points, void* workspace, size_t workspace_bytes, void* stream) {
    if (!points || !offsets || !voxels || !coords || !num_points || !pillar_offsets || !workspace) return MCAV_E_INVALID;
    if (max_points < 1 || max_points > pil::MAX_POINTS || capacity < 0 || (flags & ~MCAV_PILLAR_DECORATE)) return MCAV_E_INVALID;
    const pil::Grid g{x0, y0, z0, z1, vx, vy, nx, ny};
    pil::Layout l;
    if (!pil::grid_ok(g) || !pil::layout(B, n_max, ny, nx, l)) return MCAV_E_INVALID;
    const int columns = (flags & MCAV_PILLAR_DECORATE) ? pil::COLS_DECORATED : pil::COLS_PLAIN;
    const uintptr_t wide_voxels = ((max_points * columns) & 3) == 0 ? reinterpret_cast<uintptr_t>(voxels) : 0;      // else dword stores
    if ((reinterpret_cast<uintptr_t>(points) | wide_voxels | reinterpret_cast<uintptr_t>(coords) | reinterpret_cast<uintptr_t>(workspace)) & 15)
        return MCAV_E_INVALID;                             // 16-byte loads and stores
    if (reinterpret_cast<uintptr_t>(voxels) & 3) return MCAV_E_INVALID;
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;

    char* ws = reinterpret_cast<char*>(workspace);
    unsigned* cells = reinterpret_cast<unsigned*>(ws + l.cells);
    unsigned* tile_points = reinterpret_cast<unsigned*>(ws + l.tile_points);
    unsigned* tile_pillars = reinterpret_cast<unsigned*>(ws + l.tile_pillars);
    int2* rec = reinterpret_cast<int2*>(ws + l.rec);
    int* index = reinterpret_cast<int*>(ws + l.index);
    int* pillar_cell = reinterpret_cast<int*>(ws + l.pillar_cell);
    const pil::f32x4* pts = reinterpret_cast<const pil::f32x4*>(points);
    const unsigned per_image = (unsigned)ny * (unsigned)nx;
    const unsigned point_blocks = (unsigned)((n_max + pil::THREADS - 1) / pil::THREADS);
    hipStream_t s = as_stream(stream);

    if (hipMemsetAsync(cells, 0, sizeof(unsigned) * (size_t)l.M, s) != hipSuccess) return MCAV_E_LAUNCH;
    if (point_blocks) pil::pil_point_kernel<<<point_blocks, pil::THREADS, 0, s>>>(pts, offsets, B, (int)n_max, g, cells, rec);
    pil::pil_reduce_kernel<<<l.ntiles, pil::THREADS, 0, s>>>(cells, l.M, tile_points, tile_pillars);
    pil::pil_scan_kernel<<<1, 1024, 0, s>>>(tile_points, tile_pillars, l.ntiles, cells, l.M, pillar_offsets, B);
    pil::pil_apply_kernel<<<l.ntiles, pil::THREADS, 0, s>>>(cells, l.M, per_image, tile_points, tile_pillars, pillar_cell, pillar_offsets);
    if (point_blocks) pil::pil_fill_kernel<<<point_blocks, pil::THREADS, 0, s>>>(rec, offsets, B, (int)n_max, cells, index);
    const size_t rows = l.max_pillars < (size_t)capacity ? l.max_pillars : (size_t)capacity;
    if (rows) {
        const unsigned blocks = (unsigned)(rows < (size_t)pil::GATHER_BLOCKS ? rows : (size_t)pil::GATHER_BLOCKS);
        if (flags & MCAV_PILLAR_DECORATE)
            pil::pil_gather_kernel<true><<<blocks, 64, 0, s>>>(pts, cells, index, pillar_cell, pillar_offsets, B, g, per_image, max_points,
                                                               voxels, reinterpret_cast<int4*>(coords), num_points, (size_t)capacity, slot_points);
        else
            pil::pil_gather_kernel<false><<<blocks, 64, 0, s>>>(pts, cells, index, pillar_cell, pillar_offsets, B, g, per_image, max_points,
                                                                voxels, reinterpret_cast<int4*>(coords), num_points, (size_t)capacity, slot_points);
    }
    return launch_status();
}

MCAV_EXPORT int mcav_pillarize(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float z1, float vx,
                               float vy, int nx, int ny, int max_points, int flags, float* voxels, int* coords, int* num_points,
                               long long capacity, int* pillar_offsets, void* workspace, size_t workspace_bytes, void* stream) {
    return pillarize(points, offsets, B, n_max, x0, y0, z0, z1, vx, vy, nx, ny, max_points, flags, voxels, coords, num_points, capacity,
                     pillar_offsets, nullptr, workspace, workspace_bytes, stream);
}

MCAV_EXPORT int mcav_pillarize_indexed(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float z1,
                                       float vx, float vy, int nx, int ny, int max_points, int flags, float* voxels, int* coords,
                                       int* num_points, long long capacity, int* pillar_offsets, int* slot_points, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!slot_points) return MCAV_E_INVALID;
    return pillarize(points, offsets, B, n_max, x0, y0, z0, z1, vx, vy, nx, ny, max_points, flags, voxels, coords, num_points, capacity,
                     pillar_offsets, slot_points, workspace, workspace_bytes, stream);
}
