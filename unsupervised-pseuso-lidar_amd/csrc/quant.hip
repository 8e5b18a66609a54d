// Cloud batch -> soft-occupancy canvas [B, nz, ny, nx] and its backward to the cloud rows (include/mcav_depth.h: mcav_cloud_occupancy,
// mcav_cloud_occupancy_bwd; the definition is tests/quant_ref.py, the arithmetic csrc/quant_math.h).  The forward is a counting sort of
// the points by bird's-eye-view column (b, iy, ix) -- pillarize.hip's passes restated over plain counters, without its pillar ranks --
// and then one workgroup per tile of TILE_Y x TILE_X columns of one image, twice:
//   memset  : the per-column counters
//   point   : image by bisection over offsets, cell, one integer atomicAdd on the column's counter; (column, returned slot) kept per row;
//             a dropped row's point_count is 0
//   reduce / scan / apply : an exclusive scan over the B * ny * nx counters in tiles of 1024, giving every column's segment start
//   fill    : row indices into the segments (in arrival order, which nothing below depends on)
//   count   : per tile, a histogram of its rows over the nz bins of its columns in LDS; every row's cell count n(m') goes to the workspace
//             beside its index, and to point_count
//   canvas  : per tile, the 64-bit sums S of its nz * TILE_Y * TILE_X cells in LDS; the rows of the tile's columns and of one column
//             around it add the terms that land inside the tile with LDS integer atomics; the tile then leaves as float32 rows of the
//             canvas, 16 bytes per lane where nx allows.  A tile with no row in reach writes its zeros without touching LDS.
// There is no B * nz * ny * nx counter table and no memset of the canvas: the canvas write is the floor of the call.  Integer atomics
// only, nothing returns to the host, no allocation: the call can be captured, and two runs give the same bytes.
// The backward is one thread per cloud row: the cell from the point with the forward's function, 27 reads of d_canvas, one 16-byte store.
#include "block_ops.h"
#include "quant_math.h"

namespace mcav {
namespace qnt {

static_assert(REFUSED == MCAV_E_INVALID && SHORT_WORKSPACE == MCAV_E_WORKSPACE, "quant_math.h restates the return codes");

constexpr int THREADS = 256;
constexpr int PER_THREAD = SCAN_TILE / THREADS;
constexpr int TILE_COLS = TILE_X * TILE_Y;
constexpr int HALO_ROWS = TILE_Y + 2;
static_assert(TILE_X % 4 == 0 && PER_THREAD == 4, "16-byte rows and counter quads");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int live_points(const int* offsets, int B, int n_max) { return max(min(offsets[B], n_max), 0); }

// the four counters of a thread; beyond the grid they read as empty columns
__device__ __forceinline__ void load_cells(const unsigned* cells, unsigned M, unsigned j, unsigned (&c)[PER_THREAD]) {
    if (j + PER_THREAD <= M) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(cells + j);
        c[0] = v[0]; c[1] = v[1]; c[2] = v[2]; c[3] = v[3];
    } else {
#pragma unroll
        for (int e = 0; e < PER_THREAD; ++e) c[e] = j + e < M ? cells[j + e] : 0u;
    }
}

__global__ __launch_bounds__(THREADS) void qnt_point_kernel(const f32x4* points, const int* offsets, int B, int n_max, Grid g, unsigned* cells,
                                                            int2* rec, int* point_count) {
    const unsigned i = blockIdx.x * (unsigned)THREADS + threadIdx.x;
    if (i >= (unsigned)n_max || (int)i >= live_points(offsets, B, n_max)) return;
    const f32x4 p = points[i];
    int2 r = make_int2(-1, 0);
    int ix, iy, iz;
    if (cell_of(g, p[0], p[1], p[2], ix, iy, iz)) {
        const int b = pil::image_of(offsets, B, (int)i);
        r.x = (b * g.ny + iy) * g.nx + ix;                 // below 2^31: checked by the caller
        r.y = (int)atomicAdd(cells + r.x, 1u);
    } else if (point_count) {
        point_count[i] = 0;
    }
    rec[i] = r;
}

__global__ __launch_bounds__(THREADS) void qnt_reduce_kernel(const unsigned* cells, unsigned M, unsigned* tile_sums) {
    __shared__ unsigned wsum[THREADS / 64];
    unsigned c[PER_THREAD];
    load_cells(cells, M, blockIdx.x * (unsigned)SCAN_TILE + threadIdx.x * PER_THREAD, c);
    const unsigned total = block_sum<unsigned, THREADS / 64>((c[0] + c[1]) + (c[2] + c[3]), wsum);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// exclusive scan of the tiles' sums in one block, 1024 per pass; the total goes to cells[M], the end of the last segment
__global__ __launch_bounds__(1024) void qnt_scan_kernel(unsigned* tile_sums, unsigned ntiles, unsigned* cells, unsigned M) {
    __shared__ unsigned wsum[16];
    const unsigned total = chunked_scan<unsigned, 16>((int)ntiles, wsum, [&](int i) { return tile_sums[i]; },
                                                      [&](int i, unsigned v) { tile_sums[i] = v; });
    if (threadIdx.x == 0) cells[M] = total;
}

// counters -> segment starts, in place: a thread rewrites the four it read
__global__ __launch_bounds__(THREADS) void qnt_apply_kernel(unsigned* cells, unsigned M, const unsigned* tile_sums) {
    __shared__ unsigned wsum[THREADS / 64];
    const unsigned j = blockIdx.x * (unsigned)SCAN_TILE + threadIdx.x * PER_THREAD;
    unsigned c[PER_THREAD];
    load_cells(cells, M, j, c);
    unsigned total;
    unsigned start = tile_sums[blockIdx.x] + block_scan<unsigned, THREADS / 64>((c[0] + c[1]) + (c[2] + c[3]), wsum, total);
    unsigned s[PER_THREAD];
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e) {
        s[e] = start;
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

__global__ __launch_bounds__(THREADS) void qnt_fill_kernel(const int2* rec, const int* offsets, int B, int n_max, const unsigned* cells, int* index) {
    const unsigned i = blockIdx.x * (unsigned)THREADS + threadIdx.x;
    if (i >= (unsigned)n_max || (int)i >= live_points(offsets, B, n_max)) return;
    const int2 r = rec[i];
    if (r.x >= 0) index[cells[r.x] + (unsigned)r.y] = (int)i;
}

// The tile of a workgroup: image b, columns [x0, xe) x [y0, ye)
struct Tile {
    int b, x0, y0, xe, ye;
};
__device__ __forceinline__ Tile tile_of(const Grid& g, int tiles_x, int tiles_y) {
    const int t = (int)blockIdx.x;
    Tile w;
    w.b = t / (tiles_x * tiles_y);
    const int in_image = t - w.b * tiles_x * tiles_y;
    w.y0 = in_image / tiles_x * TILE_Y;
    w.x0 = (in_image - in_image / tiles_x * tiles_x) * TILE_X;
    w.xe = min(w.x0 + TILE_X, g.nx);
    w.ye = min(w.y0 + TILE_Y, g.ny);
    return w;
}

// The sorted positions [lo, hi) of the rows in columns [xa, xb) of row y of image b: the columns are contiguous in the sort.  cells[M]
// closes the last segment.
__device__ __forceinline__ void segment(const unsigned* cells, const Grid& g, int b, int y, int xa, int xb, unsigned& lo, unsigned& hi) {
    const unsigned row = ((unsigned)b * (unsigned)g.ny + (unsigned)y) * (unsigned)g.nx;
    lo = cells[row + (unsigned)xa];
    hi = cells[row + (unsigned)xb];
}

// LDS: unsigned hist[nz][TILE_Y][TILE_X]
__global__ __launch_bounds__(THREADS) void qnt_count_kernel(const f32x4* points, const unsigned* cells, const int* index, Grid g, int tiles_x,
                                                            int tiles_y, int* cnt, int* point_count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* hist = reinterpret_cast<unsigned*>(smem);
    const Tile w = tile_of(g, tiles_x, tiles_y);
    unsigned lo[TILE_Y], hi[TILE_Y], total = 0;
#pragma unroll
    for (int r = 0; r < TILE_Y; ++r) {
        lo[r] = hi[r] = 0;
        if (w.y0 + r < w.ye) segment(cells, g, w.b, w.y0 + r, w.x0, w.xe, lo[r], hi[r]);
        total += hi[r] - lo[r];
    }
    if (total == 0) return;                                // the whole workgroup: the bounds are uniform
    for (int e = threadIdx.x; e < g.nz * TILE_COLS; e += THREADS) hist[e] = 0u;
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int r = 0; r < TILE_Y; ++r)
            for (unsigned p = lo[r] + threadIdx.x; p < hi[r]; p += THREADS) {
                const int i = index[p];
                const f32x4 pt = points[i];
                int ix, iy, iz;
                if (!cell_of(g, pt[0], pt[1], pt[2], ix, iy, iz)) continue;       // (never: the sort holds kept rows only)
                unsigned* bin = hist + (iz * TILE_Y + (iy - w.y0)) * TILE_X + (ix - w.x0);
                if (pass == 0) {
                    atomicAdd(bin, 1u);
                } else {
                    const int c = (int)*bin;
                    cnt[p] = c;
                    if (point_count) point_count[i] = c;
                }
            }
        __syncthreads();
    }
}

// Every element of the tile from S (null: +0.0), as rows of the [B, nz, ny, nx] canvas
template <bool WIDE>
__device__ __forceinline__ void store_tile(const unsigned long long* S, const Grid& g, const Tile& w, float* canvas) {
    const int rows = w.ye - w.y0, width = w.xe - w.x0;
    constexpr int PER_LANE = WIDE ? 4 : 1, LANES = TILE_X / PER_LANE;
    for (int e = threadIdx.x; e < g.nz * rows * LANES; e += THREADS) {
        const int x = (e % LANES) * PER_LANE, yz = e / LANES, y = yz % rows, z = yz / rows;
        if (x >= width) continue;
        float v[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) v[k] = S ? from_fixed((long long)S[(z * TILE_Y + y) * TILE_X + x + k]) : 0.0f;
        float* out = canvas + (((size_t)w.b * g.nz + z) * g.ny + (w.y0 + y)) * g.nx + (w.x0 + x);
        if constexpr (WIDE) {
            f32x4 o;
            o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
            *reinterpret_cast<f32x4*>(out) = o;            // nx is a multiple of 4: so are x0 + x and the width
        } else {
            out[0] = v[0];
        }
    }
}

// LDS: unsigned long long S[nz][TILE_Y][TILE_X]
template <bool WIDE>
__global__ __launch_bounds__(THREADS) void qnt_canvas_kernel(const f32x4* points, const unsigned* cells, const int* index, const int* cnt, Grid g,
                                                             float sigma2, int tiles_x, int tiles_y, float* canvas) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* S = reinterpret_cast<unsigned long long*>(smem);
    const Tile w = tile_of(g, tiles_x, tiles_y);
    const int xa = max(w.x0 - 1, 0), xb = min(w.xe + 1, g.nx);
    unsigned lo[HALO_ROWS], hi[HALO_ROWS], total = 0;
#pragma unroll
    for (int r = 0; r < HALO_ROWS; ++r) {
        const int y = w.y0 - 1 + r;
        lo[r] = hi[r] = 0;
        if (y >= 0 && y <= w.ye && y < g.ny) segment(cells, g, w.b, y, xa, xb, lo[r], hi[r]);
        total += hi[r] - lo[r];
    }
    if (total == 0) {                                      // the whole workgroup: the bounds are uniform
        store_tile<WIDE>(nullptr, g, w, canvas);
        return;
    }
    for (int e = threadIdx.x; e < g.nz * TILE_COLS; e += THREADS) S[e] = 0ull;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < HALO_ROWS; ++r)
        for (unsigned p = lo[r] + threadIdx.x; p < hi[r]; p += THREADS) {
            const f32x4 pt = points[index[p]];
            const int n = cnt[p];
            int ix, iy, iz;
            if (!cell_of(g, pt[0], pt[1], pt[2], ix, iy, iz)) continue;           // (never: the sort holds kept rows only)
            float cx[3], cy[3], cz[3];
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                cx[o] = pil::cell_centre(ix + o - 1, g.x0, g.vx);
                cy[o] = pil::cell_centre(iy + o - 1, g.y0, g.vy);
                cz[o] = pil::cell_centre(iz + o - 1, g.z0, g.vz);
            }
            for (int oz = 0; oz < 3; ++oz) {
                const int jz = iz + oz - 1;
                if (jz < 0 || jz >= g.nz) continue;
                for (int oy = 0; oy < 3; ++oy) {
                    const int jy = iy + oy - 1;
                    if (jy < w.y0 || jy >= w.ye) continue;
#pragma unroll
                    for (int ox = 0; ox < 3; ++ox) {
                        const int jx = ix + ox - 1;
                        if (jx < w.x0 || jx >= w.xe) continue;
                        float d[3];
                        const float e = term(pt[0], pt[1], pt[2], cx[ox], cy[oy], cz[oz], sigma2, d);
                        const long long q = to_fixed(e, n, oz == 1 && oy == 1 && ox == 1);
                        if (q) atomicAdd(S + (jz * TILE_Y + (jy - w.y0)) * TILE_X + (jx - w.x0), (unsigned long long)q);
                    }
                }
            }
        }
    __syncthreads();
    store_tile<WIDE>(S, g, w, canvas);
}

__global__ __launch_bounds__(THREADS) void qnt_bwd_kernel(const f32x4* points, const int* offsets, const int* point_count, const float* d_canvas,
                                                          int B, int n_max, Grid g, float sigma2, f32x4* d_points) {
    const unsigned i = blockIdx.x * (unsigned)THREADS + threadIdx.x;
    if (i >= (unsigned)n_max) return;
    float out[3] = {0.0f, 0.0f, 0.0f};
    if ((int)i < live_points(offsets, B, n_max)) {
        const f32x4 p = points[i];
        int ix, iy, iz;
        if (cell_of(g, p[0], p[1], p[2], ix, iy, iz)) {
            const size_t per_image = (size_t)g.nz * g.ny * g.nx;
            point_grad(g, sigma2, d_canvas + pil::image_of(offsets, B, (int)i) * per_image, p[0], p[1], p[2], ix, iy, iz, point_count[i], out);
        }
    }
    f32x4 o;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2]; o[3] = 0.0f;
    d_points[i] = o;
}

}  // namespace qnt
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_cloud_occupancy_workspace_bytes(int B, long long n_max, int nz, int ny, int nx) {
    qnt::Layout l;
    return qnt::layout(B, n_max, nz, ny, nx, l) ? l.total : 0;
}

MCAV_EXPORT int mcav_cloud_occupancy(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float vx,
                                     float vy, float vz, int nx, int ny, int nz, float sigma2, float* canvas, int* point_count,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    const qnt::Grid g{x0, y0, z0, vx, vy, vz, nx, ny, nz};
    const int refused = qnt::forward_refusal(points, offsets, B, n_max, g, sigma2, canvas, point_count, workspace, workspace_bytes);
    if (refused) return refused;
    qnt::Layout l;
    qnt::layout(B, n_max, nz, ny, nx, l);
    // a tile of 64 bins is 128 KB of sums: allowed once for the largest, which covers every smaller request
    static const bool allowed = allow_dynamic_lds(sizeof(unsigned long long) * qnt::MAX_NZ * qnt::TILE_COLS, qnt::qnt_canvas_kernel<true>,
                                                  qnt::qnt_canvas_kernel<false>) &&
                                allow_dynamic_lds(sizeof(unsigned) * qnt::MAX_NZ * qnt::TILE_COLS, qnt::qnt_count_kernel);
    if (!allowed) return MCAV_E_LAUNCH;

    char* ws = reinterpret_cast<char*>(workspace);
    unsigned* cells = reinterpret_cast<unsigned*>(ws + l.cells);
    unsigned* tile_sums = reinterpret_cast<unsigned*>(ws + l.tile_sums);
    int2* rec = reinterpret_cast<int2*>(ws + l.rec);
    int* index = reinterpret_cast<int*>(ws + l.index);
    int* cnt = reinterpret_cast<int*>(ws + l.cnt);
    const qnt::f32x4* pts = reinterpret_cast<const qnt::f32x4*>(points);
    const unsigned point_blocks = (unsigned)((n_max + qnt::THREADS - 1) / qnt::THREADS);
    const int tiles_x = (nx + qnt::TILE_X - 1) / qnt::TILE_X, tiles_y = (ny + qnt::TILE_Y - 1) / qnt::TILE_Y;
    const unsigned tiles = (unsigned)B * (unsigned)tiles_x * (unsigned)tiles_y;          // at most B * ny * nx < 2^31
    const size_t cols = (size_t)nz * qnt::TILE_COLS;
    hipStream_t s = as_stream(stream);

    if (hipMemsetAsync(cells, 0, sizeof(unsigned) * (size_t)l.M, s) != hipSuccess) return MCAV_E_LAUNCH;
    if (point_blocks) qnt::qnt_point_kernel<<<point_blocks, qnt::THREADS, 0, s>>>(pts, offsets, B, (int)n_max, g, cells, rec, point_count);
    qnt::qnt_reduce_kernel<<<l.ntiles, qnt::THREADS, 0, s>>>(cells, l.M, tile_sums);
    qnt::qnt_scan_kernel<<<1, 1024, 0, s>>>(tile_sums, l.ntiles, cells, l.M);
    qnt::qnt_apply_kernel<<<l.ntiles, qnt::THREADS, 0, s>>>(cells, l.M, tile_sums);
    if (point_blocks) {
        qnt::qnt_fill_kernel<<<point_blocks, qnt::THREADS, 0, s>>>(rec, offsets, B, (int)n_max, cells, index);
        qnt::qnt_count_kernel<<<tiles, qnt::THREADS, sizeof(unsigned) * cols, s>>>(pts, cells, index, g, tiles_x, tiles_y, cnt, point_count);
    }
    if (nx % 4 == 0)
        qnt::qnt_canvas_kernel<true><<<tiles, qnt::THREADS, sizeof(unsigned long long) * cols, s>>>(pts, cells, index, cnt, g, sigma2, tiles_x,
                                                                                                    tiles_y, canvas);
    else
        qnt::qnt_canvas_kernel<false><<<tiles, qnt::THREADS, sizeof(unsigned long long) * cols, s>>>(pts, cells, index, cnt, g, sigma2, tiles_x,
                                                                                                     tiles_y, canvas);
    return launch_status();
}

MCAV_EXPORT int mcav_cloud_occupancy_bwd(const float* points, const int* offsets, const int* point_count, const float* d_canvas, int B,
                                         long long n_max, float x0, float y0, float z0, float vx, float vy, float vz, int nx, int ny, int nz,
                                         float sigma2, float* d_points, void* stream) {
    const qnt::Grid g{x0, y0, z0, vx, vy, vz, nx, ny, nz};
    const int refused = qnt::backward_refusal(points, offsets, point_count, d_canvas, B, n_max, g, sigma2, d_points);
    if (refused) return refused;
    const unsigned blocks = (unsigned)((n_max + qnt::THREADS - 1) / qnt::THREADS);
    if (blocks)
        qnt::qnt_bwd_kernel<<<blocks, qnt::THREADS, 0, as_stream(stream)>>>(reinterpret_cast<const qnt::f32x4*>(points), offsets, point_count, d_canvas,
                                                                         B, (int)n_max, g, sigma2, reinterpret_cast<qnt::f32x4*>(d_points));
    return launch_status();
}
