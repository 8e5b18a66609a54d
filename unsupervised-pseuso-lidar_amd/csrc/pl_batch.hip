// Batched network output -> float32 pseudo-LiDAR clouds (include/mcav_depth.h: mcav_pl_batch_project; the definition is
// tests/pl_batch_ref.py).  Per image of a batch: the evaluation protocol's resize of the disparity to the calibration's resolution
// (eval_math.h), pl_point's float64 un-projection into the velodyne frame (pl_math.h), the height / depth / half-space cut, and either
//   dense : an order-preserving compaction over (image, pixel) -- count per 256-pixel block, scan, scatter with the ballot rank
//   beams : one return per (image, beam, azimuth) cell -- a 64-bit integer atomicMin of (range bits << 32 | pixel) per survivor, then the
//           same count / scan / scatter over the cells
// Every pass recomputes the point instead of storing it (4 B read per network pixel, 16 B written per point); nothing returns to the host,
// no copy from the host and no allocation: the call can be captured.  No float atomics: bit-identical from run to run.
// mcav_pl_batch_project_indexed is the same sequence with one more store in the scatter: the pixel behind every row, which is all the
// backward (pl_bwd.hip) needs to know of the selection.
#include "block_ops.h"
#include "pl_math.h"

namespace mcav {
namespace plb {

constexpr int THREADS = 256;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Args {
    const float* m;                      // [B, h, w]
    const float* intensity;              // [B, h, w] or null
    const int* sizes;                    // [B, 2] (Hb, Wb)
    const PLCalib* calib;                // [B]
    const double* elev;                  // [nb + 1] or null
    const double* azim;                  // [na + 1] or null
    int h, w, Hg, Wg, nb, na;
    int per_image;                       // blocks per image of the pixel passes
    float scale;
    const float* scales;                 // [B] or null: the image's scale is scale * scales[b]
    double max_height, max_depth;
    int input_depth;
};

// P (12 doubles) + T (16 doubles) per image -> PLCalib, on the device: the table arrives in a device buffer
__global__ __launch_bounds__(THREADS) void plb_calib_kernel(const double* records, int B, PLCalib* out) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    PLCalib c;
    pl_calib(records + (size_t)b * 28 + 12, records + (size_t)b * 28, c);
    out[b] = c;
}

// The scale of image b.  With a table (mcav_pl_batch_project_scaled) it is scale * scales[b], formed once in float32, and an image whose
// scale is not finite and positive keeps no pixel (false).
__device__ __forceinline__ bool image_scale(const Args& a, int b, float& s) {
    s = a.scale;
    if (!a.scales) return true;
    s = mul(a.scale, a.scales[b]);
    return s > 0.0f && s <= 3.40282346638528859812e+38f;
}

// Pixel p of image b's padded grid: its depth and point.  false: outside the true image (or an image without a usable scale).
__device__ __forceinline__ bool pixel_point(const Args& a, int b, unsigned p, float& d, double (&q)[3], int& r, int& c) {
    if (p >= (unsigned)a.Hg * (unsigned)a.Wg) return false;
    r = (int)(p / (unsigned)a.Wg);
    c = (int)(p - (unsigned)r * (unsigned)a.Wg);
    const int Hb = min(a.sizes[2 * b], a.Hg), Wb = min(a.sizes[2 * b + 1], a.Wg);       // clamped: no read outside the plane
    if (r >= Hb || c >= Wb) return false;
    float s;
    if (!image_scale(a, b, s)) return false;
    d = depth_of(sample(a.m + (size_t)b * a.h * a.w, a.h, a.w, Hb, Wb, r, c), s, a.input_depth != 0);
    pl_point_at((double)d, r, c, a.calib[b], q);
    return true;
}

__device__ __forceinline__ bool pixel_survives(const Args& a, int b, unsigned p, float& d, double (&q)[3], int& r, int& c) {
    return pixel_point(a, b, p, d, q, r, c) && keep(q, d, a.max_height, a.max_depth);
}

__device__ __forceinline__ float pixel_intensity(const Args& a, int b, int r, int c) {
    if (!a.intensity) return 0.0f;
    const int Hb = min(a.sizes[2 * b], a.Hg), Wb = min(a.sizes[2 * b + 1], a.Wg);
    return sample(a.intensity + (size_t)b * a.h * a.w, a.h, a.w, Hb, Wb, r, c);
}

__global__ __launch_bounds__(THREADS) void plb_count_kernel(Args a, unsigned* counts) {
    __shared__ unsigned wsum[THREADS / 64];
    const int b = blockIdx.x / a.per_image;
    const unsigned p = (unsigned)(blockIdx.x - b * a.per_image) * THREADS + threadIdx.x;
    float d;
    double q[3];
    int r, c;
    const unsigned n = block_count<THREADS / 64>(pixel_survives(a, b, p, d, q, r, c), wsum);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// Exclusive scan of the per-block counts in one block (1024 entries per pass), total -> counts[nblocks]; then the images' slices:
// offsets[b] = rows before image b, an image of n survivors owning ceil(n / step) rows.
__global__ __launch_bounds__(1024) void plb_scan_kernel(unsigned* counts, int nblocks, int per_image, int B, unsigned step, int* offsets) {
    __shared__ unsigned wsum[16];
    const unsigned total = chunked_scan<unsigned, 16>(nblocks, wsum, [&](int i) { return counts[i]; }, [&](int i, unsigned v) { counts[i] = v; });
    __syncthreads();                                   // thread 0 reads what the others stored
    if (threadIdx.x == 0) {
        counts[nblocks] = total;
        unsigned rows = 0;
        for (int b = 0; b < B; ++b) {
            offsets[b] = (int)rows;
            const unsigned n = counts[(size_t)(b + 1) * per_image] - counts[(size_t)b * per_image];
            rows += (n + step - 1) / step;
        }
        offsets[B] = (int)rows;
    }
}

// pixels (or null): pixels[o] = the pixel of the image's padded grid that became row o (mcav_pl_batch_project_indexed)
__global__ __launch_bounds__(THREADS) void plb_scatter_kernel(Args a, const unsigned* scan, const int* offsets, unsigned step, f32x4* cloud,
                                                              size_t capacity, int* pixels) {
    __shared__ unsigned wsum[THREADS / 64];
    const int b = blockIdx.x / a.per_image;
    const unsigned p = (unsigned)(blockIdx.x - b * a.per_image) * THREADS + threadIdx.x;
    float d;
    double q[3];
    int r, c;
    const bool v = pixel_survives(a, b, p, d, q, r, c);
    const unsigned k = (scan[blockIdx.x] - scan[(size_t)b * a.per_image]) + block_rank<THREADS / 64>(v, wsum);       // rank among the image's survivors
    if (v && k % step == 0) {
        const size_t o = (size_t)offsets[b] + k / step;
        if (o < capacity) {
            f32x4 row;
            row[0] = (float)q[0]; row[1] = (float)q[1]; row[2] = (float)q[2]; row[3] = pixel_intensity(a, b, r, c);
            cloud[o] = row;
            if (pixels) pixels[o] = (int)p;
        }
    }
}

// ---------------------------------------------------------------------------------------------- beams
__global__ __launch_bounds__(THREADS) void plb_bin_kernel(Args a, unsigned long long* cells) {
    const int b = blockIdx.x / a.per_image;
    const unsigned p = (unsigned)(blockIdx.x - b * a.per_image) * THREADS + threadIdx.x;
    float d;
    double q[3];
    int r, c, beam, az;
    if (!pixel_survives(a, b, p, d, q, r, c)) return;
    if (!beam_cell(q, a.elev, a.nb, a.azim, a.na, beam, az)) return;
    atomicMin(cells + ((size_t)b * a.nb + beam) * a.na + az, cell_word(range_key(q), p));
}

// cell passes: per_cells blocks per image over its nb * na cells
__device__ __forceinline__ bool cell_filled(const Args& a, const unsigned long long* cells, int per_cells, int& b, unsigned long long& word) {
    b = blockIdx.x / per_cells;
    const unsigned i = (unsigned)(blockIdx.x - b * per_cells) * THREADS + threadIdx.x, n = (unsigned)a.nb * (unsigned)a.na;
    if (i >= n) return false;
    word = cells[(size_t)b * n + i];
    return word != EMPTY_CELL;
}

__global__ __launch_bounds__(THREADS) void plb_cell_count_kernel(Args a, const unsigned long long* cells, int per_cells, unsigned* counts) {
    __shared__ unsigned wsum[THREADS / 64];
    int b;
    unsigned long long word;
    const unsigned n = block_count<THREADS / 64>(cell_filled(a, cells, per_cells, b, word), wsum);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

__global__ __launch_bounds__(THREADS) void plb_cell_scatter_kernel(Args a, const unsigned long long* cells, int per_cells, const unsigned* scan,
                                                                   f32x4* cloud, size_t capacity, int* pixels) {
    __shared__ unsigned wsum[THREADS / 64];
    int b;
    unsigned long long word = EMPTY_CELL;
    const bool v = cell_filled(a, cells, per_cells, b, word);
    const size_t o = (size_t)scan[blockIdx.x] + block_rank<THREADS / 64>(v, wsum);
    if (v && o < capacity) {
        float d;
        double q[3];
        int r, c;
        if (pixel_point(a, b, (unsigned)(word & 0xffffffffull), d, q, r, c)) {       // always: the bin pass wrote this pixel
            f32x4 row;
            row[0] = (float)q[0]; row[1] = (float)q[1]; row[2] = (float)q[2]; row[3] = pixel_intensity(a, b, r, c);
            cloud[o] = row;
            if (pixels) pixels[o] = r * a.Wg + c;
        }
    }
}

struct Layout {
    size_t calib, counts, cells, total;
    int per_image, per_cells;
};

inline bool layout(int B, int Hg, int Wg, int nb, int na, Layout& l) {
    if (B <= 0 || Hg <= 0 || Wg <= 0 || nb < 0 || na < 0 || (nb == 0) != (na == 0)) return false;
    const unsigned long long px = (unsigned long long)Hg * Wg, cl = (unsigned long long)nb * na;
    if (px * B > 0x7fffffffull || cl * B > 0x7fffffffull) return false;       // int32 offsets, 32-bit pixel indices, one grid dimension
    l.per_image = (int)((px + THREADS - 1) / THREADS);
    l.per_cells = (int)((cl + THREADS - 1) / THREADS);
    const size_t nblocks = (size_t)B * (l.per_image > l.per_cells ? l.per_image : l.per_cells);
    l.calib = 0;
    l.counts = l.calib + align_up(sizeof(PLCalib) * B, 256);
    l.cells = l.counts + align_up(sizeof(unsigned) * (nblocks + 1), 256);
    l.total = l.cells + align_up(sizeof(unsigned long long) * cl * B, 256);
    return true;
}

}  // namespace plb
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_pl_batch_workspace_bytes(int B, int Hg, int Wg, int n_beams, int n_azimuth) {
    plb::Layout l;
    return plb::layout(B, Hg, Wg, n_beams, n_azimuth, l) ? l.total : 0;
}

MCAV_EXPORT int mcav_pl_beam_tables_check(const double* elev_host, int n_beams, const double* azim_host, int n_azimuth) {
    return plb::table_ok(elev_host, n_beams) && plb::table_ok(azim_host, n_azimuth) ? MCAV_OK : MCAV_E_INVALID;
}

// the three entries' body; pixels: null, or device int [capacity_points]
static int project(const float* m, int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib, const float* intensity,
                   const double* elev, const double* azim, int n_beams, int n_azimuth, float scale, const float* scales, double max_height,
                   double max_depth, int sparsity, int flags, float* cloud, size_t capacity_points, int* offsets, int* pixels, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (!m || !sizes || !calib || !cloud || !offsets || !workspace || h <= 0 || w <= 0 || sparsity < 0) return MCAV_E_INVALID;
    if (flags & ~MCAV_PLB_INPUT_DEPTH) return MCAV_E_INVALID;
    if ((elev != nullptr) != (azim != nullptr) || (elev != nullptr) != (n_beams > 0)) return MCAV_E_INVALID;
    if ((unsigned long long)h * w * (unsigned long long)(B > 0 ? B : 0) > 0x7fffffffull) return MCAV_E_INVALID;
    if (reinterpret_cast<uintptr_t>(cloud) & 15) return MCAV_E_INVALID;                  // one 16-byte store per point
    if (!(scale == scale) || max_height != max_height || max_depth != max_depth) return MCAV_E_INVALID;
    plb::Layout l;
    if (!plb::layout(B, Hg, Wg, n_beams, n_azimuth, l)) return MCAV_E_INVALID;
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return MCAV_E_INVALID;

    char* ws = reinterpret_cast<char*>(workspace);
    PLCalib* cal = reinterpret_cast<PLCalib*>(ws + l.calib);
    unsigned* counts = reinterpret_cast<unsigned*>(ws + l.counts);
    unsigned long long* cells = reinterpret_cast<unsigned long long*>(ws + l.cells);
    plb::Args a;
    a.m = m; a.intensity = intensity; a.sizes = sizes; a.calib = cal; a.elev = elev; a.azim = azim;
    a.h = h; a.w = w; a.Hg = Hg; a.Wg = Wg; a.nb = n_beams; a.na = n_azimuth;
    a.per_image = l.per_image;
    a.scale = scale; a.scales = scales; a.max_height = max_height; a.max_depth = max_depth;
    a.input_depth = (flags & MCAV_PLB_INPUT_DEPTH) ? 1 : 0;
    plb::f32x4* out = reinterpret_cast<plb::f32x4*>(cloud);
    hipStream_t s = as_stream(stream);
    const int npix = B * l.per_image;

    plb::plb_calib_kernel<<<(B + plb::THREADS - 1) / plb::THREADS, plb::THREADS, 0, s>>>(calib, B, cal);
    if (!elev) {
        const unsigned step = sparsity > 0 ? (unsigned)sparsity : 1u;
        plb::plb_count_kernel<<<npix, plb::THREADS, 0, s>>>(a, counts);
        plb::plb_scan_kernel<<<1, 1024, 0, s>>>(counts, npix, l.per_image, B, step, offsets);
        plb::plb_scatter_kernel<<<npix, plb::THREADS, 0, s>>>(a, counts, offsets, step, out, capacity_points, pixels);
        return launch_status();
    }
    const int ncell = B * l.per_cells;
    if (hipMemsetAsync(cells, 0xff, sizeof(unsigned long long) * (size_t)B * n_beams * n_azimuth, s) != hipSuccess) return MCAV_E_LAUNCH;
    plb::plb_bin_kernel<<<npix, plb::THREADS, 0, s>>>(a, cells);
    plb::plb_cell_count_kernel<<<ncell, plb::THREADS, 0, s>>>(a, cells, l.per_cells, counts);
    plb::plb_scan_kernel<<<1, 1024, 0, s>>>(counts, ncell, l.per_cells, B, 1u, offsets);
    plb::plb_cell_scatter_kernel<<<ncell, plb::THREADS, 0, s>>>(a, cells, l.per_cells, counts, out, capacity_points, pixels);
    return launch_status();
}

MCAV_EXPORT int mcav_pl_batch_project_scaled(const float* m, int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib,
                                             const float* intensity, const double* elev, const double* azim, int n_beams, int n_azimuth,
                                             float scale, const float* scales, double max_height, double max_depth, int sparsity, int flags,
                                             float* cloud, size_t capacity_points, int* offsets, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    return project(m, B, h, w, Hg, Wg, sizes, calib, intensity, elev, azim, n_beams, n_azimuth, scale, scales, max_height, max_depth, sparsity,
                   flags, cloud, capacity_points, offsets, nullptr, workspace, workspace_bytes, stream);
}

MCAV_EXPORT int mcav_pl_batch_project_indexed(const float* m, int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib,
                                              const float* intensity, const double* elev, const double* azim, int n_beams, int n_azimuth,
                                              float scale, const float* scales, double max_height, double max_depth, int sparsity, int flags,
                                              float* cloud, size_t capacity_points, int* offsets, int* pixels, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    if (!pixels) return MCAV_E_INVALID;
    return project(m, B, h, w, Hg, Wg, sizes, calib, intensity, elev, azim, n_beams, n_azimuth, scale, scales, max_height, max_depth, sparsity,
                   flags, cloud, capacity_points, offsets, pixels, workspace, workspace_bytes, stream);
}

MCAV_EXPORT int mcav_pl_batch_project(const float* m, int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib,
                                      const float* intensity, const double* elev, const double* azim, int n_beams, int n_azimuth,
                                      float scale, double max_height, double max_depth, int sparsity, int flags, float* cloud,
                                      size_t capacity_points, int* offsets, void* workspace, size_t workspace_bytes, void* stream) {
    return mcav_pl_batch_project_scaled(m, B, h, w, Hg, Wg, sizes, calib, intensity, elev, azim, n_beams, n_azimuth, scale, nullptr,
                                        max_height, max_depth, sparsity, flags, cloud, capacity_points, offsets, workspace, workspace_bytes,
                                        stream);
}
