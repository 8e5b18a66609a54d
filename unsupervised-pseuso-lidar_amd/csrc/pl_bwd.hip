// The gradient's way back from pillar voxels to the network's plane (include/mcav_depth.h: mcav_pillarize_bwd,
// mcav_pl_batch_project_bwd; the definition is tests/pl_bwd_ref.py, the arithmetic csrc/pl_bwd_math.h).  Both forwards select: a pixel
// becomes a cloud row or not, a row a pillar slot or not.  The indexed forwards record that selection (pixels, slot_points), and every
// destination here has at most one source, so both backwards are plain scatters through it, and the resize's adjoint is a gather:
//   pillarize_bwd : memset d_points; one wavefront per pillar, its gradient block through LDS, the column sums of the mean's derivative
//                   in float64 in slot order, one 16-byte store per used slot
//   project_bwd   : memset G [B, Hg, Wg]; a) one thread per cloud row: the plane value resampled, dq/dd, dd/dv, one store into the row's
//                   pixel of G; b) one thread per element of m: the float64 sum over the outputs whose taps touch it, in ascending order
// No atomics, nothing returns to the host, no allocation: the calls can be captured, and two runs give the same bytes.
#include "mcav_common.h"
#include "pl_bwd_math.h"

namespace mcav {
namespace plg {

constexpr int THREADS = 256;
constexpr int PILLAR_BLOCKS = 8192;              // as pillarize.hip's gather: single-wave blocks, the pillars beyond by the grid's stride

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int C>
__global__ __launch_bounds__(64) void pil_bwd_kernel(const float* d_voxels, const int* slot_points, const int* num_points,
                                                     const int* pillar_offsets, int B, int N, size_t capacity, f32x4* d_points, int n_max) {
    __shared__ float tile[pil::MAX_POINTS * C];
    const int lane = threadIdx.x;
    const size_t total_pillars = (size_t)max(pillar_offsets[B], 0);
    const size_t P = total_pillars < capacity ? total_pillars : capacity;
    for (size_t r = blockIdx.x; r < P; r += gridDim.x) {
        const int total = N * C;
        const float* in = d_voxels + r * (size_t)total;
        for (int e = lane; e < total; e += 64) tile[e] = in[e];
        __syncthreads();
        const int count = min(max(num_points[r], 0), N);
        if (lane < count) {
            const int i = slot_points[r * (size_t)N + lane];
            if (i >= 0 && i < n_max) {                     // the forward's own rows; anything else writes nowhere
                const float* g = tile + lane * C;
                f32x4 row;
#pragma unroll
                for (int col = 0; col < 4; ++col)
                    row[col] = point_grad(g, C, col, C == pil::COLS_DECORATED && col < 3 ? column_sum(tile + 4 + col, C, count) : 0.0, count);
                d_points[i] = row;
            }
        }
        __syncthreads();                                   // the next pillar reuses tile
    }
}

struct PlaneArgs {
    const float* m;                      // [B, h, w]
    const int* sizes;                    // [B, 2]
    const double* calib;                 // [B, 28]: P (12), T (16)
    const float* scales;                 // [B] or null
    int B, h, w, Hg, Wg;
    float scale;
    int input_depth;
};

// a) cloud row o -> its pixel of G
__global__ __launch_bounds__(THREADS) void plb_bwd_rows_kernel(PlaneArgs a, const f32x4* d_points, const int* pixels, const int* offsets,
                                                               size_t capacity, float* G) {
    const size_t o = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const size_t rows = (size_t)max(offsets[a.B], 0);
    if (o >= capacity || o >= rows) return;
    const int b = pil::image_of(offsets, a.B, (int)o);
    const int p = pixels[o];
    if (p < 0 || (long long)p >= (long long)a.Hg * a.Wg) return;
    const int r = p / a.Wg, c = p - r * a.Wg;
    const int Hb = min(a.sizes[2 * b], a.Hg), Wb = min(a.sizes[2 * b + 1], a.Wg);       // clamped as the forward clamps them
    if (r >= Hb || c >= Wb) return;
    float s;
    if (!image_scale(a.scale, a.scales, b, s)) return;
    PLCalib k;
    pl_calib(a.calib + (size_t)b * 28 + 12, a.calib + (size_t)b * 28, k);
    const float v = plb::sample(a.m + (size_t)b * a.h * a.w, a.h, a.w, Hb, Wb, r, c);
    const f32x4 g = d_points[o];
    const float g3[3] = {g[0], g[1], g[2]};
    G[((size_t)b * a.Hg + r) * a.Wg + c] = plane_grad(g3, v, s, a.input_depth != 0, r, c, k);
}

// b) element (b, y, x) of d_m <- the outputs of G whose taps touch it
__global__ __launch_bounds__(THREADS) void plb_bwd_plane_kernel(PlaneArgs a, const float* G, float* d_m) {
    const size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const size_t per = (size_t)a.h * a.w;
    if (e >= per * a.B) return;
    const int b = (int)(e / per);
    const int y = (int)((e - b * per) / a.w), x = (int)(e - b * per - (size_t)y * a.w);
    const int Hb = min(a.sizes[2 * b], a.Hg), Wb = min(a.sizes[2 * b + 1], a.Wg);
    float s, out = 0.0f;
    // every read of G lies inside the image's (Hb, Wb) <= (Hg, Wg): the windows end at Hb - 1 and Wb - 1, the direct read has h == Hb
    if (image_scale(a.scale, a.scales, b, s) && Hb >= 1 && Wb >= 1)
        out = resize_adjoint(G + (size_t)b * a.Hg * a.Wg, a.Wg, a.h, a.w, Hb, Wb, y, x);
    d_m[e] = out;
}

inline bool plane_layout(int B, int Hg, int Wg, size_t& bytes) {
    if (B <= 0 || Hg <= 0 || Wg <= 0) return false;
    const unsigned long long px = (unsigned long long)Hg * Wg;
    if (px * B > 0x7fffffffull) return false;
    bytes = align_up(sizeof(float) * (size_t)px * B, 256);
    return true;
}

}  // namespace plg
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT int mcav_pillarize_bwd(const float* d_voxels, const int* slot_points, const int* num_points, const int* pillar_offsets, int B,
                                   long long capacity, int max_points, int flags, float* d_points, long long n_max, void* stream) {
    if (!d_voxels || !slot_points || !num_points || !pillar_offsets || !d_points) return MCAV_E_INVALID;
    if (B <= 0 || B > 65535 || n_max < 0 || n_max > 0x7fffffffll || capacity < 0) return MCAV_E_INVALID;
    if (max_points < 1 || max_points > pil::MAX_POINTS || (flags & ~MCAV_PILLAR_DECORATE)) return MCAV_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_points) & 15) || (reinterpret_cast<uintptr_t>(d_voxels) & 3)) return MCAV_E_INVALID;
    hipStream_t s = as_stream(stream);
    if (n_max && hipMemsetAsync(d_points, 0, sizeof(float) * 4 * (size_t)n_max, s) != hipSuccess) return MCAV_E_LAUNCH;
    const size_t rows = (size_t)capacity < (size_t)n_max ? (size_t)capacity : (size_t)n_max;       // a pillar holds at least one row
    if (rows) {
        const unsigned blocks = (unsigned)(rows < (size_t)plg::PILLAR_BLOCKS ? rows : (size_t)plg::PILLAR_BLOCKS);
        plg::f32x4* out = reinterpret_cast<plg::f32x4*>(d_points);
        if (flags & MCAV_PILLAR_DECORATE)
            plg::pil_bwd_kernel<pil::COLS_DECORATED><<<blocks, 64, 0, s>>>(d_voxels, slot_points, num_points, pillar_offsets, B, max_points,
                                                                            (size_t)capacity, out, (int)n_max);
        else
            plg::pil_bwd_kernel<pil::COLS_PLAIN><<<blocks, 64, 0, s>>>(d_voxels, slot_points, num_points, pillar_offsets, B, max_points,
                                                                        (size_t)capacity, out, (int)n_max);
    }
    return launch_status();
}

MCAV_EXPORT size_t mcav_pl_batch_project_bwd_workspace_bytes(int B, int Hg, int Wg) {
    size_t bytes;
    return plg::plane_layout(B, Hg, Wg, bytes) ? bytes : 0;
}

MCAV_EXPORT int mcav_pl_batch_project_bwd(const float* d_points, size_t capacity_points, const int* pixels, const int* offsets, const float* m,
                                          int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib, float scale,
                                          const float* scales, int flags, float* d_m, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d_points || !pixels || !offsets || !m || !sizes || !calib || !d_m || !workspace || h <= 0 || w <= 0) return MCAV_E_INVALID;
    if (flags & ~MCAV_PLB_INPUT_DEPTH) return MCAV_E_INVALID;
    if ((unsigned long long)h * w * (unsigned long long)(B > 0 ? B : 0) > 0x7fffffffull) return MCAV_E_INVALID;
    if (reinterpret_cast<uintptr_t>(d_points) & 15) return MCAV_E_INVALID;                // one 16-byte load per row
    if (!(scale == scale)) return MCAV_E_INVALID;
    size_t bytes;
    if (!plg::plane_layout(B, Hg, Wg, bytes)) return MCAV_E_INVALID;
    if (workspace_bytes < bytes) return MCAV_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return MCAV_E_INVALID;

    float* G = reinterpret_cast<float*>(workspace);
    plg::PlaneArgs a;
    a.m = m; a.sizes = sizes; a.calib = calib; a.scales = scales;
    a.B = B; a.h = h; a.w = w; a.Hg = Hg; a.Wg = Wg;
    a.scale = scale;
    a.input_depth = (flags & MCAV_PLB_INPUT_DEPTH) ? 1 : 0;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(G, 0, sizeof(float) * (size_t)B * Hg * Wg, s) != hipSuccess) return MCAV_E_LAUNCH;
    const size_t most = (size_t)B * Hg * Wg;                                              // a pixel owns at most one row
    const size_t rows = capacity_points < most ? capacity_points : most;
    if (rows)
        plg::plb_bwd_rows_kernel<<<(unsigned)((rows + plg::THREADS - 1) / plg::THREADS), plg::THREADS, 0, s>>>(
            a, reinterpret_cast<const plg::f32x4*>(d_points), pixels, offsets, capacity_points, G);
    const size_t elems = (size_t)B * h * w;
    plg::plb_bwd_plane_kernel<<<(unsigned)((elems + plg::THREADS - 1) / plg::THREADS), plg::THREADS, 0, s>>>(a, G, d_m);
    return launch_status();
}
