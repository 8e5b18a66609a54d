// Metric scale of a monocular prediction from the ground plane (include/mcav_depth.h: mcav_ground_scale; DNet's dense geometrical
// constraint).  Definition: tests/ground_scale_ref.py.  Per-pixel math: ground_math.h.
//
// Two launches on the caller's stream, no host synchronisation, no allocation, no copy (the call can be captured):
//   pixel    one workgroup per 8 x 32 tile of one image's INTERIOR (the border has no 3x3 neighbourhood and is never ground): the rays of
//            the tile's rows and columns are formed in float64 from the calibration record, the tile's points plus a one-pixel halo are
//            staged in LDS (each depth converted once instead of nine times), each thread forms its pixel's key -- the bits of hgt, which
//            order positive floats, or 0xFFFFFFFF -- and stores it to the workspace, with the optional mask byte (the threads next to
//            the border write the border's zeros).
//   select   one workgroup per image: exact radix select, 11 + 11 + 10 bits, of the ranks floor((n-1)/2) and n/2 among the image's ground
//            keys, three passes over the stored keys with the histograms in LDS (eval_depth.hip's scheme, its global histogram and its
//            extra launches left out: nothing crosses a workgroup, so no hand-off and no zero-filled state); thread 0 writes the row.
// LDS integer atomics only (counts: exact in any order): rows and mask are bit-identical from run to run.
#include "block_ops.h"
#include "ground_math.h"

namespace mcav {
namespace gs {

constexpr int TILE_H = 8, TILE_W = 32, THREADS = TILE_H * TILE_W;
constexpr int HALO_H = TILE_H + 2, HALO_W = TILE_W + 2;
constexpr int SEL_THREADS = 1024, SEL_WAVES = SEL_THREADS / 64, BINS = RADIX_BINS;

struct Args {
    const float* m;                      // [B, h, w]
    const int* sizes;                    // [B, 2]
    const double* calib;                 // [B, 28], P first
    const int* boxes;                    // [B, 4] or null
    int h, w, tiles_x, tiles_y;
    float camera_height, cos_max, fallback;
    int min_ground, input_depth;
    float* rows;                         // [B, 4]
    unsigned char* mask;                 // [B, h, w] or null
    unsigned* keys;                      // [B, (h - 2) * (w - 2)]
};

__global__ __launch_bounds__(THREADS) void gs_pixel_kernel(Args a) {
    __shared__ float s_xn[HALO_W], s_yn[HALO_H];
    __shared__ float s_X[HALO_H][HALO_W], s_Y[HALO_H][HALO_W], s_Z[HALO_H][HALO_W];
    const int per_image = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / per_image, t = blockIdx.x - b * per_image;
    const int ty0 = (t / a.tiles_x) * TILE_H, tx0 = (t % a.tiles_x) * TILE_W;      // the halo's origin; the tile's is one further on each axis
    const int tid = threadIdx.x;
    const double* P = a.calib + (size_t)b * 28;
    if (tid < HALO_W) {
        const int c = min(tx0 + tid, a.w - 1);
        s_xn[tid] = ray(c, a.sizes[2 * b + 1], a.w, P[2], P[0]);
    } else if (tid >= 64 && tid < 64 + HALO_H) {
        const int r = min(ty0 + tid - 64, a.h - 1);
        s_yn[tid - 64] = ray(r, a.sizes[2 * b], a.h, P[4 + 2], P[4 + 1]);
    }
    __syncthreads();
    const float* mp = a.m + (size_t)b * a.h * a.w;
    for (int i = tid; i < HALO_H * HALO_W; i += THREADS) {
        const int hr = i / HALO_W, hc = i - hr * HALO_W;
        const int r = min(ty0 + hr, a.h - 1), c = min(tx0 + hc, a.w - 1);              // clamped: no read outside the plane
        const float d = depth_of(mp[(size_t)r * a.w + c], a.input_depth != 0);
        s_X[hr][hc] = mul(s_xn[hc], d);
        s_Y[hr][hc] = mul(s_yn[hr], d);
        s_Z[hr][hc] = d;
    }
    __syncthreads();
    const int lr = tid / TILE_W, lc = tid - lr * TILE_W;
    const int r = ty0 + 1 + lr, c = tx0 + 1 + lc;
    if (r > a.h - 2 || c > a.w - 2) return;                                            // a partial tile; no barrier follows
    float X[9], Y[9], Z[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        X[k] = s_X[lr + k / 3][lc + k % 3];
        Y[k] = s_Y[lr + k / 3][lc + k % 3];
        Z[k] = s_Z[lr + k / 3][lc + k % 3];
    }
    float hgt;
    const Box box = clamp_box(a.boxes ? a.boxes + 4 * b : nullptr, a.h, a.w);
    const bool g = ground_pixel(X, Y, Z, a.cos_max, hgt) && in_box(box, r, c);
    a.keys[(size_t)b * (a.h - 2) * (a.w - 2) + (size_t)(r - 1) * (a.w - 2) + (c - 1)] = pixel_key(g, hgt);
    if (a.mask) {
        unsigned char* mk = a.mask + (size_t)b * a.h * a.w;
        // the border pixel (rr, cc) is written by the interior pixel nearest to it
        const int r_lo = r == 1 ? 0 : r, r_hi = r == a.h - 2 ? a.h - 1 : r;
        const int c_lo = c == 1 ? 0 : c, c_hi = c == a.w - 2 ? a.w - 1 : c;
        for (int rr = r_lo; rr <= r_hi; ++rr)
            for (int cc = c_lo; cc <= c_hi; ++cc) mk[(size_t)rr * a.w + cc] = (rr == r && cc == c && g) ? 1 : 0;
    }
}

// One digit into an LDS histogram.  The heights of a road lie close together, so most lanes of a wave carry the same digit and a plain
// atomicAdd per lane would be served one lane at a time: up to four rounds in which the lanes that share the first lane's digit add their
// number at once, then the rest one by one.  Called by whole waves (take = false for a lane without a key).
__device__ __forceinline__ void hist_add(unsigned* bins, bool take, unsigned d) {
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < 4; ++round) {
        const unsigned long long act = __ballot(take);
        if (!act) return;
        const int leader = __ffsll((long long)act) - 1;
        const unsigned dl = (unsigned)__shfl((int)d, leader, 64);
        const bool same = take && d == dl;
        const unsigned long long sm = __ballot(same);
        if (lane == leader) atomicAdd(&bins[dl], (unsigned)__popcll(sm));
        take = take && !same;
    }
    if (take) atomicAdd(&bins[d], 1u);
}

__global__ __launch_bounds__(SEL_THREADS) void gs_select_kernel(Args a) {
    __shared__ unsigned lh[2][BINS];
    __shared__ unsigned wtot[SEL_WAVES];
    __shared__ unsigned s_pre[2], s_left[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned count = 0;                                    // the number of ground pixels, in every thread
    const unsigned n = (unsigned)(a.h - 2) * (unsigned)(a.w - 2);
    const unsigned* kb = a.keys + (size_t)b * n;
    for (int p = 0; p < RADIX_PASSES; ++p) {
        for (int i = tid; i < 2 * BINS; i += SEL_THREADS) (&lh[0][0])[i] = 0u;
        __syncthreads();                                   // (also: every thread has read the previous pass's state)
        const auto [shift, dmask, pmask] = radix_pass(p);
        const unsigned pre0 = p ? s_pre[0] & pmask : 0u, pre1 = p ? s_pre[1] & pmask : 0u;
        const bool two = p && pre0 != pre1;                // neighbouring ranks nearly always share their prefix: one histogram serves both
        for (unsigned base = 0; base < n; base += SEL_THREADS) {      // uniform over the workgroup
            const unsigned i = base + (unsigned)tid;
            const unsigned key = i < n ? kb[i] : NOT_GROUND;
            const bool gnd = key != NOT_GROUND;
            const unsigned d = (key >> shift) & dmask;
            hist_add(lh[0], gnd && (key & pmask) == pre0, d);
            if (two) hist_add(lh[1], gnd && (key & pmask) == pre1, d);      // (uniform; pass 0: every key matches both ranks)
        }
        __syncthreads();
        if (p == 0) {                                      // the sum of every bin
            count = block_sum<unsigned, SEL_WAVES>(lh[0][2 * tid] + lh[0][2 * tid + 1], wtot);
            if (count == 0) break;                         // uniform
        }
        unsigned pick[2] = {0u, 0u}, left[2] = {0u, 0u};
        bool mine[2];
        for (int r = 0; r < 2; ++r) {
            const unsigned* src = lh[two ? r : 0];
            const unsigned c[2] = {src[2 * tid], src[2 * tid + 1]};
            const unsigned k = p ? s_left[r] : (r == 0 ? (count - 1) / 2 : count / 2);
            mine[r] = pick_bin<2, SEL_WAVES>(c, k, wtot, pick[r], left[r]);
        }
        __syncthreads();                                   // every thread has read the state
        for (int r = 0; r < 2; ++r)
            if (mine[r]) {
                s_pre[r] = (p ? s_pre[r] : 0u) | (pick[r] << shift);
                s_left[r] = left[r];
            }
        __syncthreads();
    }
    if (tid == 0) {
        float row[4];
        image_row(count, count ? ev::bits_float(s_pre[0]) : 0.0f, count ? ev::bits_float(s_pre[1]) : 0.0f, a.camera_height, a.min_ground,
                  a.fallback, row);
        for (int k = 0; k < 4; ++k) a.rows[4 * b + k] = row[k];
    }
}

inline bool shape_ok(int B, int h, int w) {
    return B > 0 && h >= 3 && w >= 3 && (unsigned long long)B * h * w < 0x80000000ull;
}
inline size_t keys_bytes(int B, int h, int w) { return align_up(sizeof(unsigned) * (size_t)B * (h - 2) * (w - 2), 256); }

}  // namespace gs
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_ground_scale_workspace_bytes(int B, int h, int w) { return gs::shape_ok(B, h, w) ? gs::keys_bytes(B, h, w) : 0; }

MCAV_EXPORT int mcav_ground_scale(const float* m, int B, int h, int w, const int* sizes, const double* calib, const int* boxes,
                                  float camera_height, float cos_max, int min_ground, float fallback, int flags, float* rows,
                                  unsigned char* mask_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || !sizes || !calib || !rows || !workspace) return MCAV_E_INVALID;
    if (!gs::shape_ok(B, h, w) || !gs::scalars_ok(camera_height, cos_max, min_ground, flags)) return MCAV_E_INVALID;
    if (workspace_bytes < gs::keys_bytes(B, h, w)) return MCAV_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return MCAV_E_INVALID;
    gs::Args a;
    a.m = m; a.sizes = sizes; a.calib = calib; a.boxes = boxes;
    a.h = h; a.w = w;
    a.tiles_x = (w - 2 + gs::TILE_W - 1) / gs::TILE_W;
    a.tiles_y = (h - 2 + gs::TILE_H - 1) / gs::TILE_H;
    a.camera_height = camera_height; a.cos_max = cos_max; a.fallback = fallback;
    a.min_ground = min_ground;
    a.input_depth = (flags & MCAV_GS_INPUT_DEPTH) ? 1 : 0;
    a.rows = rows; a.mask = mask_out;
    a.keys = reinterpret_cast<unsigned*>(workspace);
    hipStream_t s = as_stream(stream);
    gs::gs_pixel_kernel<<<B * a.tiles_x * a.tiles_y, gs::THREADS, 0, s>>>(a);
    gs::gs_select_kernel<<<B, gs::SEL_THREADS, 0, s>>>(a);
    return launch_status();
}
