// The KITTI depth evaluation protocol with per-image median scaling (monodepth2 evaluate_depth.py): mcav_eval_depth (include/mcav_depth.h).
// Definition: tests/eval_protocol_ref.py.  Per-pixel math: eval_math.h.
//
// Launches, all on the caller's stream, no host synchronisation (the call can be captured in a hipGraph):
//   (init, gather, hist and select run with MCAV_EVAL_MEDIAN_SCALING only)
//   init      zero the per-image counters and histograms in the workspace
//   gather    one pass over each image's crop box of the padded ground truth: mask, bilinear disparity sample, depth; the masked gt and
//             pred values are appended as order-preserving keys to per-image buffers: ballot + popcount per wave, one integer
//             atomic per workgroup to reserve the slots.  The append order varies from run to run, which no median depends on.
//   3 x (hist, select)   exact radix select, 11 + 11 + 10 bits, of the ranks floor((n-1)/2) and n/2 of both key buffers of every image:
//             hist counts the keys that still match each rank's prefix in LDS and adds its bins to the global histogram with integer
//             atomics (exact, any order); select scans the 2048 bins of one (image, buffer) and fixes the next digit of both ranks.
//   metrics   re-reads gt and disparity in the crop box, applies ratio = median(gt) / median(pred) and the clip, and leaves the eleven
//             float64 sums of its tile in a slab (fixed order inside the workgroup)
//   finalize  adds each image's slab entries in a fixed order and writes its row.
// No float atomics anywhere: rows are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include "eval_math.h"
#include "kernel_timer.h"
#include "block_ops.h"

namespace mcav {

constexpr int EV_THREADS = 256;
constexpr int EV_PPT = 8;                              // gather / metrics: pixels per thread, EV_THREADS apart
constexpr int EV_TILE = EV_THREADS * EV_PPT;           // crop-box pixels per workgroup
constexpr int EV_KPT = 16;                             // hist: keys per thread
constexpr int EV_KTILE = EV_THREADS * EV_KPT;          // keys per workgroup
constexpr int EV_BINS = RADIX_BINS;

struct EVBox {
    int y0, y1, x0, x1;      // half-open, inside the true size, inside the padded size
};

// sizes [B,2] (Hb, Wb) and boxes [B,4] (y0, y1, x0, x1) as the caller gave them, clamped: nothing outside [0, Hb) x [0, Wb) is read
__device__ __forceinline__ EVBox ev_box(const int* sizes, const int* boxes, int b, int Hg, int Wg) {
    const int Hb = min(max(sizes[2 * b], 0), Hg), Wb = min(max(sizes[2 * b + 1], 0), Wg);
    EVBox r;
    r.y0 = min(max(boxes[4 * b + 0], 0), Hb);
    r.y1 = min(max(boxes[4 * b + 1], r.y0), Hb);
    r.x0 = min(max(boxes[4 * b + 2], 0), Wb);
    r.x1 = min(max(boxes[4 * b + 3], r.x0), Wb);
    return r;
}

struct EVArgs {
    const float* gt;           // [B,Hg,Wg]
    const float* disp;         // [B,h,w]
    const int* sizes;          // [B,2]
    const int* boxes;          // [B,4]
    int B, Hg, Wg, h, w;
    float min_depth, max_depth, scale;
    const float* scales;       // [B] or null: the image's scale is scale * scales[b]
    int flags;
    float* rows;               // [B,11]
    unsigned* meta;            // [B][2]: number of masked pixels, NaN flag of pred
    unsigned* state;           // [B][2 buffers][2 ranks][2]: key prefix, rank left inside the prefix
    unsigned* hist;            // [B][2 buffers][2 ranks][EV_BINS]
    unsigned* keys;            // [B][2 buffers][Hg*Wg]: gt keys, pred keys
    double* slab;              // [B][G][NSUM]
    int G;                     // metrics workgroups per image
};

__device__ __forceinline__ size_t ev_plane(const EVArgs& a) { return (size_t)a.Hg * a.Wg; }

// The image's disparity -> depth at ground-truth pixel (y, x), before any ratio
__device__ __forceinline__ float ev_pred(const EVArgs& a, const float* dp, float sy, float sx, int y, int x, float scale) {
    return ev::disp_depth(ev::bilinear_sample(dp, a.h, a.w, sy, sx, y, x), scale);
}

// The scale of image b: the caller's, times the image's own where a table came (mcav_eval_depth_scaled), formed once in float32
__device__ __forceinline__ float ev_image_scale(const EVArgs& a, int b) { return a.scales ? ev::mul_rn(a.scale, a.scales[b]) : a.scale; }

__device__ __forceinline__ void ev_axis_scales(const EVArgs& a, int b, float& sy, float& sx) {
    const int Hb = min(max(a.sizes[2 * b], 1), a.Hg), Wb = min(max(a.sizes[2 * b + 1], 1), a.Wg);
    sy = ev::axis_scale(a.h, Hb);
    sx = ev::axis_scale(a.w, Wb);
}

// median(gt) / median(pred) of image b from the selected keys (after the last select); NaN without pixels or with a NaN prediction
__device__ __forceinline__ float ev_ratio(const EVArgs& a, int b) {
    if (!(a.flags & MCAV_EVAL_MEDIAN_SCALING)) return 1.0f;
    const unsigned n = a.meta[2 * b];
    if (n == 0 || a.meta[2 * b + 1]) return NAN;
    const unsigned* st = a.state + (size_t)b * 8;
    const float mg = ev::median_of(ev::key_float(st[0]), ev::key_float(st[2]), n);
    const float mp = ev::median_of(ev::key_float(st[4]), ev::key_float(st[6]), n);
    return ev::div_rn(mg, mp);
}

__global__ __launch_bounds__(EV_THREADS) void eval_init_kernel(EVArgs a) {
    const int b = blockIdx.x;
    if (threadIdx.x < 2) a.meta[2 * b + threadIdx.x] = 0u;
    unsigned* hb = a.hist + (size_t)b * 4 * EV_BINS;
    for (int i = threadIdx.x; i < 4 * EV_BINS; i += EV_THREADS) hb[i] = 0u;
}

__global__ __launch_bounds__(EV_THREADS) void eval_gather_kernel(EVArgs a) {
    __shared__ unsigned s_cnt[EV_THREADS / 64], s_base;
    __shared__ int s_nan;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const EVBox bx = ev_box(a.sizes, a.boxes, b, a.Hg, a.Wg);
    const int bw = bx.x1 - bx.x0, nbox = (bx.y1 - bx.y0) * bw;
    const int start = blockIdx.x * EV_TILE;
    if (start >= nbox) return;                         // uniform over the workgroup
    float sy, sx;
    ev_axis_scales(a, b, sy, sx);
    const float scale = ev_image_scale(a, b);
    const size_t plane = ev_plane(a);
    const float* gp = a.gt + (size_t)b * plane;
    const float* dp = a.disp + (size_t)b * a.h * a.w;
    float gv[EV_PPT], pv[EV_PPT];
    unsigned long long bal[EV_PPT];
    unsigned cnt = 0;
    bool nan_seen = false;
#pragma unroll
    for (int k = 0; k < EV_PPT; ++k) {
        const int i = start + k * EV_THREADS + tid;
        const bool in = i < nbox;
        const int q = in ? i : 0;
        const int y = bx.y0 + q / bw, x = bx.x0 + q % bw;
        const float g = in ? gp[(size_t)y * a.Wg + x] : 0.0f;
        const bool m = in && g > a.min_depth && g < a.max_depth;
        const float p = m ? ev_pred(a, dp, sy, sx, y, x, scale) : 0.0f;
        nan_seen |= m && p != p;
        bal[k] = __ballot(m);
        cnt += (unsigned)__popcll(bal[k]);
        gv[k] = g;
        pv[k] = p;
    }
    // one integer atomic per workgroup reserves the slots of all its masked pixels; the waves share them out in LDS
    if (tid == 0) s_nan = 0;
    __syncthreads();
    if (lane == 0) s_cnt[wave] = cnt;
    if (nan_seen) s_nan = 1;
    __syncthreads();
    if (tid == 0) {
        const unsigned tot = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        s_base = tot ? atomicAdd(&a.meta[2 * b], tot) : 0u;
        if (s_nan) atomicOr(&a.meta[2 * b + 1], 1u);
    }
    __syncthreads();
    unsigned o = s_base;
    for (int w = 0; w < wave; ++w) o += s_cnt[w];
    unsigned* kg = a.keys + (size_t)b * 2 * plane;
    unsigned* kp = kg + plane;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < EV_PPT; ++k) {
        if ((bal[k] >> lane) & 1ull) {
            const unsigned at = o + (unsigned)__popcll(bal[k] & below);
            kg[at] = ev::float_key(gv[k]);
            kp[at] = ev::float_key(pv[k]);
        }
        o += (unsigned)__popcll(bal[k]);
    }
}

// pass p: per (image, buffer) histogram of digit p of the keys that match each rank's prefix so far.  Pass 0: every key matches both
// ranks, so only rank 0's histogram is formed (select reads it for both).
__global__ __launch_bounds__(EV_THREADS) void eval_hist_kernel(EVArgs a, int p) {
    __shared__ unsigned lh[2][EV_BINS];
    const int buf = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const unsigned n = a.meta[2 * b];
    const unsigned start = (unsigned)blockIdx.x * EV_KTILE;
    if (start >= n) return;                            // uniform over the workgroup
    for (int i = tid; i < 2 * EV_BINS; i += EV_THREADS) (&lh[0][0])[i] = 0u;
    __syncthreads();
    const auto [shift, dmask, pmask] = radix_pass(p);
    const unsigned* st = a.state + ((size_t)b * 2 + buf) * 4;
    const unsigned pre0 = p ? st[0] & pmask : 0u, pre1 = p ? st[2] & pmask : 0u;
    const unsigned* kb = a.keys + ((size_t)b * 2 + buf) * ev_plane(a);
#pragma unroll 4
    for (int k = 0; k < EV_KPT; ++k) {
        const unsigned i = start + (unsigned)(k * EV_THREADS + tid);
        if (i < n) {
            const unsigned key = kb[i], d = (key >> shift) & dmask;
            if ((key & pmask) == pre0) atomicAdd(&lh[0][d], 1u);
            if (p && (key & pmask) == pre1) atomicAdd(&lh[1][d], 1u);
        }
    }
    __syncthreads();
    unsigned* hg = a.hist + ((size_t)b * 2 + buf) * 2 * EV_BINS;
    for (int i = tid; i < (p ? 2 : 1) * EV_BINS; i += EV_THREADS) {
        const unsigned v = (&lh[0][0])[i];
        if (v) atomicAdd(&hg[i], v);
    }
}

// pass p: for one (image, buffer), the bin of each rank, its digit appended to the prefix and the rank left inside it; the histogram is
// zeroed for the next pass (and the next call).
__global__ __launch_bounds__(EV_THREADS) void eval_select_kernel(EVArgs a, int p) {
    __shared__ unsigned wtot[EV_THREADS / 64];
    constexpr int PER = EV_BINS / EV_THREADS;          // 8 bins per thread
    const int buf = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const unsigned n = a.meta[2 * b];
    if (n == 0) return;                                // nothing was counted: the histogram is still zero
    unsigned* hg = a.hist + ((size_t)b * 2 + buf) * 2 * EV_BINS;
    unsigned* st = a.state + ((size_t)b * 2 + buf) * 4;
    const int shift = radix_pass(p).shift;
    unsigned pick[2] = {0u, 0u}, left[2] = {0u, 0u};
    bool mine[2];
    for (int r = 0; r < 2; ++r) {
        const unsigned* src = hg + (size_t)(p ? r : 0) * EV_BINS + tid * PER;
        unsigned c[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) c[j] = src[j];
        const unsigned k = p ? st[2 * r + 1] : (r == 0 ? (n - 1) / 2 : n / 2);
        mine[r] = pick_bin<PER, EV_THREADS / 64>(c, k, wtot, pick[r], left[r]);
    }
    __syncthreads();                                   // every thread has read the state and the bins
    for (int r = 0; r < 2; ++r)
        if (mine[r]) {
            st[2 * r] = (p ? st[2 * r] : 0u) | (pick[r] << shift);
            st[2 * r + 1] = left[r];
        }
    for (int i = tid; i < 2 * EV_BINS; i += EV_THREADS) hg[i] = 0u;
}

__global__ __launch_bounds__(EV_THREADS) void eval_metrics_kernel(EVArgs a) {
    __shared__ double s_red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const EVBox bx = ev_box(a.sizes, a.boxes, b, a.Hg, a.Wg);
    const int bw = bx.x1 - bx.x0, nbox = (bx.y1 - bx.y0) * bw;
    const int start = blockIdx.x * EV_TILE;
    double s[ev::NSUM];
#pragma unroll
    for (int k = 0; k < ev::NSUM; ++k) s[k] = 0.0;
    if (start < nbox) {                                // uniform over the workgroup
        float sy, sx;
        ev_axis_scales(a, b, sy, sx);
        const float ratio = ev_ratio(a, b), scale = ev_image_scale(a, b);
        const float* gp = a.gt + (size_t)b * ev_plane(a);
        const float* dp = a.disp + (size_t)b * a.h * a.w;
        for (int k = 0; k < EV_PPT; ++k) {
            const int i = start + k * EV_THREADS + tid;
            if (i >= nbox) break;
            const int y = bx.y0 + i / bw, x = bx.x0 + i % bw;
            const float g = gp[(size_t)y * a.Wg + x];
            if (!(g > a.min_depth && g < a.max_depth)) continue;
            float p = ev_pred(a, dp, sy, sx, y, x, scale);
            if (a.flags & MCAV_EVAL_MEDIAN_SCALING) p = ev::mul_rn(p, ratio);
            ev::pixel_terms(g, ev::clip(p, a.min_depth, a.max_depth), s);
        }
    }
    double* out = a.slab + ((size_t)b * a.G + blockIdx.x) * ev::NSUM;
#pragma unroll
    for (int k = 0; k < ev::NSUM; ++k) {
        const double t = block_sum<double, EV_THREADS / 64>(s[k], s_red);
        if (tid == 0) out[k] = t;
    }
}

__global__ __launch_bounds__(EV_THREADS) void eval_finalize_kernel(EVArgs a) {
    __shared__ double s_red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s[ev::NSUM];
#pragma unroll
    for (int k = 0; k < ev::NSUM; ++k) s[k] = 0.0;
    for (int i = tid; i < a.G; i += EV_THREADS) {     // thread t takes entries t, t + 256, ...
        const double* src = a.slab + ((size_t)b * a.G + i) * ev::NSUM;
#pragma unroll
        for (int k = 0; k < ev::NSUM; ++k) s[k] += src[k];
    }
#pragma unroll
    for (int k = 0; k < ev::NSUM; ++k) s[k] = block_sum<double, EV_THREADS / 64>(s[k], s_red);
    if (tid == 0) {
        float m[9];
        ev::metrics_row(s, m);
        float* row = a.rows + (size_t)b * 11;
        for (int k = 0; k < 9; ++k) row[k] = m[k];
        row[9] = (float)s[10];
        row[10] = s[10] > 0.0 ? ev_ratio(a, b) : NAN;
    }
}

struct EVLayout {
    size_t meta_off, state_off, hist_off, keys_off, slab_off, total;
    int G;
};

inline EVLayout ev_layout(int B, int Hg, int Wg) {
    EVLayout l;
    const size_t plane = (size_t)Hg * Wg;
    l.G = (int)((plane + EV_TILE - 1) / EV_TILE);
    size_t o = 0;
    l.meta_off = o;  o = align_up(o + sizeof(unsigned) * 2 * (size_t)B, 256);
    l.state_off = o; o = align_up(o + sizeof(unsigned) * 8 * (size_t)B, 256);
    l.hist_off = o;  o = align_up(o + sizeof(unsigned) * 4 * EV_BINS * (size_t)B, 256);
    l.keys_off = o;  o = align_up(o + sizeof(unsigned) * 2 * plane * (size_t)B, 256);
    l.slab_off = o;  o = align_up(o + sizeof(double) * ev::NSUM * (size_t)l.G * B, 256);
    l.total = o;
    return l;
}

inline bool ev_shape_ok(int B, int Hg, int Wg, int h, int w) {
    if (B <= 0 || Hg <= 0 || Wg <= 0 || h <= 0 || w <= 0) return false;
    if (B > 65535) return false;                                                   // grid y / z
    return (size_t)Hg * Wg <= (size_t)0x7fffffff - EV_KTILE;                        // int pixel indices
}

}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_eval_depth_workspace_bytes(int B, int Hg, int Wg) {
    if (!ev_shape_ok(B, Hg, Wg, 1, 1)) return 0;
    return ev_layout(B, Hg, Wg).total;
}

MCAV_EXPORT int mcav_eval_depth_scaled(const float* gt, const float* disp, int B, int Hg, int Wg, int h, int w, const int* sizes,
                                       const int* boxes, float min_depth, float max_depth, float scale, const float* scales, int flags,
                                       float* rows, void* workspace, size_t workspace_bytes, void* stream) {
    if (!gt || !disp || !sizes || !boxes || !rows || !workspace) return MCAV_E_INVALID;
    if (!ev_shape_ok(B, Hg, Wg, h, w)) return MCAV_E_INVALID;
    if (flags & ~MCAV_EVAL_MEDIAN_SCALING) return MCAV_E_INVALID;
    if (!(min_depth > 0.0f) || !(max_depth > min_depth) || !isfinite(scale)) return MCAV_E_INVALID;     // (a NaN fails each test)
    const EVLayout l = ev_layout(B, Hg, Wg);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    EVArgs a = {};
    a.gt = gt; a.disp = disp; a.sizes = sizes; a.boxes = boxes;
    a.B = B; a.Hg = Hg; a.Wg = Wg; a.h = h; a.w = w;
    a.min_depth = min_depth; a.max_depth = max_depth; a.scale = scale; a.scales = scales; a.flags = flags;
    a.rows = rows;
    a.meta = reinterpret_cast<unsigned*>(ws + l.meta_off);
    a.state = reinterpret_cast<unsigned*>(ws + l.state_off);
    a.hist = reinterpret_cast<unsigned*>(ws + l.hist_off);
    a.keys = reinterpret_cast<unsigned*>(ws + l.keys_off);
    a.slab = reinterpret_cast<double*>(ws + l.slab_off);
    a.G = l.G;
    hipStream_t s = as_stream(stream);
    const size_t plane = (size_t)Hg * Wg;
    const int kg = (int)((plane + EV_KTILE - 1) / EV_KTILE);
    if (flags & MCAV_EVAL_MEDIAN_SCALING) {            // without scaling no median is needed: metrics + finalize only
        timed_launch(eval_init_kernel, dim3(B), dim3(EV_THREADS), 0, s, a);
        timed_launch(eval_gather_kernel, dim3(l.G, B), dim3(EV_THREADS), 0, s, a);
        for (int p = 0; p < RADIX_PASSES; ++p) {
            timed_launch(eval_hist_kernel, dim3(kg, 2, B), dim3(EV_THREADS), 0, s, a, p);
            timed_launch(eval_select_kernel, dim3(2, B), dim3(EV_THREADS), 0, s, a, p);
        }
    }
    timed_launch(eval_metrics_kernel, dim3(l.G, B), dim3(EV_THREADS), 0, s, a);
    timed_launch(eval_finalize_kernel, dim3(B), dim3(EV_THREADS), 0, s, a);
    return launch_status();
}

MCAV_EXPORT int mcav_eval_depth(const float* gt, const float* disp, int B, int Hg, int Wg, int h, int w, const int* sizes, const int* boxes,
                                float min_depth, float max_depth, float scale, int flags, float* rows, void* workspace, size_t workspace_bytes,
                                void* stream) {
    return mcav_eval_depth_scaled(gt, disp, B, Hg, Wg, h, w, sizes, boxes, min_depth, max_depth, scale, nullptr, flags, rows, workspace,
                                  workspace_bytes, stream);
}
