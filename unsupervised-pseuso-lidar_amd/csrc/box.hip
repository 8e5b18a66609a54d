// Oriented-box overlap and batched greedy suppression (include/mcav_depth.h: mcav_box_iou, mcav_box_nms; the definition is
// tests/box_ref.py, the arithmetic csrc/box_math.h).  Four kernels, wave64:
//   iou     one workgroup per 64 x 64 tile of the [na, nb] matrix: the tile's rows of both operands are gathered once into LDS (a 7-float
//           row is not 16-byte aligned), prepared there by 128 threads, then a lane is a column and a wave walks 16 rows
//   select  one workgroup of 1024 threads per image: counts the candidates (the score first, 4 bytes per anchor; a box row is read only
//           when the score passes); above pre_max finds the cut key by block_ops.h's radix select over an LDS histogram, three passes, the
//           lowest indices of the tie bin filling the rest; compacts the survivors in index order (a scan of 1024 flags per pass) as
//           (key, index) pairs in LDS, orders the <= 4096 pairs there (bitonic), and writes the order, the classes, the prepared boxes in
//           that order and the count to the workspace
//   mask    per image the 64 x 64 tiles of the upper triangle below the candidate count: a lane is a column, a wave walks rows, the
//           64-bit __ballot of (iou > thresh, same class, column behind row) is the row's word of the tile
//   scan    one wavefront per image; lane l owns word l of the 4096-bit "removed" set.  Per chunk of 64 candidates: the chunk's 64 mask
//           rows are loaded first (they do not depend on the decisions), the chunk is resolved serially on its diagonal word by the lane
//           that owns it, the kept rows are ORed into the set; keep, num and the gathered rows leave from here, and the tails are filled
// The histogram's LDS integer adds are the only atomics (exact in any order); nothing returns to the host, no allocation, every launch
// on the caller's stream: the call can be captured, and two runs give the same bytes.
#include "block_ops.h"
#include "box_math.h"
#include "kernel_timer.h"

namespace mcav {
namespace box {

static_assert(REFUSED == MCAV_E_INVALID && SHORT_WORKSPACE == MCAV_E_WORKSPACE, "box_math.h restates the return codes");
static_assert(NMS_MAX_CANDIDATES == MCAV_NMS_MAX_CANDIDATES && MODE_BEV == MCAV_BOX_IOU_BEV && MODE_3D == MCAV_BOX_IOU_3D, "box_math.h restates the header");

constexpr int TILE = 64;
constexpr int THREADS = 256;                    // iou, mask: four waves, 16 rows of a tile each
constexpr int SEL_THREADS = 1024, SEL_WAVES = 16;
constexpr int BINS_PER_THREAD = RADIX_BINS / SEL_THREADS;
typedef unsigned long long u64;
typedef float f32x4 __attribute__((ext_vector_type(4)));

union PrepWords {
    Prep p;
    f32x4 w[5];
    __device__ PrepWords() {}
};

__device__ __forceinline__ Prep load_prep(const Prep* src) {
    PrepWords u;
    const f32x4* s = reinterpret_cast<const f32x4*>(src);
#pragma unroll
    for (int k = 0; k < 5; ++k) u.w[k] = s[k];
    return u.p;
}
__device__ __forceinline__ void store_prep(Prep* dst, const Prep& p) {
    PrepWords u;
    u.p = p;
    f32x4* d = reinterpret_cast<f32x4*>(dst);
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = u.w[k];
}

// ---------------------------------------------------------------------------------------------- iou
__global__ __launch_bounds__(THREADS) void box_iou_kernel(const float* a, int na, const float* b, int nb, int mode, float* out) {
    __shared__ float raw[2][TILE * COLS];
    __shared__ __attribute__((aligned(16))) Prep prep[2][TILE];
    const int row0 = (int)blockIdx.y * TILE, col0 = (int)blockIdx.x * TILE;
    const int rows = min(TILE, na - row0), cols = min(TILE, nb - col0);
    for (int e = threadIdx.x; e < rows * COLS; e += THREADS) raw[0][e] = a[(size_t)row0 * COLS + e];
    for (int e = threadIdx.x; e < cols * COLS; e += THREADS) raw[1][e] = b[(size_t)col0 * COLS + e];
    __syncthreads();
    if (threadIdx.x < 2 * TILE) {
        const int which = threadIdx.x >> 6, r = threadIdx.x & 63;
        if (r < (which ? cols : rows)) prep[which][r] = prepare(&raw[which][r * COLS]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane >= cols) return;
    const Prep pb = prep[1][lane];
    for (int r = wave; r < rows; r += THREADS / 64) out[(size_t)(row0 + r) * nb + (col0 + lane)] = iou(prep[0][r], pb, mode);
}

// ---------------------------------------------------------------------------------------------- select
struct SelectArgs {
    const float* boxes;
    const float* scores;
    const int* classes;
    int A, pre_max;
    float score_thresh;
    int* count;
    int* order;
    int* cls;
    Prep* prep;
};

// the key of anchor i of the image, if it is a candidate
__device__ __forceinline__ bool candidate(const float* sc, const float* bx, float score_thresh, int i, unsigned& key) {
    const float s = sc[i];
    if (!score_passes(s, score_thresh)) return false;
    float v[COLS];
#pragma unroll
    for (int k = 0; k < COLS; ++k) v[k] = bx[(size_t)i * COLS + k];
    if (!valid(v)) return false;
    key = order_key(s);
    return true;
}

__global__ __launch_bounds__(SEL_THREADS) void box_select_kernel(SelectArgs a) {
    __shared__ u64 pairs[NMS_MAX_CANDIDATES];
    __shared__ unsigned hist[RADIX_BINS];
    __shared__ unsigned s_w[SEL_WAVES];
    __shared__ unsigned s_sel[2];
    const int b = blockIdx.x, tid = threadIdx.x, A = a.A;
    const float* sc = a.scores + (size_t)b * A;
    const float* bx = a.boxes + (size_t)b * A * COLS;

    unsigned mine = 0;
    for (int i = tid; i < A; i += SEL_THREADS) {
        unsigned key;
        mine += candidate(sc, bx, a.score_thresh, i, key) ? 1u : 0u;
    }
    const unsigned total = block_sum<unsigned, SEL_WAVES>(mine, s_w);

    // every candidate below `cut` stays, and the first `ties` of those at it (in index order)
    unsigned cut = 0xffffffffu, ties = 0u;
    if (total > (unsigned)a.pre_max) {                     // uniform over the workgroup
        unsigned prefix = 0u, k = (unsigned)a.pre_max - 1u;
        for (int p = 0; p < RADIX_PASSES; ++p) {
            const RadixPass rp = radix_pass(p);
            for (int e = tid; e < RADIX_BINS; e += SEL_THREADS) hist[e] = 0u;
            __syncthreads();
            for (int i = tid; i < A; i += SEL_THREADS) {
                unsigned key;
                if (candidate(sc, bx, a.score_thresh, i, key) && (key & rp.pmask) == prefix) atomicAdd(&hist[(key >> rp.shift) & rp.dmask], 1u);
            }
            __syncthreads();
            unsigned c[BINS_PER_THREAD];
#pragma unroll
            for (int j = 0; j < BINS_PER_THREAD; ++j) c[j] = hist[tid * BINS_PER_THREAD + j];
            unsigned pick, left;
            if (pick_bin<BINS_PER_THREAD, SEL_WAVES>(c, k, s_w, pick, left)) {
                s_sel[0] = pick;
                s_sel[1] = left;
            }
            __syncthreads();
            prefix |= s_sel[0] << rp.shift;
            k = s_sel[1];
            __syncthreads();
        }
        cut = prefix;
        ties = k + 1u;
    }
    const int n = (int)min(total, (unsigned)a.pre_max);

    // compaction in index order: the scan carries the counts below the cut (low half) and at it (high half) of 1024 anchors
    unsigned below_before = 0u, ties_before = 0u;
    for (int base = 0; base < A; base += SEL_THREADS) {
        const int i = base + tid;
        unsigned key = 0u;
        const bool cand = i < A && candidate(sc, bx, a.score_thresh, i, key);
        const bool below = cand && key < cut, tie = cand && key == cut;
        unsigned sum;
        const unsigned ex = block_scan<unsigned, SEL_WAVES>((below ? 1u : 0u) | (tie ? 0x10000u : 0u), s_w, sum);
        const unsigned tie_rank = ties_before + (ex >> 16);
        if (below || (tie && tie_rank < ties)) pairs[below_before + (ex & 0xffffu) + min(tie_rank, ties)] = order_pair(key, (unsigned)i);
        below_before += sum & 0xffffu;
        ties_before += sum >> 16;
    }
    int width = 64;
    while (width < n) width <<= 1;
    __syncthreads();
    for (int e = n + tid; e < width; e += SEL_THREADS) pairs[e] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= width; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < width / 2; t += SEL_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const u64 x = pairs[lo], y = pairs[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    pairs[lo] = y;
                    pairs[hi] = x;
                }
            }
            __syncthreads();
        }

    const size_t slot0 = (size_t)b * a.pre_max;
    for (int j = tid; j < n; j += SEL_THREADS) {
        const unsigned idx = (unsigned)pairs[j];
        a.order[slot0 + j] = (int)idx;
        a.cls[slot0 + j] = a.classes ? a.classes[(size_t)b * A + idx] : 0;
        float v[COLS];
#pragma unroll
        for (int c = 0; c < COLS; ++c) v[c] = bx[(size_t)idx * COLS + c];
        store_prep(a.prep + slot0 + j, prepare(v));
    }
    if (tid == 0) a.count[b] = n;
}

// ---------------------------------------------------------------------------------------------- mask
__global__ __launch_bounds__(THREADS) void box_mask_kernel(const int* count, const int* cls, const Prep* prep, int pre_max, int words, float iou_thresh,
                                                           int mode, u64* mask) {
    __shared__ __attribute__((aligned(16))) Prep rows[TILE];
    __shared__ int row_cls[TILE];
    const int ct = blockIdx.x, rt = blockIdx.y, b = blockIdx.z;
    const int n = count[b];
    if (rt > ct || ct * TILE >= n) return;                 // the whole workgroup; rt <= ct: the row tile starts below n too
    const size_t slot0 = (size_t)b * pre_max;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int live_rows = min(TILE, n - rt * TILE);
    if ((int)threadIdx.x < live_rows) {
        store_prep(&rows[threadIdx.x], load_prep(prep + slot0 + rt * TILE + threadIdx.x));
        row_cls[threadIdx.x] = cls[slot0 + rt * TILE + threadIdx.x];
    }
    const int col = ct * TILE + lane;
    Prep pc;
    int col_cls = 0;
    if (col < n) {
        pc = load_prep(prep + slot0 + col);
        col_cls = cls[slot0 + col];
    }
    __syncthreads();
    for (int r = wave; r < live_rows; r += THREADS / 64) {
        const int row = rt * TILE + r;
        bool hit = false;
        if (col < n && col > row && col_cls == row_cls[r]) hit = iou(rows[r], pc, mode) > iou_thresh;
        const u64 word = __ballot(hit);
        if (lane == 0) mask[(slot0 + row) * words + ct] = word;
    }
}

// ---------------------------------------------------------------------------------------------- scan
struct ScanArgs {
    const float* boxes;
    const float* scores;
    const int* count;
    const int* order;
    const u64* mask;
    int A, pre_max, post_max, words;
    int* keep;
    int* num;
    float* out_boxes;
    float* out_scores;
};

__global__ __launch_bounds__(64) void box_scan_kernel(ScanArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.count[b];
    const size_t slot0 = (size_t)b * a.pre_max, out0 = (size_t)b * a.post_max;
    u64 removed = 0ull;
    int kept = 0;
    for (int c = 0; c * 64 < n && kept < a.post_max; ++c) {
        u64 row[64];
        const bool reads = lane >= c && lane * 64 < n;     // words in front of the diagonal and behind the count were not written
#pragma unroll
        for (int r = 0; r < 64; ++r) row[r] = reads && c * 64 + r < n ? a.mask[(slot0 + c * 64 + r) * a.words + lane] : 0ull;
        u64 keptbits = 0ull;
        if (lane == c) {
            u64 cur = removed;
            int k = kept;
#pragma unroll
            for (int r = 0; r < 64; ++r)
                if (c * 64 + r < n && !((cur >> r) & 1ull) && k < a.post_max) {
                    keptbits |= 1ull << r;
                    cur |= row[r];
                    ++k;
                }
        }
        keptbits = __shfl(keptbits, c, 64);
#pragma unroll
        for (int r = 0; r < 64; ++r)
            if ((keptbits >> r) & 1ull) removed |= row[r];
        if ((keptbits >> lane) & 1ull) {
            const size_t at = out0 + kept + __popcll(keptbits & ((1ull << lane) - 1ull));
            const int idx = a.order[slot0 + c * 64 + lane];
            const size_t src = (size_t)b * a.A + idx;
            a.keep[at] = idx;
            if (a.out_scores) a.out_scores[at] = a.scores[src];
            if (a.out_boxes)
#pragma unroll
                for (int k = 0; k < COLS; ++k) a.out_boxes[at * COLS + k] = a.boxes[src * COLS + k];
        }
        kept += __popcll(keptbits);
    }
    for (int j = kept + lane; j < a.post_max; j += 64) {
        a.keep[out0 + j] = -1;
        if (a.out_scores) a.out_scores[out0 + j] = 0.0f;
        if (a.out_boxes)
#pragma unroll
            for (int k = 0; k < COLS; ++k) a.out_boxes[(out0 + j) * COLS + k] = 0.0f;
    }
    if (lane == 0) a.num[b] = kept;
}

}  // namespace box
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT int mcav_box_iou(const float* a, long long na, const float* b, long long nb, int mode, float* out, void* stream) {
    const int refused = box::iou_refusal(a, na, b, nb, mode, out);
    if (refused) return refused;
    if (na == 0 || nb == 0) return MCAV_OK;
    const dim3 grid((unsigned)((nb + box::TILE - 1) / box::TILE), (unsigned)((na + box::TILE - 1) / box::TILE));
    timed_launch(box::box_iou_kernel, grid, dim3(box::THREADS), 0, as_stream(stream), a, (int)na, b, (int)nb, mode, out);
    return launch_status();
}

MCAV_EXPORT size_t mcav_box_nms_workspace_bytes(int B, long long A, int pre_max) {
    box::Layout l;
    return box::layout(B, A, pre_max, l) ? l.total : 0;
}

MCAV_EXPORT int mcav_box_nms(const float* boxes, const float* scores, const int* classes, int B, long long A, float score_thresh, float iou_thresh,
                             int mode, int pre_max, int post_max, int* keep, int* num, float* out_boxes, float* out_scores, void* workspace,
                             size_t workspace_bytes, void* stream) {
    const int refused = box::nms_refusal(boxes, scores, classes, B, A, score_thresh, iou_thresh, mode, pre_max, post_max, keep, num, out_boxes,
                                         out_scores, workspace, workspace_bytes);
    if (refused) return refused;
    box::Layout l;
    box::layout(B, A, pre_max, l);
    char* ws = reinterpret_cast<char*>(workspace);
    int* count = reinterpret_cast<int*>(ws + l.count);
    int* order = reinterpret_cast<int*>(ws + l.order);
    int* cls = reinterpret_cast<int*>(ws + l.cls);
    box::Prep* prep = reinterpret_cast<box::Prep*>(ws + l.prep);
    box::u64* mask = reinterpret_cast<box::u64*>(ws + l.mask);
    hipStream_t s = as_stream(stream);

    const box::SelectArgs sel{boxes, scores, classes, (int)A, pre_max, score_thresh, count, order, cls, prep};
    timed_launch(box::box_select_kernel, dim3(B), dim3(box::SEL_THREADS), 0, s, sel);          // (per-dispatch times for tools/box_bench.py)
    timed_launch(box::box_mask_kernel, dim3(l.words, l.words, B), dim3(box::THREADS), 0, s, (const int*)count, (const int*)cls,
                 (const box::Prep*)prep, pre_max, l.words, iou_thresh, mode, mask);
    const box::ScanArgs scan{boxes, scores, count, order, mask, (int)A, pre_max, post_max, l.words, keep, num, out_boxes, out_scores};
    timed_launch(box::box_scan_kernel, dim3(B), dim3(64), 0, s, scan);
    return launch_status();
}
