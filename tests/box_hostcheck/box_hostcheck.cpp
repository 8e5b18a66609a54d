// TEST INFRASTRUCTURE (CPU): drives csrc/box_math.h -- the functions the box kernels (csrc/box.hip) call -- with plain host loops: the
// prepared boxes, the pair intersection and both overlaps, the IoU matrix, and the whole greedy suppression (candidates, their order by a
// plain sort of the header's (key, index) pairs, the cut at pre_max, the walk over the kept rows, the gathered outputs and their tails).
// The argument checks and the workspace formula are the header's, the ones the product runs.
// Built by tests/test_box_cpu.py with g++ -ffp-contract=off, as a shared library and (with -DBOX_STANDALONE) as a program that either
// reads one suppression case from a file and writes its result to another -- the form that runs under the sanitizers -- or, as
// `box_hostcheck --sincos-ulp [threads]`, measures box_sincos against the float64 sine and cosine over every float32 heading a valid box
// may have and prints the largest error in ulp.  Never loaded by the product.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "box_math.h"

using namespace mcav;

extern "C" void box_host_constants(int* out4, float* out5) {
    out4[0] = box::MAX_VERTS;
    out4[1] = box::NMS_MAX_CANDIDATES;
    out4[2] = (int)sizeof(box::Prep);
    out4[3] = box::COLS;
    out5[0] = box::MIN_EXTENT;
    out5[1] = box::MAX_EXTENT;
    out5[2] = box::MAX_HEADING;
    out5[3] = box::CIRCLE_SLACK;
    out5[4] = box::BOX_SINCOS_MAX_ULP;
}

extern "C" void box_host_sincos(const float* h, float* s, float* c, long long n) {
    for (long long i = 0; i < n; ++i) box::box_sincos(h[i], s[i], c[i]);
}

extern "C" void box_host_prepare(const float* boxes, long long n, float* prep20) {
    for (long long i = 0; i < n; ++i) {
        const box::Prep p = box::prepare(boxes + i * box::COLS);
        memcpy(prep20 + i * 20, &p, sizeof p);
    }
}

// row i of a against row i of b: the intersection and the overlap in `mode`
extern "C" void box_host_pairs(const float* a, const float* b, long long n, int mode, float* inter, float* iou) {
    for (long long i = 0; i < n; ++i) {
        const box::Prep pa = box::prepare(a + i * box::COLS), pb = box::prepare(b + i * box::COLS);
        inter[i] = box::inter_bev(pa, pb);
        iou[i] = box::iou(pa, pb, mode);
    }
}

extern "C" int box_host_iou(const float* a, long long na, const float* b, long long nb, int mode, float* out) {
    const int rc = box::iou_refusal(a, na, b, nb, mode, out);
    if (rc) return rc;
    std::vector<box::Prep> pb((size_t)nb);
    for (long long j = 0; j < nb; ++j) pb[(size_t)j] = box::prepare(b + j * box::COLS);
    for (long long i = 0; i < na; ++i) {
        const box::Prep pa = box::prepare(a + i * box::COLS);
        for (long long j = 0; j < nb; ++j) out[i * nb + j] = box::iou(pa, pb[(size_t)j], mode);
    }
    return 0;
}

extern "C" size_t box_host_workspace_bytes(int B, long long A, int pre_max) {
    box::Layout l;
    return box::layout(B, A, pre_max, l) ? l.total : 0;
}

// the candidates of one image in the order walked, cut at pre_max
static std::vector<unsigned long long> ordered(const float* boxes, const float* scores, long long A, float score_thresh, int pre_max) {
    std::vector<unsigned long long> pairs;
    for (long long i = 0; i < A; ++i)
        if (box::score_passes(scores[i], score_thresh) && box::valid(boxes + i * box::COLS))
            pairs.push_back(box::order_pair(box::order_key(scores[i]), (uint32_t)i));
    std::sort(pairs.begin(), pairs.end());
    if (pairs.size() > (size_t)pre_max) pairs.resize((size_t)pre_max);
    return pairs;
}

// order [B, pre_max] (-1 behind the count), count [B]
extern "C" void box_host_select(const float* boxes, const float* scores, int B, long long A, float score_thresh, int pre_max, int* order,
                                int* count) {
    for (int b = 0; b < B; ++b) {
        const auto pairs = ordered(boxes + (size_t)b * A * box::COLS, scores + (size_t)b * A, A, score_thresh, pre_max);
        count[b] = (int)pairs.size();
        for (int j = 0; j < pre_max; ++j) order[(size_t)b * pre_max + j] = j < count[b] ? (int)(uint32_t)pairs[(size_t)j] : -1;
    }
}

// mcav_box_nms on the host; the header's refusal codes.  workspace is checked, not used.
extern "C" int box_host_nms(const float* boxes, const float* scores, const int* classes, int B, long long A, float score_thresh, float iou_thresh,
                            int mode, int pre_max, int post_max, int* keep, int* num, float* out_boxes, float* out_scores,
                            const void* workspace, size_t workspace_bytes) {
    const int rc = box::nms_refusal(boxes, scores, classes, B, A, score_thresh, iou_thresh, mode, pre_max, post_max, keep, num, out_boxes,
                                    out_scores, workspace, workspace_bytes);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        const float* bx = boxes + (size_t)b * A * box::COLS;
        const float* sc = scores + (size_t)b * A;
        const int* cl = classes ? classes + (size_t)b * A : nullptr;
        const auto pairs = ordered(bx, sc, A, score_thresh, pre_max);
        std::vector<box::Prep> prep(pairs.size());
        for (size_t j = 0; j < pairs.size(); ++j) prep[j] = box::prepare(bx + (size_t)(uint32_t)pairs[j] * box::COLS);
        std::vector<size_t> kept;
        for (size_t j = 0; j < pairs.size() && kept.size() < (size_t)post_max; ++j) {
            const uint32_t idx = (uint32_t)pairs[j];
            bool dead = false;
            for (size_t e = 0; e < kept.size() && !dead; ++e) {
                const size_t k = kept[e];
                if (cl && cl[(uint32_t)pairs[k]] != cl[idx]) continue;
                dead = box::iou(prep[k], prep[j], mode) > iou_thresh;
            }
            if (!dead) kept.push_back(j);
        }
        num[b] = (int)kept.size();
        for (int e = 0; e < post_max; ++e) {
            const bool live = (size_t)e < kept.size();
            const uint32_t idx = live ? (uint32_t)pairs[kept[(size_t)e]] : 0u;
            keep[(size_t)b * post_max + e] = live ? (int)idx : -1;
            if (out_scores) out_scores[(size_t)b * post_max + e] = live ? sc[idx] : 0.0f;
            if (out_boxes)
                for (int c = 0; c < box::COLS; ++c) out_boxes[((size_t)b * post_max + e) * box::COLS + c] = live ? bx[(size_t)idx * box::COLS + c] : 0.0f;
        }
    }
    return 0;
}

// |got - want| in ulp of want (want = m 2^ex, m in [0.5, 1): a float32 ulp is 2^(ex - 24)); a zero wants a zero
static double ulp_error(float got, double want) {
    if (want == 0.0) return got == 0.0f ? 0.0 : 1e30;
    int ex;
    frexp(want, &ex);
    return fabs((double)got - want) / ldexp(1.0, ex - 24);
}

static double sincos_error_ulp(float h) {
    float s, c;
    box::box_sincos(h, s, c);
    return std::max(ulp_error(s, sin((double)h)), ulp_error(c, cos((double)h)));
}

// The largest error over the headings +-h whose bit patterns are first, first + stride, ... <= last (patterns ascend with |h|), and
// where it was found
extern "C" double box_host_sincos_scan(uint32_t first, uint32_t last, uint32_t stride, float* worst_at) {
    double worst = -1.0;
    for (uint64_t u = first; u <= last; u += stride) {
        float h;
        const uint32_t bits = (uint32_t)u;
        memcpy(&h, &bits, 4);
        for (int sign = 0; sign < 2; ++sign) {
            const float v = sign ? -h : h;
            const double err = sincos_error_ulp(v);
            if (err > worst) { worst = err; *worst_at = v; }
        }
    }
    return worst;
}

#ifdef BOX_STANDALONE
#include <thread>

static int sincos_ulp_main(int threads) {
    uint32_t last;
    const float lim = box::MAX_HEADING;
    memcpy(&last, &lim, 4);
    std::vector<double> worst((size_t)threads, 0.0);
    std::vector<float> at((size_t)threads, 0.0f);
    std::vector<std::thread> pool;
    for (int k = 0; k < threads; ++k)
        pool.emplace_back([&, k] { worst[k] = box_host_sincos_scan((uint32_t)k, last, (uint32_t)threads, &at[k]); });
    for (auto& th : pool) th.join();
    double w = 0.0;
    float where = 0.0f;
    for (int k = 0; k < threads; ++k)
        if (worst[k] > w) { w = worst[k]; where = at[k]; }
    printf("box_sincos: %llu arguments with |h| <= %g, largest error %.6f ulp at h = %a (header: %g)\n", 2ull * ((unsigned long long)last + 1ull),
           (double)lim, w, (double)where, (double)box::BOX_SINCOS_MAX_ULP);
    return w <= (double)box::BOX_SINCOS_MAX_ULP ? 0 : 1;
}

// in : int64 [8] = B A pre_max post_max mode has_classes has_out workspace_bytes; float32 [2] = score_thresh iou_thresh;
//      float32 boxes [B, A, 7]; float32 scores [B, A]; int32 classes [B, A] if has_classes
// out: int32 status; int32 keep [B, post_max]; int32 num [B]; if has_out float32 out_boxes [B, post_max, 7], out_scores [B, post_max].
//      Every buffer is exactly as large as the call may touch.
template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--sincos-ulp")) return sincos_ulp_main(argc >= 3 ? atoi(argv[2]) : 16);
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> hd;
    std::vector<float> th, boxes, scores;
    std::vector<int32_t> classes;
    if (!(rd(f, hd, 8) && rd(f, th, 2))) return 2;
    const int B = (int)hd[0], pre_max = (int)hd[2], post_max = (int)hd[3], mode = (int)hd[4];
    const size_t A = (size_t)hd[1], rows = (size_t)B * A, outs = (size_t)B * (size_t)post_max;
    const bool ok = rd(f, boxes, rows * 7) && rd(f, scores, rows) && (!hd[5] || rd(f, classes, rows));
    fclose(f);
    if (!ok) return 2;
    std::vector<int32_t> keep(outs), num((size_t)B);
    std::vector<float> out_boxes(hd[6] ? outs * 7 : 0), out_scores(hd[6] ? outs : 0);
    void* ws = nullptr;
    if (posix_memalign(&ws, 256, (size_t)hd[7] ? (size_t)hd[7] : 1)) return 2;
    const int32_t status = box_host_nms(boxes.data(), scores.data(), hd[5] ? classes.data() : nullptr, B, (long long)A, th[0], th[1], mode, pre_max,
                                        post_max, keep.data(), num.data(), hd[6] ? out_boxes.data() : nullptr,
                                        hd[6] ? out_scores.data() : nullptr, ws, (size_t)hd[7]);
    free(ws);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&status, 4, 1, o);
    fwrite(keep.data(), 4, keep.size(), o);
    fwrite(num.data(), 4, num.size(), o);
    if (hd[6]) { fwrite(out_boxes.data(), 4, out_boxes.size(), o); fwrite(out_scores.data(), 4, out_scores.size(), o); }
    fclose(o);
    return 0;
}
#endif
