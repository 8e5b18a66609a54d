// TEST INFRASTRUCTURE (CPU): drives the per-pixel math of csrc/pl_math.h and csrc/eval_math.h -- the functions the batch projection
// kernels (csrc/pl_batch.hip) call -- with plain host loops in the kernels' order of passes.  Built by tests/test_pl_batch_cpu.py with
// g++ -ffp-contract=off, as a shared library and (with -DPLB_STANDALONE) as a program that reads one case from a file and writes its
// result to another, which is the form that runs under the sanitizers.  Never loaded by the product.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pl_math.h"

using namespace mcav;

namespace {

struct Case {
    const float* m;
    const float* intensity;
    const int* sizes;
    const double* calib;                 // [B, 28]: P then T
    const double* elev;
    const double* azim;
    int B, h, w, Hg, Wg, nb, na;
    float scale;
    double max_height, max_depth;
    int input_depth;
};

bool pixel_point(const Case& a, int b, int r, int c, float& d, double (&q)[3]) {
    const int Hb = a.sizes[2 * b] < a.Hg ? a.sizes[2 * b] : a.Hg, Wb = a.sizes[2 * b + 1] < a.Wg ? a.sizes[2 * b + 1] : a.Wg;
    if (r >= Hb || c >= Wb) return false;
    PLCalib cal;
    pl_calib(a.calib + (size_t)b * 28 + 12, a.calib + (size_t)b * 28, cal);
    d = plb::depth_of(plb::sample(a.m + (size_t)b * a.h * a.w, a.h, a.w, Hb, Wb, r, c), a.scale, a.input_depth != 0);
    pl_point_at((double)d, r, c, cal, q);
    return true;
}

void write_row(const Case& a, int b, int r, int c, const double (&q)[3], float* cloud, size_t o, size_t capacity) {
    if (o >= capacity) return;
    const int Hb = a.sizes[2 * b] < a.Hg ? a.sizes[2 * b] : a.Hg, Wb = a.sizes[2 * b + 1] < a.Wg ? a.sizes[2 * b + 1] : a.Wg;
    cloud[4 * o + 0] = (float)q[0];
    cloud[4 * o + 1] = (float)q[1];
    cloud[4 * o + 2] = (float)q[2];
    cloud[4 * o + 3] = a.intensity ? plb::sample(a.intensity + (size_t)b * a.h * a.w, a.h, a.w, Hb, Wb, r, c) : 0.0f;
}

}  // namespace

// The whole call on the host.  -1: refused (tables).
extern "C" int plb_host_project(const float* m, int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib,
                                const float* intensity, const double* elev, const double* azim, int nb, int na, float scale,
                                double max_height, double max_depth, int sparsity, int flags, float* cloud, size_t capacity, int* offsets) {
    if (elev && !(plb::table_ok(elev, nb) && plb::table_ok(azim, na))) return -1;
    const Case a{m, intensity, sizes, calib, elev, azim, B, h, w, Hg, Wg, nb, na, scale, max_height, max_depth, flags & 1};
    const size_t step = sparsity > 0 ? (size_t)sparsity : 1;
    size_t rows = 0;
    std::vector<unsigned long long> cells;
    for (int b = 0; b < B; ++b) {
        offsets[b] = (int)rows;
        if (elev) cells.assign((size_t)nb * na, plb::EMPTY_CELL);
        size_t rank = 0;
        for (int r = 0; r < Hg; ++r)
            for (int c = 0; c < Wg; ++c) {
                float d;
                double q[3];
                if (!pixel_point(a, b, r, c, d, q) || !plb::keep(q, d, max_height, max_depth)) continue;
                if (!elev) {
                    if (rank % step == 0) write_row(a, b, r, c, q, cloud, rows + rank / step, capacity);
                    ++rank;
                    continue;
                }
                int beam, az;
                if (!plb::beam_cell(q, elev, nb, azim, na, beam, az)) continue;
                const unsigned long long word = plb::cell_word(plb::range_key(q), (uint32_t)((size_t)r * Wg + c));
                unsigned long long& slot = cells[(size_t)beam * na + az];
                if (word < slot) slot = word;
            }
        if (!elev) {
            rows += (rank + step - 1) / step;
            continue;
        }
        for (size_t i = 0; i < cells.size(); ++i) {
            if (cells[i] == plb::EMPTY_CELL) continue;
            const uint32_t p = (uint32_t)(cells[i] & 0xffffffffull);
            const int r = (int)(p / (uint32_t)Wg), c = (int)(p % (uint32_t)Wg);
            float d;
            double q[3];
            pixel_point(a, b, r, c, d, q);
            write_row(a, b, r, c, q, cloud, rows++, capacity);
        }
    }
    offsets[B] = (int)rows;
    return 0;
}

// plb::bilinear_sample / disp_depth against eval_math.h's own, over a whole resized image: the number of values whose bits differ
extern "C" int plb_host_differs_from_eval(const float* plane, int h, int w, int H, int W, float scale) {
    int bad = 0;
    const float sy = ev::axis_scale(h, H), sx = ev::axis_scale(w, W);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const float a = plb::bilinear_sample(plane, h, w, sy, sx, r, c), b = ev::bilinear_sample(plane, h, w, sy, sx, r, c);
            bad += ev::float_bits(a) != ev::float_bits(b);
            bad += ev::float_bits(plb::disp_depth(a, scale)) != ev::float_bits(ev::disp_depth(b, scale));
        }
    return bad;
}

extern "C" int plb_host_table_bin(const double* tab, int n, double v) { return plb::table_bin(tab, n, v); }
extern "C" int plb_host_table_ok(const double* tab, int n) { return plb::table_ok(tab, n) ? 1 : 0; }

#ifdef PLB_STANDALONE
// in : int32 [12] = B h w Hg Wg nb na sparsity flags has_intensity capacity 0; float64 [3] = scale max_height max_depth;
//      int32 sizes [2B]; float64 calib [28B]; float32 m [B h w]; float32 intensity [B h w] if has_intensity; float64 elev [nb + 1] and
//      azim [na + 1] if nb > 0
// out: int32 status; int32 offsets [B + 1]; float32 cloud [capacity, 4] (0xff-filled where nothing was written)
template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> hd, sizes;
    std::vector<double> sc, calib, elev, azim;
    std::vector<float> m, inten;
    bool ok = rd(f, hd, 12) && rd(f, sc, 3);
    if (!ok) return 2;
    const int B = hd[0], h = hd[1], w = hd[2], nb = hd[5], na = hd[6];
    const size_t cap = (size_t)hd[10];
    ok = rd(f, sizes, (size_t)2 * B) && rd(f, calib, (size_t)28 * B) && rd(f, m, (size_t)B * h * w) &&
         rd(f, inten, hd[9] ? (size_t)B * h * w : 0) && rd(f, elev, nb > 0 ? (size_t)nb + 1 : 0) && rd(f, azim, nb > 0 ? (size_t)na + 1 : 0);
    fclose(f);
    if (!ok) return 2;
    std::vector<int32_t> offsets((size_t)B + 1, 0);
    std::vector<float> cloud(cap * 4);
    for (size_t i = 0; i < cloud.size(); ++i) cloud[i] = ev::bits_float(0xffffffffu);
    const int32_t status = plb_host_project(m.data(), B, h, w, hd[3], hd[4], sizes.data(), calib.data(), hd[9] ? inten.data() : nullptr,
                                            nb > 0 ? elev.data() : nullptr, nb > 0 ? azim.data() : nullptr, nb, na, (float)sc[0], sc[1], sc[2],
                                            hd[7], hd[8], cloud.data(), cap, offsets.data());
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    fwrite(&status, 4, 1, g);
    fwrite(offsets.data(), 4, offsets.size(), g);
    if (!cloud.empty()) fwrite(cloud.data(), 4, cloud.size(), g);
    fclose(g);
    return 0;
}
#endif
