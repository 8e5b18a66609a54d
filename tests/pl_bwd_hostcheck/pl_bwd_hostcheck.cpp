// TEST INFRASTRUCTURE (CPU): drives csrc/pl_bwd_math.h -- the functions the kernels of csrc/pl_bwd.hip call -- with plain host loops in
// the kernels' order: per pillar its used slots; per cloud row its pixel of G; per element of the network's plane the window of outputs
// that touch it.  Built by tests/test_pl_bwd_cpu.py with g++ -ffp-contract=off, as a shared library and (with -DPL_BWD_STANDALONE) as a
// program that reads one case from a file and writes its result to another, which is the form that runs under the sanitizers.  Never
// loaded by the product.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pl_bwd_math.h"

using namespace mcav;

// mcav_pillarize_bwd on the host.  -1: refused.
extern "C" int pl_bwd_pillars_host(const float* d_voxels, const int* slot_points, const int* num_points, const int* pillar_offsets, int B,
                                   long long capacity, int N, int C, float* d_points, long long n_max) {
    if (!d_voxels || !slot_points || !num_points || !pillar_offsets || !d_points) return -1;
    if (B <= 0 || B > 65535 || n_max < 0 || n_max > 0x7fffffffll || capacity < 0 || N < 1 || N > pil::MAX_POINTS) return -1;
    if (C != pil::COLS_PLAIN && C != pil::COLS_DECORATED) return -1;
    for (long long e = 0; e < 4 * n_max; ++e) d_points[e] = 0.0f;
    const long long total = pillar_offsets[B] > 0 ? pillar_offsets[B] : 0;
    const long long P = total < capacity ? total : capacity;
    for (long long r = 0; r < P; ++r) {
        const float* tile = d_voxels + (size_t)r * N * C;
        int count = num_points[r] < 0 ? 0 : num_points[r];
        if (count > N) count = N;
        for (int lane = 0; lane < count; ++lane) {
            const int i = slot_points[(size_t)r * N + lane];
            if (i < 0 || i >= n_max) continue;
            for (int col = 0; col < 4; ++col)
                d_points[(size_t)i * 4 + col] =
                    plg::point_grad(tile + (size_t)lane * C, C, col, C == pil::COLS_DECORATED && col < 3 ? plg::column_sum(tile + 4 + col, C, count) : 0.0, count);
        }
    }
    return 0;
}

// mcav_pl_batch_project_bwd on the host; G: [B, Hg, Wg], the workspace's plane, handed out for the tests.  -1: refused.
extern "C" int pl_bwd_plane_host(const float* d_points, long long capacity, const int* pixels, const int* offsets, const float* m, int B, int h,
                                 int w, int Hg, int Wg, const int* sizes, const double* calib, float scale, const float* scales, int flags,
                                 float* d_m, float* G) {
    if (!d_points || !pixels || !offsets || !m || !sizes || !calib || !d_m || !G || h <= 0 || w <= 0 || capacity < 0) return -1;
    if (B <= 0 || Hg <= 0 || Wg <= 0 || (flags & ~1) || !(scale == scale)) return -1;
    if ((unsigned long long)Hg * Wg * B > 0x7fffffffull || (unsigned long long)h * w * B > 0x7fffffffull) return -1;
    const bool input_depth = flags & 1;
    for (size_t e = 0; e < (size_t)B * Hg * Wg; ++e) G[e] = 0.0f;
    const long long rows = offsets[B] < 0 ? 0 : offsets[B];
    for (long long o = 0; o < rows && o < capacity; ++o) {
        const int b = pil::image_of(offsets, B, (int)o);
        const int p = pixels[o];
        if (p < 0 || (long long)p >= (long long)Hg * Wg) continue;
        const int r = p / Wg, c = p - r * Wg;
        const int Hb = sizes[2 * b] < Hg ? sizes[2 * b] : Hg, Wb = sizes[2 * b + 1] < Wg ? sizes[2 * b + 1] : Wg;
        if (r >= Hb || c >= Wb) continue;
        float s;
        if (!plg::image_scale(scale, scales, b, s)) continue;
        PLCalib k;
        pl_calib(calib + (size_t)b * 28 + 12, calib + (size_t)b * 28, k);
        const float v = plb::sample(m + (size_t)b * h * w, h, w, Hb, Wb, r, c);
        G[((size_t)b * Hg + r) * Wg + c] = plg::plane_grad(d_points + (size_t)o * 4, v, s, input_depth, r, c, k);
    }
    for (int b = 0; b < B; ++b) {
        const int Hb = sizes[2 * b] < Hg ? sizes[2 * b] : Hg, Wb = sizes[2 * b + 1] < Wg ? sizes[2 * b + 1] : Wg;
        float s;
        const bool live = plg::image_scale(scale, scales, b, s) && Hb >= 1 && Wb >= 1;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                d_m[((size_t)b * h + y) * w + x] = live ? plg::resize_adjoint(G + (size_t)b * Hg * Wg, Wg, h, w, Hb, Wb, y, x) : 0.0f;
    }
    return 0;
}

// the window of source i and the taps of output o along one axis resized from n_in to n_out
extern "C" void pl_bwd_window_host(int i, int n_in, int n_out, int* lo, int* hi) {
    plg::adjoint_window(i, n_in, ev::axis_scale(n_in, n_out), n_out, *lo, *hi);
}
extern "C" void pl_bwd_taps_host(int o, int n_in, int n_out, int* i0, int* i1, float* l) {
    ev::bilinear_axis(o, n_in, ev::axis_scale(n_in, n_out), *i0, *i1, *l);
}

#ifdef PL_BWD_STANDALONE
// in : int64 [16] = B capacity N C n_max | rows_capacity h w Hg Wg flags has_scales 0 0 0 0; float32 scale;
//      pillars: int32 pillar_offsets [B + 1], num_points [capacity], slot_points [capacity, N]; float32 d_voxels [capacity, N, C]
//      plane:   int32 offsets [B + 1], pixels [rows_capacity], sizes [B, 2]; float64 calib [B, 28]; float32 scales [B] if has_scales,
//               m [B, h, w], d_points [rows_capacity, 4]
// out: int32 status of each call; float32 d_points [n_max, 4]; float32 d_m [B, h, w]
template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> hd;
    std::vector<float> sc;
    if (!rd(f, hd, 16) || !rd(f, sc, 1)) return 2;
    const int B = (int)hd[0], N = (int)hd[2], C = (int)hd[3], h = (int)hd[6], w = (int)hd[7], Hg = (int)hd[8], Wg = (int)hd[9];
    const size_t cap = (size_t)hd[1], n_max = (size_t)hd[4], rows_cap = (size_t)hd[5];
    std::vector<int32_t> poff, num, slots, offsets, pixels, sizes;
    std::vector<float> dvox, scales, m, dpts;
    std::vector<double> calib;
    const bool ok = rd(f, poff, (size_t)B + 1) && rd(f, num, cap) && rd(f, slots, cap * N) && rd(f, dvox, cap * N * C) &&
                    rd(f, offsets, (size_t)B + 1) && rd(f, pixels, rows_cap) && rd(f, sizes, (size_t)B * 2) && rd(f, calib, (size_t)B * 28) &&
                    rd(f, scales, hd[11] ? (size_t)B : 0) && rd(f, m, (size_t)B * h * w) && rd(f, dpts, rows_cap * 4);
    fclose(f);
    if (!ok) return 2;
    std::vector<float> out_points(n_max * 4), out_m((size_t)B * h * w), G((size_t)B * Hg * Wg);
    const int32_t st[2] = {
        pl_bwd_pillars_host(dvox.data(), slots.data(), num.data(), poff.data(), B, (long long)cap, N, C, out_points.data(), (long long)n_max),
        pl_bwd_plane_host(dpts.data(), (long long)rows_cap, pixels.data(), offsets.data(), m.data(), B, h, w, Hg, Wg, sizes.data(), calib.data(),
                          sc[0], hd[11] ? scales.data() : nullptr, (int)hd[10], out_m.data(), G.data())};
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(st, 4, 2, o);
    fwrite(out_points.data(), 4, out_points.size(), o);
    fwrite(out_m.data(), 4, out_m.size(), o);
    fclose(o);
    return 0;
}
#endif
