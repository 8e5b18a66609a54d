// TEST INFRASTRUCTURE (CPU): drives the per-pixel math of csrc/ground_math.h -- the functions the ground-scale kernels
// (csrc/ground_scale.hip) call -- with plain host loops.  Built by tests/test_ground_scale_cpu.py with g++ -ffp-contract=off, as a shared
// library and (with -DGS_STANDALONE) as a program that reads one case from a file and writes its result to another, which is the form
// that runs under the sanitizers.  Never loaded by the product.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ground_math.h"

using namespace mcav;

// The whole call on the host: rows [B, 4], mask [B, h, w], hgt [B, h, w] (written on ground pixels only).  -1: refused.
extern "C" int gs_host_ground_scale(const float* m, int B, int h, int w, const int* sizes, const double* calib, const int* boxes,
                                    float camera_height, float cos_max, int min_ground, float fallback, int flags, float* rows,
                                    unsigned char* mask, float* hgt_out) {
    if (B <= 0 || h < 3 || w < 3 || !gs::scalars_ok(camera_height, cos_max, min_ground, flags)) return -1;
    std::vector<float> xn((size_t)w), yn((size_t)h), X((size_t)h * w), Y((size_t)h * w), Z((size_t)h * w), heights;
    for (int b = 0; b < B; ++b) {
        const double* P = calib + (size_t)b * 28;
        for (int c = 0; c < w; ++c) xn[c] = gs::ray(c, sizes[2 * b + 1], w, P[2], P[0]);
        for (int r = 0; r < h; ++r) yn[r] = gs::ray(r, sizes[2 * b], h, P[4 + 2], P[4 + 1]);
        const float* mp = m + (size_t)b * h * w;
        for (int r = 0; r < h; ++r)
            for (int c = 0; c < w; ++c) {
                const size_t i = (size_t)r * w + c;
                const float d = gs::depth_of(mp[i], (flags & 1) != 0);
                X[i] = gs::mul(xn[c], d);
                Y[i] = gs::mul(yn[r], d);
                Z[i] = d;
            }
        const gs::Box box = gs::clamp_box(boxes ? boxes + 4 * b : nullptr, h, w);
        heights.clear();
        for (int r = 0; r < h; ++r)
            for (int c = 0; c < w; ++c) {
                const size_t i = (size_t)b * h * w + (size_t)r * w + c;
                mask[i] = 0;
                if (r < 1 || r > h - 2 || c < 1 || c > w - 2) continue;
                float x9[9], y9[9], z9[9], hgt;
                for (int k = 0; k < 9; ++k) {
                    const size_t j = (size_t)(r - 1 + k / 3) * w + (c - 1 + k % 3);
                    x9[k] = X[j]; y9[k] = Y[j]; z9[k] = Z[j];
                }
                const bool g = gs::ground_pixel(x9, y9, z9, cos_max, hgt) && gs::in_box(box, r, c);
                if (gs::pixel_key(g, hgt) == gs::NOT_GROUND) continue;
                mask[i] = 1;
                hgt_out[i] = hgt;
                heights.push_back(hgt);
            }
        std::sort(heights.begin(), heights.end());
        const size_t n = heights.size();
        float row[4];
        gs::image_row((uint32_t)n, n ? heights[(n - 1) / 2] : 0.0f, n ? heights[n / 2] : 0.0f, camera_height, min_ground, fallback, row);
        for (int k = 0; k < 4; ++k) rows[4 * b + k] = row[k];
    }
    return 0;
}

extern "C" int gs_host_scalars_ok(float camera_height, float cos_max, int min_ground, int flags) {
    return gs::scalars_ok(camera_height, cos_max, min_ground, flags) ? 1 : 0;
}

#ifdef GS_STANDALONE
// in : int32 [8] = B h w min_ground flags has_boxes 0 0; float32 [4] = camera_height cos_max fallback 0; int32 sizes [2B];
//      float64 calib [28B]; int32 boxes [4B] if has_boxes; float32 m [B h w]
// out: int32 status; float32 rows [4B]; uint8 mask [B h w]; float32 hgt [B h w] (0xff-filled where nothing was written)
template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> hd, sizes, boxes;
    std::vector<float> sc, m;
    std::vector<double> calib;
    if (!(rd(f, hd, 8) && rd(f, sc, 4))) return 2;
    const int B = hd[0], h = hd[1], w = hd[2];
    if (B <= 0 || h <= 0 || w <= 0) return 2;
    const size_t px = (size_t)B * h * w;
    const bool ok = rd(f, sizes, (size_t)2 * B) && rd(f, calib, (size_t)28 * B) && rd(f, boxes, hd[5] ? (size_t)4 * B : 0) && rd(f, m, px);
    fclose(f);
    if (!ok) return 2;
    std::vector<float> rows((size_t)4 * B), hgt(px);
    std::vector<unsigned char> mask(px);
    for (size_t i = 0; i < px; ++i) hgt[i] = ev::bits_float(0xffffffffu);
    const int32_t status = gs_host_ground_scale(m.data(), B, h, w, sizes.data(), calib.data(), hd[5] ? boxes.data() : nullptr, sc[0], sc[1],
                                                hd[3], sc[2], hd[4], rows.data(), mask.data(), hgt.data());
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    fwrite(&status, 4, 1, g);
    fwrite(rows.data(), 4, rows.size(), g);
    fwrite(mask.data(), 1, mask.size(), g);
    fwrite(hgt.data(), 4, hgt.size(), g);
    fclose(g);
    return 0;
}
#endif
