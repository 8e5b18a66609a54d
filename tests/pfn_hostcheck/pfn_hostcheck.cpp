// TEST INFRASTRUCTURE (CPU): drives the arithmetic and the row search of csrc/pfn_math.h -- the functions the pillar feature net's kernels
// (csrc/pfn_image.hip) call -- with plain host loops in the kernel's order: per canvas row and column tile, the 64-probe search of coords
// for the tile's first row, the members of the window of TILE rows behind it, per member the layer, the ReLU and the maximum over the
// used slots, then the tile's cells into the canvas.
// Built by tests/test_pfn_cpu.py with g++ -ffp-contract=off, as a shared library and (with -DPFN_STANDALONE) as a program that reads one
// case from a file and writes its result to another, which is the form that runs under the sanitizers.  Never loaded by the product.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pfn_math.h"

using namespace mcav;

static const int TILE = 128;             // csrc/pfn_image.hip

// The whole call on the host.  -1: refused.  flags & 1: canvas [B, ny, nx, c_out].  canvas or features may be null, not both.
extern "C" int pfn_host_pseudo_image(const float* voxels, const int* coords, const int* num_points, const int* pillar_offsets, int B,
                                     long long capacity, int N, int C, int nx, int ny, const float* weight, const float* bias,
                                     const float* bias_pad, int c_out, int flags, float* canvas, float* features) {
    if (!voxels || !coords || !num_points || !pillar_offsets || !weight || !bias || !bias_pad || (!canvas && !features)) return -1;
    if (B <= 0 || B > 65535 || capacity < 0 || nx < 1 || ny < 1 || N < 1 || N > pfn::MAX_POINTS) return -1;
    if ((unsigned long long)B * (unsigned long long)ny * (unsigned long long)nx > 0x7fffffffull) return -1;
    if (!pfn::columns_ok(C) || !pfn::c_out_ok(c_out) || (flags & ~1)) return -1;
    const bool nhwc = flags & 1;
    const long long P = pfn::live_pillars(pillar_offsets, B, capacity);
    std::vector<float> feat((size_t)c_out);
    auto pillar = [&](long long r) {
        const int n = pfn::used_slots(num_points[r], N);
        const float* rows = voxels + (size_t)r * N * C;
        for (int o = 0; o < c_out; ++o) {
            pfn::Max m = pfn::max_start(n < N, bias_pad[o]);
            for (int k = 0; k < n; ++k) pfn::max_join(m, pfn::act(pfn::pre(rows + (size_t)k * C, weight + (size_t)o * C, C, bias[o])));
            feat[o] = pfn::max_value(m);
        }
    };
    if (!canvas) {
        for (long long r = 0; r < P; ++r) {
            pillar(r);
            memcpy(features + (size_t)r * c_out, feat.data(), sizeof(float) * c_out);
        }
        return 0;
    }
    const size_t plane = (size_t)ny * nx;
    std::vector<float> image((size_t)c_out * TILE);
    for (int b = 0; b < B; ++b)
        for (int iy = 0; iy < ny; ++iy) {
            long long lo, hi;
            pfn::image_rows(pillar_offsets, b, P, lo, hi);
            long long first = pfn::first_at_or_after(coords, lo, hi, iy, 0);            // one search per canvas row
            for (int x0 = 0; x0 < nx; x0 += TILE) {
                const int w = nx - x0 < TILE ? nx - x0 : TILE;
                std::fill(image.begin(), image.end(), 0.0f);
                int members = 0;
                for (long long r = first; r < hi && r < first + TILE; ++r) {             // the window of TILE rows, its members
                    if (!pfn::in_tile(coords, r, b, iy, x0, w)) continue;
                    ++members;
                    const int col = coords[4 * r + 3] - x0;
                    pillar(r);
                    for (int o = 0; o < c_out; ++o) image[(size_t)o * TILE + col] = feat[o];
                    if (features) memcpy(features + (size_t)r * c_out, feat.data(), sizeof(float) * c_out);
                }
                first += members;                                                        // the next tile's rows follow this tile's
                for (int o = 0; o < c_out; ++o)
                    for (int col = 0; col < w; ++col) {
                        const size_t at = nhwc ? (((size_t)b * ny + iy) * nx + x0 + col) * c_out + o
                                               : ((size_t)b * c_out + o) * plane + (size_t)iy * nx + x0 + col;
                        canvas[at] = image[(size_t)o * TILE + col];
                    }
            }
        }
    return 0;
}

// C's fmaf, elementwise: what tests/pfn_ref.py's fma32 is held against
extern "C" void pfn_host_fmaf(const float* a, const float* b, const float* c, float* out, long long n) {
    for (long long i = 0; i < n; ++i) out[i] = fmaf(a[i], b[i], c[i]);
}

extern "C" long long pfn_host_first_at_or_after(const int* coords, long long lo, long long hi, int y, int x) {
    return pfn::first_at_or_after(coords, lo, hi, y, x);
}

#ifdef PFN_STANDALONE
// in : int64 [10] = B capacity N C nx ny c_out flags want_features 0; int32 offsets [B + 1]; int32 num_points [capacity]; int32 coords
//      [capacity, 4]; float32 voxels [capacity, N, C]; float32 weight [c_out, C], bias [c_out], bias_pad [c_out]
// out: int32 status; float32 canvas [B * c_out * ny * nx]; float32 features [capacity, c_out] if asked for (both 0xff-filled where nothing
//      was written)
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
    if (!rd(f, hd, 10)) return 2;
    const int B = (int)hd[0], N = (int)hd[2], C = (int)hd[3], nx = (int)hd[4], ny = (int)hd[5], c_out = (int)hd[6];
    const size_t cap = (size_t)hd[1];
    std::vector<int32_t> offsets, num, coords;
    std::vector<float> vox, weight, bias, pad;
    const bool ok = rd(f, offsets, (size_t)B + 1) && rd(f, num, cap) && rd(f, coords, cap * 4) && rd(f, vox, cap * N * C) &&
                    rd(f, weight, (size_t)c_out * C) && rd(f, bias, (size_t)c_out) && rd(f, pad, (size_t)c_out);
    fclose(f);
    if (!ok) return 2;
    std::vector<float> canvas((size_t)B * c_out * ny * nx), features(hd[8] ? cap * c_out : 0);
    memset(canvas.data(), 0xff, canvas.size() * sizeof(float));
    if (!features.empty()) memset(features.data(), 0xff, features.size() * sizeof(float));
    const int32_t status = pfn_host_pseudo_image(vox.data(), coords.data(), num.data(), offsets.data(), B, (long long)cap, N, C, nx, ny,
                                                 weight.data(), bias.data(), pad.data(), c_out, (int)hd[7], canvas.data(),
                                                 hd[8] ? features.data() : nullptr);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&status, 4, 1, o);
    fwrite(canvas.data(), 4, canvas.size(), o);
    if (!features.empty()) fwrite(features.data(), 4, features.size(), o);
    fclose(o);
    return 0;
}
#endif
