// TEST INFRASTRUCTURE (CPU): drives csrc/quant_math.h -- the functions the soft-occupancy kernels (csrc/quant.hip) call -- with plain host
// loops: the cell of every row, the cells' counts, then every kept row's terms added as 64-bit integers from the LAST row to the first
// (the sums must not depend on the order, as on the device where the atomics land in any order), the canvas from the sums; and the
// backward, one row at a time.  The argument checks and the workspace formula are the header's, the ones the product runs.
// Built by tests/test_quant_cpu.py with g++ -ffp-contract=off, as a shared library and (with -DQUANT_STANDALONE) as a program that either
// reads one case from a file and writes its result to another -- the form that runs under the sanitizers -- or, as
// `quant_hostcheck --exp-ulp [threads]`, measures quant_exp against the float64 exponential over every float32 argument whose result
// is not zero and prints the largest error in ulp.  Never loaded by the product.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "quant_math.h"

using namespace mcav;

static qnt::Grid grid_of(float x0, float y0, float z0, float vx, float vy, float vz, int nx, int ny, int nz) {
    return qnt::Grid{x0, y0, z0, vx, vy, vz, nx, ny, nz};
}

static int live_rows(const int* offsets, int B, long long n_max) {
    const long long n = offsets[B] < n_max ? offsets[B] : n_max;
    return n > 0 ? (int)n : 0;
}

extern "C" size_t quant_host_workspace_bytes(int B, long long n_max, int nz, int ny, int nx) {
    qnt::Layout l;
    return qnt::layout(B, n_max, nz, ny, nx, l) ? l.total : 0;
}

// The forward on the host; the header's refusal codes.  workspace is checked, not used.
extern "C" int quant_host_occupancy(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float vx,
                                    float vy, float vz, int nx, int ny, int nz, float sigma2, float* canvas, int* point_count,
                                    const void* workspace, size_t workspace_bytes) {
    const qnt::Grid g = grid_of(x0, y0, z0, vx, vy, vz, nx, ny, nz);
    const int rc = qnt::forward_refusal(points, offsets, B, n_max, g, sigma2, canvas, point_count, workspace, workspace_bytes);
    if (rc) return rc;
    const size_t per_image = (size_t)nz * ny * nx, total = per_image * B;
    const int n = live_rows(offsets, B, n_max);
    std::vector<int> counts(total, 0);
    std::vector<long long> cell((size_t)n, -1), sums(total, 0);
    for (int i = 0; i < n; ++i) {
        int ix, iy, iz;
        if (!qnt::cell_of(g, points[4 * (size_t)i], points[4 * (size_t)i + 1], points[4 * (size_t)i + 2], ix, iy, iz)) continue;
        cell[i] = (long long)(pil::image_of(offsets, B, i) * per_image + ((size_t)iz * ny + iy) * nx + ix);
        ++counts[(size_t)cell[i]];
    }
    for (int i = n - 1; i >= 0; --i) {
        if (point_count) point_count[i] = cell[i] < 0 ? 0 : counts[(size_t)cell[i]];
        if (cell[i] < 0) continue;
        const size_t image = (size_t)cell[i] / per_image * per_image, in_image = (size_t)cell[i] - image;
        const int ix = (int)(in_image % nx), iy = (int)(in_image / nx % ny), iz = (int)(in_image / nx / ny);
        const float* p = points + 4 * (size_t)i;
        for (int oz = -1; oz <= 1; ++oz)
            for (int oy = -1; oy <= 1; ++oy)
                for (int ox = -1; ox <= 1; ++ox) {
                    const int jx = ix + ox, jy = iy + oy, jz = iz + oz;
                    if (jx < 0 || jx >= nx || jy < 0 || jy >= ny || jz < 0 || jz >= nz) continue;
                    float d[3];
                    const float e = qnt::term(p[0], p[1], p[2], pil::cell_centre(jx, x0, vx), pil::cell_centre(jy, y0, vy),
                                              pil::cell_centre(jz, z0, vz), sigma2, d);
                    sums[image + ((size_t)jz * ny + jy) * nx + jx] += qnt::to_fixed(e, counts[(size_t)cell[i]], !(ox | oy | oz));
                }
    }
    for (size_t m = 0; m < total; ++m) canvas[m] = qnt::from_fixed(sums[m]);
    return 0;
}

extern "C" int quant_host_occupancy_bwd(const float* points, const int* offsets, const int* point_count, const float* d_canvas, int B,
                                        long long n_max, float x0, float y0, float z0, float vx, float vy, float vz, int nx, int ny, int nz,
                                        float sigma2, float* d_points) {
    const qnt::Grid g = grid_of(x0, y0, z0, vx, vy, vz, nx, ny, nz);
    const int rc = qnt::backward_refusal(points, offsets, point_count, d_canvas, B, n_max, g, sigma2, d_points);
    if (rc) return rc;
    const size_t per_image = (size_t)nz * ny * nx;
    const int n = live_rows(offsets, B, n_max);
    for (long long i = 0; i < n_max; ++i) {
        float out[3] = {0.0f, 0.0f, 0.0f};
        int ix, iy, iz;
        if (i < n && qnt::cell_of(g, points[4 * (size_t)i], points[4 * (size_t)i + 1], points[4 * (size_t)i + 2], ix, iy, iz))
            qnt::point_grad(g, sigma2, d_canvas + pil::image_of(offsets, B, (int)i) * per_image, points[4 * (size_t)i], points[4 * (size_t)i + 1],
                            points[4 * (size_t)i + 2], ix, iy, iz, point_count[i], out);
        float* row = d_points + 4 * (size_t)i;
        row[0] = out[0]; row[1] = out[1]; row[2] = out[2]; row[3] = 0.0f;
    }
    return 0;
}

// out[0..3] = TILE_X, TILE_Y, MAX_NZ, SCAN_TILE
extern "C" void quant_host_constants(int* out) {
    out[0] = qnt::TILE_X; out[1] = qnt::TILE_Y; out[2] = qnt::MAX_NZ; out[3] = qnt::SCAN_TILE;
}
extern "C" float quant_host_exp_max_ulp() { return qnt::QEXP_MAX_ULP; }
extern "C" float quant_host_exp_cut() { return qnt::QEXP_CUT; }
extern "C" void quant_host_exp(const float* t, float* out, long long n) {
    for (long long i = 0; i < n; ++i) out[i] = qnt::quant_exp(t[i]);
}
extern "C" int quant_host_cell(float x, float y, float z, float x0, float y0, float z0, float vx, float vy, float vz, int nx, int ny, int nz,
                               int* cell3) {
    return qnt::cell_of(grid_of(x0, y0, z0, vx, vy, vz, nx, ny, nz), x, y, z, cell3[0], cell3[1], cell3[2]) ? 1 : 0;
}

// |quant_exp(t) - exp(t)| in ulp of exp(t), 0 where quant_exp gives 0 below the cut
static double exp_error_ulp(float t) {
    const float got = qnt::quant_exp(t);
    if (got == 0.0f && t < qnt::QEXP_CUT) return 0.0;
    const double want = exp((double)t);
    int ex;
    frexp(want, &ex);                                       // want = m 2^ex, m in [0.5, 1): a float32 ulp is 2^(ex - 24)
    return fabs((double)got - want) / ldexp(1.0, ex - 24);
}

// The largest error over the negative arguments whose bit patterns are first, first + stride, ... <= last (0x80000000 is -0.0, patterns
// ascend with |t|), and where it was found
extern "C" double quant_host_exp_scan(uint32_t first, uint32_t last, uint32_t stride, float* worst_at) {
    double worst = -1.0;
    for (uint64_t u = first; u <= last; u += stride) {
        float t;
        const uint32_t bits = (uint32_t)u;
        memcpy(&t, &bits, 4);
        const double err = exp_error_ulp(t);
        if (err > worst) { worst = err; *worst_at = t; }
    }
    return worst;
}

#ifdef QUANT_STANDALONE
#include <thread>

static int exp_ulp_main(int threads) {
    uint32_t last;
    const float cut = qnt::QEXP_CUT;
    memcpy(&last, &cut, 4);
    const uint32_t first = 0x80000000u;
    std::vector<double> worst((size_t)threads, 0.0);
    std::vector<float> at((size_t)threads, 0.0f);
    std::vector<std::thread> pool;
    for (int k = 0; k < threads; ++k)
        pool.emplace_back([&, k] { worst[k] = quant_host_exp_scan(first + (uint32_t)k, last, (uint32_t)threads, &at[k]); });
    for (auto& th : pool) th.join();
    double w = exp_error_ulp(0.0f);
    float where = 0.0f;
    for (int k = 0; k < threads; ++k)
        if (worst[k] > w) { w = worst[k]; where = at[k]; }
    printf("quant_exp: %llu arguments in [%g, -0] and +0, largest error %.6f ulp at t = %a (header: %g)\n",
           (unsigned long long)(last - first) + 2ull, (double)cut, w, (double)where, (double)qnt::QEXP_MAX_ULP);
    return w <= (double)qnt::QEXP_MAX_ULP ? 0 : 1;
}

// in : int64 [8] = B n_max nx ny nz record workspace_bytes 0; float32 [8] = x0 y0 z0 vx vy vz sigma2 0; int32 offsets [B + 1];
//      float32 points [n_max, 4]; float32 d_canvas [B, nz, ny, nx]
// out: int32 forward status, int32 backward status; float32 canvas [B, nz, ny, nx]; int32 point_count [n_max]; float32 d_points [n_max, 4]
//      (0xff-filled where nothing was written).  Every buffer is exactly as large as the call may touch.
template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--exp-ulp")) return exp_ulp_main(argc >= 3 ? atoi(argv[2]) : 16);
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> hd;
    std::vector<float> gr, points, d_canvas;
    std::vector<int32_t> offsets;
    if (!(rd(f, hd, 8) && rd(f, gr, 8))) return 2;
    const int B = (int)hd[0], nx = (int)hd[2], ny = (int)hd[3], nz = (int)hd[4];
    const size_t n_max = (size_t)hd[1], cells = (size_t)B * nz * ny * nx;
    const bool ok = rd(f, offsets, (size_t)B + 1) && rd(f, points, n_max * 4) && rd(f, d_canvas, cells);
    fclose(f);
    if (!ok) return 2;
    std::vector<float> canvas(cells), d_points(n_max * 4);
    std::vector<int32_t> count(n_max);
    memset(canvas.data(), 0xff, canvas.size() * 4);
    if (n_max) { memset(d_points.data(), 0xff, d_points.size() * 4); memset(count.data(), 0xff, count.size() * 4); }
    void* ws = nullptr;
    if (posix_memalign(&ws, 256, (size_t)hd[6] ? (size_t)hd[6] : 1)) return 2;
    int32_t status[2];
    status[0] = quant_host_occupancy(points.data(), offsets.data(), B, (long long)n_max, gr[0], gr[1], gr[2], gr[3], gr[4], gr[5], nx, ny, nz,
                                     gr[6], canvas.data(), hd[5] ? count.data() : nullptr, ws, (size_t)hd[6]);
    status[1] = hd[5] ? quant_host_occupancy_bwd(points.data(), offsets.data(), count.data(), d_canvas.data(), B, (long long)n_max, gr[0], gr[1],
                                                 gr[2], gr[3], gr[4], gr[5], nx, ny, nz, gr[6], d_points.data())
                      : 0;
    free(ws);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(status, 4, 2, o);
    fwrite(canvas.data(), 4, canvas.size(), o);
    if (n_max) { fwrite(count.data(), 4, count.size(), o); fwrite(d_points.data(), 4, d_points.size(), o); }
    fclose(o);
    return 0;
}
#endif
