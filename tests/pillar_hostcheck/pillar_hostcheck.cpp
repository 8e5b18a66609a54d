// TEST INFRASTRUCTURE (CPU): drives the per-point and per-pillar math of csrc/pillar_math.h -- the functions the pillar kernels
// (csrc/pillarize.hip) call -- with plain host loops in the kernels' order of passes: count per cell, scan, fill, then per pillar the
// ordered selection 64 entries at a time, the means and the row block.  The segments are filled from the LAST point to the first, the
// opposite of cloud order: the selection has to do all the ordering, as it must on the device where the atomics land in any order.
// Built by tests/test_pillar_cpu.py with g++ -ffp-contract=off, as a shared library and (with -DPIL_STANDALONE) as a program that reads
// one case from a file and writes its result to another, which is the form that runs under the sanitizers.  Never loaded by the product.
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pillar_math.h"

using namespace mcav;

// The whole call on the host.  -1: refused.
extern "C" int pil_host_pillarize(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float z1,
                                  float vx, float vy, int nx, int ny, int N, int flags, float* voxels, int* coords, int* num_points,
                                  long long capacity, int* pillar_offsets) {
    const pil::Grid g{x0, y0, z0, z1, vx, vy, nx, ny};
    if (B <= 0 || n_max < 0 || N < 1 || N > pil::MAX_POINTS || capacity < 0 || (flags & ~1) || !pil::grid_ok(g)) return -1;
    const int C = (flags & 1) ? pil::COLS_DECORATED : pil::COLS_PLAIN;
    const size_t per_image = (size_t)ny * nx, M = per_image * B;
    const int n = offsets[B] < n_max ? offsets[B] : (int)n_max;
    std::vector<unsigned> cells(M + 1, 0u);
    std::vector<int> cell_of_point((size_t)(n > 0 ? n : 0), -1);
    for (int i = 0; i < n; ++i) {
        int ix, iy;
        if (!pil::cell_of(g, points[4 * (size_t)i], points[4 * (size_t)i + 1], points[4 * (size_t)i + 2], ix, iy)) continue;
        const int cell = (pil::image_of(offsets, B, i) * ny + iy) * nx + ix;
        cell_of_point[i] = cell;
        ++cells[cell];
    }
    std::vector<int> pillar_cell;
    unsigned start = 0;
    for (size_t j = 0; j < M; ++j) {
        if (j % per_image == 0) pillar_offsets[j / per_image] = (int)pillar_cell.size();
        const unsigned c = cells[j];
        cells[j] = start;
        if (c) pillar_cell.push_back((int)j);
        start += c;
    }
    cells[M] = start;
    pillar_offsets[B] = (int)pillar_cell.size();
    std::vector<int> index(start), fill(M, 0);
    for (int i = n - 1; i >= 0; --i)
        if (cell_of_point[i] >= 0) index[cells[cell_of_point[i]] + fill[cell_of_point[i]]++] = i;

    int kept[2][pil::MAX_POINTS], chunk[64];
    float tile[pil::MAX_POINTS * pil::COLS_DECORATED];
    for (size_t r = 0; r < pillar_cell.size() && r < (size_t)capacity; ++r) {
        const unsigned cell = (unsigned)pillar_cell[r], first = cells[cell], count = cells[cell + 1] - first;
        int k = 0, cur = 0;
        for (unsigned done = 0; done < count; done += 64u) {
            const int c = (int)(count - done < 64u ? count - done : 64u);
            for (int lane = 0; lane < 64; ++lane) chunk[lane] = lane < c ? index[first + done + lane] : INT_MAX;
            for (int lane = 0; lane < k; ++lane) {
                const int rk = pil::rank_among(kept[cur][lane], kept[cur], k, chunk, c);
                if (rk < N) kept[cur ^ 1][rk] = kept[cur][lane];
            }
            for (int lane = 0; lane < c; ++lane) {
                const int rc = pil::rank_among(chunk[lane], kept[cur], k, chunk, c);
                if (rc < N) kept[cur ^ 1][rc] = chunk[lane];
            }
            k = k + c < N ? k + c : N;
            cur ^= 1;
        }
        memset(tile, 0, sizeof(float) * (size_t)N * C);
        for (int lane = 0; lane < k; ++lane) memcpy(tile + lane * C, points + 4 * (size_t)kept[cur][lane], 16);
        const int b = (int)(cell / per_image);
        const unsigned in_image = cell - (unsigned)(b * per_image);
        const int iy = (int)(in_image / (unsigned)nx), ix = (int)(in_image % (unsigned)nx);
        if (C == pil::COLS_DECORATED) {
            const float mx = pil::column_mean(tile + 0, C, k), my = pil::column_mean(tile + 1, C, k), mz = pil::column_mean(tile + 2, C, k);
            const float cx = pil::cell_centre(ix, x0, vx), cy = pil::cell_centre(iy, y0, vy);
            for (int lane = 0; lane < k; ++lane) {
                float* row = tile + lane * C;
                pil::decorate(row[0], row[1], row[2], mx, my, mz, cx, cy, row + 4);
            }
        }
        memcpy(voxels + r * (size_t)N * C, tile, sizeof(float) * (size_t)N * C);
        coords[4 * r + 0] = b; coords[4 * r + 1] = 0; coords[4 * r + 2] = iy; coords[4 * r + 3] = ix;
        num_points[r] = k;
    }
    return 0;
}

extern "C" int pil_host_axis_cell(float v, float origin, float size, int n) {
    int cell = -1;
    return pil::axis_cell(v, origin, size, n, cell) ? cell : -1;
}
extern "C" int pil_host_image_of(const int* offsets, int B, int i) { return pil::image_of(offsets, B, i); }

#ifdef PIL_STANDALONE
// in : int64 [8] = B n_max nx ny N flags capacity 0; float32 [6] = x0 y0 z0 z1 vx vy; int32 offsets [B + 1]; float32 points [n_max, 4]
// out: int32 status; int32 pillar_offsets [B + 1]; int32 num_points [capacity]; int32 coords [capacity, 4]; float32 voxels [capacity, N, C]
//      (0xff-filled where nothing was written)
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
    std::vector<float> gr, points;
    std::vector<int32_t> offsets;
    bool ok = rd(f, hd, 8) && rd(f, gr, 6);
    if (!ok) return 2;
    const int B = (int)hd[0], N = (int)hd[4], C = (hd[5] & 1) ? 9 : 4;
    const size_t cap = (size_t)hd[6];
    ok = rd(f, offsets, (size_t)B + 1) && rd(f, points, (size_t)hd[1] * 4);
    fclose(f);
    if (!ok) return 2;
    std::vector<int32_t> poff((size_t)B + 1, -1), num(cap, -1), coords(cap * 4, -1);
    std::vector<float> vox(cap * N * C);
    if (!vox.empty()) memset(vox.data(), 0xff, vox.size() * sizeof(float));
    const int32_t status = pil_host_pillarize(points.data(), offsets.data(), B, hd[1], gr[0], gr[1], gr[2], gr[3], gr[4], gr[5], (int)hd[2],
                                              (int)hd[3], N, (int)hd[5], vox.data(), coords.data(), num.data(), (long long)cap, poff.data());
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&status, 4, 1, o);
    fwrite(poff.data(), 4, poff.size(), o);
    if (cap) {
        fwrite(num.data(), 4, num.size(), o);
        fwrite(coords.data(), 4, coords.size(), o);
        fwrite(vox.data(), 4, vox.size(), o);
    }
    fclose(o);
    return 0;
}
#endif
