// TEST INFRASTRUCTURE (CPU): drives csrc/pfn_stats_math.h -- the functions the moments kernels (csrc/pfn_stats.hip) call -- with plain host
// loops in the kernels' order: groups of STATS_ROWS rows dealt to the wavefronts of the fixed grid, a group's used slots dealt to the
// lanes 64 at a time, a lane's terms into its float64 accumulators; then block_sum's order (the butterfly, the wavefronts from left to
// right) into the slab, and a slab row added as the second kernel's lanes add it.  The adjoint is the header's chain per element.
// Built by tests/test_pfn_stats_cpu.py with g++ -ffp-contract=off, as a shared library and (with -DPFN_STATS_STANDALONE) as a program that
// reads one case from a file and writes its result to another, which is the form that runs under the sanitizers.  Never loaded by the
// product.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pfn_stats_math.h"

using namespace mcav;

static void butterfly(double* lane) {                        // wave_sum: every lane ends with the total
    double next[64];
    for (int off = 32; off > 0; off >>= 1) {
        for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ off];
        memcpy(lane, next, sizeof(next));
    }
}

static bool stats_ok(const void* a, const void* b, const void* c, int B, long long capacity, int N, int C) {
    return a && b && c && B > 0 && B <= 65535 && capacity >= 0 && N >= 1 && N <= pfn::MAX_POINTS && pfn::columns_ok(C);
}

template <int C>
static void moments_host(const float* voxels, const int* num_points, long long P, int N, int G, double* moments) {
    const int S = pfn::stats_sums(C), W = pfn::STATS_WAVES, ROWS = pfn::STATS_ROWS;
    std::vector<double> slab((size_t)S * G), acc((size_t)W * 64 * S);
    for (int block = 0; block < G; ++block) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int wave = 0; wave < W; ++wave)
            for (long long r0 = ((long long)block * W + wave) * ROWS; r0 < P; r0 += (long long)G * W * ROWS) {
                int j = 0;                                   // the group's used slots in (row, slot) order: slot j goes to lane j % 64
                for (int i = 0; i < ROWS && r0 + i < P; ++i) {
                    const int n = pfn::used_slots(num_points[r0 + i], N);
                    acc[((size_t)wave * 64 + i) * S] += (double)n;
                    for (int k = 0; k < n; ++k, ++j) {
                        double* mine = acc.data() + ((size_t)wave * 64 + j % 64) * S;
                        pfn::moments_add<C>(voxels + ((size_t)(r0 + i) * N + k) * C, mine + 1, mine + 1 + C);
                    }
                }
            }
        for (int q = 0; q < S; ++q) {
            double total = 0.0;
            for (int wave = 0; wave < W; ++wave) {
                double lane[64];
                for (int l = 0; l < 64; ++l) lane[l] = acc[((size_t)wave * 64 + l) * S + q];
                butterfly(lane);
                total = wave == 0 ? lane[0] : total + lane[0];
            }
            slab[(size_t)q * G + block] = total;
        }
    }
    moments[0] = (double)(P * N);
    for (int q = 0; q < S; ++q) {
        double lane[64];
        for (int l = 0; l < 64; ++l) {
            lane[l] = 0.0;
            for (int c = l; c < G; c += 64) lane[l] += slab[(size_t)q * G + c];
        }
        butterfly(lane);
        if (q <= C) {
            moments[1 + q] = lane[0];
            continue;
        }
        for (int c = 0; c < C; ++c)
            for (int d = c; d < C; ++d)
                if (pfn::stats_at(C, c, d) == q - 1 - C) moments[2 + C + c * C + d] = moments[2 + C + d * C + c] = lane[0];
    }
}

// -1: refused
extern "C" int pfn_stats_host(const float* voxels, const int* num_points, const int* pillar_offsets, int B, long long capacity, int N, int C,
                              double* moments) {
    if (!stats_ok(voxels, num_points, pillar_offsets, B, capacity, N, C) || !moments) return -1;
    const long long P = pfn::live_pillars(pillar_offsets, B, capacity);
    const int G = pfn::stats_grid(capacity);
    if (C == 4) moments_host<4>(voxels, num_points, P, N, G, moments);
    else moments_host<9>(voxels, num_points, P, N, G, moments);
    return 0;
}

extern "C" int pfn_stats_bwd_host(const float* voxels, const int* num_points, const int* pillar_offsets, int B, long long capacity, int N, int C,
                                  const double* g, const double* H, float* d_voxels) {
    if (!stats_ok(voxels, num_points, pillar_offsets, B, capacity, N, C) || !g || !H || !d_voxels) return -1;
    const long long P = pfn::live_pillars(pillar_offsets, B, capacity);
    std::vector<double> G((size_t)C * C);
    for (int c = 0; c < C; ++c)
        for (int d = 0; d < C; ++d) G[(size_t)c * C + d] = pfn::adjoint_entry(H, C, c, d);
    for (long long r = 0; r < capacity; ++r) {
        const int n = r < P ? pfn::used_slots(num_points[r], N) : 0;
        for (int e = 0; e < N * C; ++e) {
            const int k = e / C, c = e % C;
            d_voxels[(size_t)r * N * C + e] =
                k < n ? pfn::moments_bwd_value(g[c], G.data() + (size_t)c * C, voxels + ((size_t)r * N + k) * C, C) : 0.0f;
        }
    }
    return 0;
}

#ifdef PFN_STATS_STANDALONE
// in : int64 [4] = B capacity N C; int32 offsets [B + 1]; int32 num_points [capacity]; float32 voxels [capacity, N, C]; float64 g [C], H [C, C]
// out: int32 status of the moments, int32 status of the adjoint; float64 moments [2 + C + C C]; float32 d_voxels [capacity, N, C]
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
    if (!rd(f, hd, 4)) return 2;
    const int B = (int)hd[0], N = (int)hd[2], C = (int)hd[3];
    const size_t cap = (size_t)hd[1];
    std::vector<int32_t> offsets, num;
    std::vector<float> vox;
    std::vector<double> gH;
    const bool ok = rd(f, offsets, (size_t)B + 1) && rd(f, num, cap) && rd(f, vox, cap * N * C) && rd(f, gH, (size_t)C + (size_t)C * C);
    fclose(f);
    if (!ok) return 2;
    std::vector<double> moments((size_t)pfn::stats_moments(C), -7.0);
    std::vector<float> dv(cap * N * C, -7.0f);
    const int32_t status[2] = {pfn_stats_host(vox.data(), num.data(), offsets.data(), B, (long long)cap, N, C, moments.data()),
                               pfn_stats_bwd_host(vox.data(), num.data(), offsets.data(), B, (long long)cap, N, C, gH.data(), gH.data() + C,
                                                  dv.data())};
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(status, 4, 2, o);
    fwrite(moments.data(), 8, moments.size(), o);
    if (!dv.empty()) fwrite(dv.data(), 4, dv.size(), o);
    fclose(o);
    return 0;
}
#endif
