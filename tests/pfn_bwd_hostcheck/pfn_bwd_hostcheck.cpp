// TEST INFRASTRUCTURE (CPU): drives csrc/pfn_bwd_math.h -- the functions the pillar feature net's backward kernels (csrc/pfn_bwd.hip) call
// -- with plain host loops in the kernel's order: chunks of BWD_CHUNK rows dealt to the workgroups of the fixed grid, a chunk's rows dealt
// to the wavefronts, per row the winner of every channel, its terms into the wavefront's float64 accumulators, d_voxels from (g, slot);
// then the wavefronts' accumulators in order into the slab, and a slab row added as the second kernel's lanes add it.
// Built by tests/test_pfn_bwd_cpu.py with g++ -ffp-contract=off, as a shared library and (with -DPFN_BWD_STANDALONE) as a program that
// reads one case from a file and writes its result to another, which is the form that runs under the sanitizers.  Never loaded by the
// product.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pfn_bwd_math.h"

using namespace mcav;

static const int WAVES = 4;              // csrc/pfn_bwd.hip

// The whole call on the host.  -1: refused.  flags & 1: d_canvas [B, ny, nx, c_out].  d_voxels and slots (int32 [capacity, c_out]:
// win_slot of the rows below P, untouched behind them) may be null.
extern "C" int pfn_bwd_host(const float* voxels, const int* coords, const int* num_points, const int* pillar_offsets, int B,
                            long long capacity, int N, int C, int nx, int ny, const float* weight, const float* bias, const float* bias_pad,
                            int c_out, int flags, const float* d_canvas, const float* d_features, float* d_weight, float* d_bias,
                            float* d_bias_pad, float* d_voxels, int* slots) {
    if (!voxels || !coords || !num_points || !pillar_offsets || !weight || !bias || !bias_pad || (!d_canvas && !d_features)) return -1;
    if (!d_weight || !d_bias || !d_bias_pad) return -1;
    if (B <= 0 || B > 65535 || capacity < 0 || nx < 1 || ny < 1 || N < 1 || N > pfn::MAX_POINTS) return -1;
    if ((unsigned long long)B * (unsigned long long)ny * (unsigned long long)nx > 0x7fffffffull) return -1;
    if (!pfn::columns_ok(C) || !pfn::c_out_ok(c_out) || (flags & ~1)) return -1;
    const bool nhwc = flags & 1;
    const long long P = pfn::live_pillars(pillar_offsets, B, capacity);
    const int G = pfn::bwd_grid(capacity), S = pfn::bwd_sums(C);
    const long long rows = P;
    if (d_voxels)                                                                // behind the last pillar: zeros up to the capacity
        for (size_t e = (size_t)P * N * C; e < (size_t)capacity * N * C; ++e) d_voxels[e] = 0.0f;
    std::vector<double> slab((size_t)c_out * S * G, 0.0), acc((size_t)WAVES * c_out * S);
    std::vector<float> g((size_t)c_out);
    std::vector<int> slot((size_t)c_out);
    for (int block = 0; block < G; ++block) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (long long r0 = (long long)block * pfn::BWD_CHUNK; r0 < rows; r0 += (long long)G * pfn::BWD_CHUNK)
            for (int i = 0; i < pfn::BWD_CHUNK; ++i) {
                const long long r = r0 + i;
                if (r >= rows) break;
                float* out = d_voxels ? d_voxels + (size_t)r * N * C : nullptr;
                double* mine = acc.data() + (size_t)(i % WAVES) * c_out * S;
                const int n = pfn::used_slots(num_points[r], N);
                const float* x = voxels + (size_t)r * N * C;
                const bool in = d_canvas && pfn::cell_inside(coords, r, B, ny, nx);
                for (int o = 0; o < c_out; ++o) {
                    const float part = in ? d_canvas[pfn::canvas_index(nhwc, coords[4 * r], o, coords[4 * r + 2], coords[4 * r + 3], c_out, ny, nx)] : 0.0f;
                    g[o] = pfn::upstream(part, d_features != nullptr, d_features ? d_features[(size_t)r * c_out + o] : 0.0f);
                    slot[o] = pfn::win_slot(pfn::winner(x, n, N, C, weight + (size_t)o * C, bias[o], bias_pad[o]));
                    if (slots) slots[(size_t)r * c_out + o] = slot[o];
                    double* s = mine + (size_t)o * S;
                    if (slot[o] >= 0) {
                        s[C] += (double)g[o];
                        for (int c = 0; c < C; ++c) s[c] += (double)g[o] * (double)x[(size_t)slot[o] * C + c];
                    } else if (slot[o] == pfn::PADDING) {
                        s[C + 1] += (double)g[o];
                    }
                }
                if (out)
                    for (int e = 0; e < N * C; ++e) out[e] = e < n * C ? pfn::d_voxel(g, slot, weight, c_out, C, e / C, e % C) : 0.0f;
            }
        for (int q = 0; q < c_out * S; ++q) {                                    // wavefront 0's, then 1's, 2's, 3's
            double v = acc[q];
            for (int w = 1; w < WAVES; ++w) v += acc[(size_t)w * c_out * S + q];
            slab[(size_t)q * G + block] = v;
        }
    }
    for (int q = 0; q < c_out * S; ++q) {                                        // lane l: columns l, l + 64, ...; then the butterfly
        double lane[64], next[64];
        for (int l = 0; l < 64; ++l) {
            lane[l] = 0.0;
            for (int c = l; c < G; c += 64) lane[l] += slab[(size_t)q * G + c];
        }
        for (int off = 32; off > 0; off >>= 1) {
            for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ off];
            memcpy(lane, next, sizeof(lane));
        }
        const int o = q / S, s = q % S;
        (s < C ? d_weight[o * C + s] : (s == C ? d_bias[o] : d_bias_pad[o])) = (float)lane[0];
    }
    return 0;
}

#ifdef PFN_BWD_STANDALONE
// in : int64 [12] = B capacity N C nx ny c_out flags has_canvas has_features want_voxels 0; int32 offsets [B + 1]; int32 num_points
//      [capacity]; int32 coords [capacity, 4]; float32 voxels [capacity, N, C]; float32 weight [c_out, C], bias [c_out], bias_pad [c_out];
//      float32 d_canvas [B * c_out * ny * nx] if has_canvas; float32 d_features [capacity, c_out] if has_features
// out: int32 status; float32 d_weight, d_bias, d_bias_pad; float32 d_voxels [capacity, N, C] if asked for; int32 slots [capacity, c_out]
//      (the last two 0xff-filled where nothing was written)
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
    if (!rd(f, hd, 12)) return 2;
    const int B = (int)hd[0], N = (int)hd[2], C = (int)hd[3], nx = (int)hd[4], ny = (int)hd[5], c_out = (int)hd[6];
    const size_t cap = (size_t)hd[1];
    std::vector<int32_t> offsets, num, coords;
    std::vector<float> vox, weight, bias, pad, dc, df;
    const bool ok = rd(f, offsets, (size_t)B + 1) && rd(f, num, cap) && rd(f, coords, cap * 4) && rd(f, vox, cap * N * C) &&
                    rd(f, weight, (size_t)c_out * C) && rd(f, bias, (size_t)c_out) && rd(f, pad, (size_t)c_out) &&
                    rd(f, dc, hd[8] ? (size_t)B * c_out * ny * nx : 0) && rd(f, df, hd[9] ? cap * c_out : 0);
    fclose(f);
    if (!ok) return 2;
    std::vector<float> dw((size_t)c_out * C), db((size_t)c_out), dp((size_t)c_out), dv(hd[10] ? cap * N * C : 0);
    std::vector<int32_t> slots(cap * c_out);
    if (!dv.empty()) memset(dv.data(), 0xff, dv.size() * sizeof(float));
    if (!slots.empty()) memset(slots.data(), 0xff, slots.size() * sizeof(int32_t));
    const int32_t status = pfn_bwd_host(vox.data(), coords.data(), num.data(), offsets.data(), B, (long long)cap, N, C, nx, ny, weight.data(),
                                        bias.data(), pad.data(), c_out, (int)hd[7], hd[8] ? dc.data() : nullptr, hd[9] ? df.data() : nullptr,
                                        dw.data(), db.data(), dp.data(), hd[10] ? dv.data() : nullptr, slots.data());
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&status, 4, 1, o);
    fwrite(dw.data(), 4, dw.size(), o);
    fwrite(db.data(), 4, db.size(), o);
    fwrite(dp.data(), 4, dp.size(), o);
    if (!dv.empty()) fwrite(dv.data(), 4, dv.size(), o);
    if (!slots.empty()) fwrite(slots.data(), 4, slots.size(), o);
    fclose(o);
    return 0;
}
#endif
