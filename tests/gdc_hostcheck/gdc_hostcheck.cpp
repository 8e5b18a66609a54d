// csrc/gdc_math.h compiled for the host (g++ -ffp-contract=off): the graph of mcav_gdc_graph, pixel by pixel, with the header's validity
// tests, back-projection, squared distance, ordered insertion and closed-form weights, to be held against tests/gdc_ref.py bit for bit.
// Built as a shared library for the tests, and with -DGDC_STANDALONE as a program of its own (in.bin -> out.bin) for the sanitizer run.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gdc_math.h"

using namespace mcav::gdc;

template <int KC>
static void graph_image(const float* depth, const float* sparse, const float* K, int H, int W, const Params& pr, int* nbr, float* weights,
                        unsigned char* flags) {
    std::vector<Point> pts((size_t)H * W);
    std::vector<char> ok((size_t)H * W);
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const size_t i = (size_t)v * W + u;
            ok[i] = in_range(depth[i], pr.min_depth, pr.max_depth);
            pts[i] = ok[i] ? back_project(u, v, depth[i], K[0], K[1], K[2], K[3]) : Point{0.0f, 0.0f, 0.0f};
        }
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const size_t i = (size_t)v * W + u;
            float bd[KC], w[KC], dz[KC];
            int bi[KC];
            best_init<KC>(bd, bi);
            if (ok[i])
                for (int y = v - pr.radius; y <= v + pr.radius; ++y)
                    for (int x = u - pr.radius; x <= u + pr.radius; ++x) {
                        if (y < 0 || y >= H || x < 0 || x >= W) continue;
                        const size_t j = (size_t)y * W + x;
                        if (j == i || !ok[j]) continue;
                        best_insert<KC>(bd, bi, dist2(pts[i], pts[j]), (int)j);
                    }
            int m = 0;
            for (int s = 0; s < KC; ++s) {
                const bool used = s < pr.k && bi[s] >= 0;
                m += used ? 1 : 0;
                dz[s] = used ? pts[bi[s]].z - pts[i].z : 0.0f;
            }
            lle_weights<KC>(dz, m, pr.k, pr.reg, w);
            for (int s = 0; s < pr.k; ++s) {
                nbr[i * pr.k + s] = s < m ? bi[s] : -1;
                weights[i * pr.k + s] = w[s];
            }
            const bool known = ok[i] && in_range(sparse[i], pr.min_depth, pr.max_depth);
            flags[i] = (unsigned char)((m > 0 ? IN_GRAPH : 0) | (known ? KNOWN : 0));
        }
}

extern "C" int gdc_host_graph(const float* depth, const float* sparse, const float* K, int B, int H, int W, int k, int radius, float reg,
                              float min_depth, float max_depth, int* nbr, float* weights, unsigned char* flags) {
    const Params pr{reg, min_depth, max_depth, k, radius};
    if (!params_ok(pr) || B < 1 || H < 1 || W < 1) return -1;
    const size_t n = (size_t)H * W;
    for (int b = 0; b < B; ++b) {
        const float *d = depth + b * n, *s = sparse + b * n, *Kb = K + 4 * b;
        int* nb = nbr + b * n * k;
        float* wb = weights + b * n * k;
        unsigned char* fb = flags + b * n;
        if (k <= 4) graph_image<4>(d, s, Kb, H, W, pr, nb, wb, fb);
        else if (k <= 8) graph_image<8>(d, s, Kb, H, W, pr, nb, wb, fb);
        else if (k <= 12) graph_image<12>(d, s, Kb, H, W, pr, nb, wb, fb);
        else graph_image<16>(d, s, Kb, H, W, pr, nb, wb, fb);
    }
    return 0;
}

extern "C" int gdc_host_params_ok(int k, int radius, float reg, float min_depth, float max_depth) {
    return params_ok(Params{reg, min_depth, max_depth, k, radius}) ? 1 : 0;
}

#ifdef GDC_STANDALONE
// in.bin: int32 B H W k radius, float32 reg min_depth max_depth, depth, sparse, K.  out.bin: int32 rc, nbr, weights, flags.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int head[5];
    float par[3];
    if (fread(head, sizeof(int), 5, f) != 5 || fread(par, sizeof(float), 3, f) != 3) return 2;
    const int B = head[0], H = head[1], W = head[2], k = head[3], radius = head[4];
    if (B < 1 || H < 1 || W < 1 || k < 1 || k > MAX_K) return 2;
    const size_t N = (size_t)B * H * W;
    std::vector<float> depth(N), sparse(N), K((size_t)B * 4), weights(N * k);
    std::vector<int> nbr(N * k);
    std::vector<unsigned char> flags(N);
    if (fread(depth.data(), 4, N, f) != N || fread(sparse.data(), 4, N, f) != N || fread(K.data(), 4, K.size(), f) != K.size()) return 2;
    fclose(f);
    const int rc = gdc_host_graph(depth.data(), sparse.data(), K.data(), B, H, W, k, radius, par[0], par[1], par[2], nbr.data(), weights.data(),
                                  flags.data());
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&rc, sizeof(int), 1, f);
    fwrite(nbr.data(), 4, nbr.size(), f);
    fwrite(weights.data(), 4, weights.size(), f);
    fwrite(flags.data(), 1, flags.size(), f);
    fclose(f);
    return 0;
}
#endif
