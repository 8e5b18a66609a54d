// TEST INFRASTRUCTURE (CPU): drives the per-pixel math of csrc/edge_math.h -- the functions the edge-aware smoothness kernels
// (csrc/edge_smooth.hip) call -- with plain host loops, in the kernels' arithmetic: fp32 per pixel, float64 per-sample sums.  Built by
// tests/test_edge_smooth_cpu.py with g++; never loaded by the product.
#include <cstddef>

#include "edge_math.h"

using namespace mcav;

// loss = weight * E; grad = upstream * weight * dE/dd.  disp [B,1,h,w], img [B,3,H,W], f = H / h (the caller checks the shape).
extern "C" int edge_hostcheck(const float* disp, const float* img, int B, int H, int W, int h, int w, float weight, float upstream,
                              double* loss, float* grad) {
    const int f = H / h;
    const size_t n = (size_t)h * w, hw_full = (size_t)H * W;
    float cx, cy;
    es::pair_scales(B, h, w, cx, cy);
    double e = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* dp = disp + b * n;
        const float* ip = img + b * 3 * hw_full;
        auto D = [&](int y, int x) { return dp[(size_t)y * w + x]; };
        auto C = [&](int y, int x) { return es::rgb_at(ip, hw_full, W, f, y, x); };
        double sm = 0.0, sr = 0.0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                sm += D(y, x);
                sr += es::pixel_loss(D, C, y, x, h, w, cx, cy);
            }
        const double m = sm / (double)n;
        e += es::sample_loss(m, sr);
        float inv, k;
        es::grad_factors(m, sr, h, w, inv, k);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                grad[b * n + (size_t)y * w + x] = upstream * weight * es::pixel_grad(es::pixel_stencil(D, C, y, x, h, w, cx, cy), inv, k);
    }
    *loss = (double)weight * e;
    return 0;
}
