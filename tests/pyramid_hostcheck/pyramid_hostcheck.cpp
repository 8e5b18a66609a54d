// TEST INFRASTRUCTURE (CPU): drives the per-pixel math of csrc/pyramid_math.h -- the functions the depth-pyramid kernels
// (csrc/depth_pyramid.hip) call -- with plain host loops in the kernels' arithmetic and order (fp32; the adjoint along x, then along y, each
// in ascending index order).  Built by tests/test_pyramid_cpu.py with g++; never loaded by the product.
#include <cstddef>
#include <vector>

#include "pyramid_math.h"

using namespace mcav;

static float scale_of(int n_in, int n_out) { return (float)n_in / (float)n_out; }

extern "C" void pyr_taps(int o, int h, int H, int* i0, int* i1, float* lam) { pyr::bil_src(o, scale_of(h, H), h, *i0, *i1, *lam); }

extern "C" float pyr_weight(int o, int i, int h, int H) { return pyr::tap_weight(o, i, scale_of(h, H), h); }

extern "C" void pyr_window(int i, int h, int H, int* lo, int* hi) { pyr::adjoint_window(i, scale_of(h, H), h, H, *lo, *hi); }

// out [B,H,W] from disp [B,h,w]
extern "C" void pyr_fwd(const float* disp, int B, int h, int w, int H, int W, int resize_then_depth, float* out) {
    const float sy = scale_of(h, H), sx = scale_of(w, W);
    for (int b = 0; b < B; ++b)
        for (int oy = 0; oy < H; ++oy)
            for (int ox = 0; ox < W; ++ox) {
                int y0, y1, x0, x1;
                float ly, lx;
                pyr::bil_src(oy, sy, h, y0, y1, ly);
                pyr::bil_src(ox, sx, w, x0, x1, lx);
                out[((size_t)b * H + oy) * W + ox] = pyr::fwd_value(disp + (size_t)b * h * w, w, y0, y1, ly, x0, x1, lx, resize_then_depth != 0);
            }
}

// d_disp [B,h,w] from d_out [B,H,W] (and out under resize_then_depth, disp otherwise)
extern "C" void pyr_bwd(const float* disp, const float* out, const float* d_out, int B, int h, int w, int H, int W, int resize_then_depth,
                        float* d_disp) {
    const float sy = scale_of(h, H), sx = scale_of(w, W);
    std::vector<float> xr((size_t)H * w);
    for (int b = 0; b < B; ++b) {
        const float* g = d_out + (size_t)b * H * W;
        const float* D = out + (size_t)b * H * W;
        for (int oy = 0; oy < H; ++oy)
            for (int ix = 0; ix < w; ++ix) {
                int lo, hi;
                pyr::adjoint_window(ix, sx, w, W, lo, hi);
                float acc = 0.f;
                for (int ox = lo; ox <= hi; ++ox) {
                    float v = g[(size_t)oy * W + ox];
                    if (resize_then_depth) v *= pyr::depth_slope(D[(size_t)oy * W + ox]);
                    acc += pyr::tap_weight(ox, ix, sx, w) * v;
                }
                xr[(size_t)oy * w + ix] = acc;
            }
        for (int iy = 0; iy < h; ++iy) {
            int lo, hi;
            pyr::adjoint_window(iy, sy, h, H, lo, hi);
            for (int ix = 0; ix < w; ++ix) {
                float acc = 0.f;
                for (int oy = lo; oy <= hi; ++oy) acc += pyr::tap_weight(oy, iy, sy, h) * xr[(size_t)oy * w + ix];
                const size_t at = ((size_t)b * h + iy) * w + ix;
                if (!resize_then_depth) acc *= pyr::depth_slope(pyr::depth_of(disp[at]));
                d_disp[at] = acc;
            }
        }
    }
}
