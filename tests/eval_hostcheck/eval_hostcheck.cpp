// TEST INFRASTRUCTURE (CPU): drives the per-pixel math of csrc/eval_math.h -- the functions the evaluation kernels (csrc/eval_depth.hip)
// call -- with plain host loops.  Built by tests/test_eval_depth_cpu.py with g++ -ffp-contract=off; never loaded by the product.
#include <cstddef>
#include <cstdint>

#include "eval_math.h"

using namespace mcav;

// out[i] = disp_depth(d[i], scale)
extern "C" void ev_depth(const float* d, float scale, float* out, int n) {
    for (int i = 0; i < n; ++i) out[i] = ev::disp_depth(d[i], scale);
}

// keys[i] = float_key(x[i]); back[i] = key_float(keys[i])
extern "C" void ev_keys(const float* x, uint32_t* keys, float* back, int n) {
    for (int i = 0; i < n; ++i) {
        keys[i] = ev::float_key(x[i]);
        back[i] = ev::key_float(keys[i]);
    }
}

// disp [h, w] resized to [Hb, Wb], one bilinear sample per output pixel
extern "C" void ev_resize(const float* disp, int h, int w, int Hb, int Wb, float* out) {
    const float sy = ev::axis_scale(h, Hb), sx = ev::axis_scale(w, Wb);
    for (int y = 0; y < Hb; ++y)
        for (int x = 0; x < Wb; ++x) out[(size_t)y * Wb + x] = ev::bilinear_sample(disp, h, w, sy, sx, y, x);
}

// np.median of float32 from the two middle order statistics
extern "C" float ev_median(float lo, float hi, uint32_t n) { return ev::median_of(lo, hi, n); }
