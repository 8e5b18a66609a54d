// TEST INFRASTRUCTURE (CPU): drives the per-pixel math of csrc/augment_math.h -- the functions the augmentation kernels (csrc/augment.hip)
// call -- with plain host loops.  Built by tests/test_augment_cpu.py with g++ -ffp-contract=off; never loaded by the product.
#include <cstddef>
#include <cstdint>

#include "augment_math.h"

using namespace mcav;

// out[i] = L(rgb[i])
extern "C" void au_luma(const uint8_t* rgb, int n, int* out) {
    for (int i = 0; i < n; ++i) out[i] = au::luma(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}

// out[i] = blend(a[i], b[i], alpha)
extern "C" void au_blend(const uint8_t* a, const uint8_t* b, int n, float alpha, uint8_t* out) {
    for (int i = 0; i < n; ++i) out[i] = (uint8_t)au::blend(a[i], b[i], alpha);
}

// Pillow's RGB -> HSV
extern "C" void au_rgb_to_hsv(const uint8_t* rgb, int n, uint8_t* hsv) {
    for (int i = 0; i < n; ++i) {
        int h, s, v;
        au::rgb_to_hsv(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], h, s, v);
        hsv[3 * i] = (uint8_t)h, hsv[3 * i + 1] = (uint8_t)s, hsv[3 * i + 2] = (uint8_t)v;
    }
}

// op applied in place to every pixel: 0..3 as MCAV_AUG_OP_* (contrast with the given grey `mean`)
extern "C" void au_op(uint8_t* rgb, int n, int op, float factor, int shift, int mean) {
    for (int i = 0; i < n; ++i) {
        int r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        if (op == au::OP_CONTRAST) au::contrast(mean, factor, r, g, b);
        else au::pointwise(op, factor, shift, r, g, b);
        rgb[3 * i] = (uint8_t)r, rgb[3 * i + 1] = (uint8_t)g, rgb[3 * i + 2] = (uint8_t)b;
    }
}

extern "C" int au_contrast_mean(uint64_t sum_l, uint64_t n) { return au::contrast_mean(sum_l, n); }
