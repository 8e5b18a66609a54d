// Per-pixel arithmetic of monodepth2's colour jitter (mcav_image_preprocess_augment, include/mcav_depth.h), shared by the HIP kernels
// (augment.hip) and by the host-compiled check in tests/augment_hostcheck (never by the product).  The definition is tests/augment_ref.py:
// Pillow's convert("L"), ImagingBlend (ImageEnhance.Brightness / Contrast / Color) and the RGB <-> HSV conversions behind torchvision's
// adjust_hue, each reading and writing uint8.  Every float32 and float64 operation is rounded on its own, in Pillow's promotion order:
// contraction is switched off in the functions (clang) and for the host-compiled check (g++ -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MCAV_AU_HD __host__ __device__ __forceinline__
#else
#define MCAV_AU_HD inline
#endif
// HIP compiles with fp-contract=fast: a product and a sum that both allow it fuse into an FMA, one rounding instead of two.  Every
// function below that multiplies or adds switches contraction off for its body.
#if defined(__clang__)
#define MCAV_AU_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MCAV_AU_NO_CONTRACT
#endif

namespace mcav {
namespace au {

// Rounded float32 / float64 operations.  Plain operators under the pragma: __fmul_rn and its kin lower to the same IR operations as the
// operators, with the contraction flag of the header that defines them, and fuse all the same.
MCAV_AU_HD float fmul(float a, float b) {
    MCAV_AU_NO_CONTRACT
    return a * b;
}
MCAV_AU_HD float fadd(float a, float b) {
    MCAV_AU_NO_CONTRACT
    return a + b;
}
MCAV_AU_HD float fdiv(float a, float b) {
    MCAV_AU_NO_CONTRACT
    return a / b;
}
MCAV_AU_HD double dmul(double a, double b) {
    MCAV_AU_NO_CONTRACT
    return a * b;
}
MCAV_AU_HD double dadd(double a, double b) {
    MCAV_AU_NO_CONTRACT
    return a + b;
}
MCAV_AU_HD double dsub(double a, double b) {
    MCAV_AU_NO_CONTRACT
    return a - b;
}
MCAV_AU_HD double ddiv(double a, double b) {
    MCAV_AU_NO_CONTRACT
    return a / b;
}

// The operation ids of mcav_augment_record.order (include/mcav_depth.h: MCAV_AUG_OP_*).
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };

// convert("L"): ITU-R 601-2 luma in 16-bit fixed point.
MCAV_AU_HD int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ImagingBlend: a + alpha * (b - a) in float32; truncated for 0 <= alpha <= 1, clipped to [0, 255] and truncated otherwise.
MCAV_AU_HD int blend(int a, int b, float alpha) {
    MCAV_AU_NO_CONTRACT
    const float t = fadd((float)a, fmul(alpha, (float)(b - a)));
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

MCAV_AU_HD int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's rgb2hsv_row (Convert.c): float quotients, the hue sum in double stored to float, fmod in double.
MCAV_AU_HD void rgb_to_hsv(int r, int g, int b, int& h8, int& s8, int& v8) {
    MCAV_AU_NO_CONTRACT
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    v8 = maxc;
    if (minc == maxc) {
        h8 = 0;
        s8 = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = fdiv(cr, (float)maxc);
    const float rc = fdiv((float)(maxc - r), cr), gc = fdiv((float)(maxc - g), cr), bc = fdiv((float)(maxc - b), cr);
    float h;
    if (r == maxc) h = bc - gc;                                                 // float - float: one rounding
    else if (g == maxc) h = (float)dsub(dadd(2.0, (double)rc), (double)bc);
    else h = (float)dsub(dadd(4.0, (double)gc), (double)rc);
    h = (float)fmod(dadd(ddiv((double)h, 6.0), 1.0), 1.0);
    h8 = clip8((int)dmul((double)h, 255.0));
    s8 = clip8((int)dmul((double)s, 255.0));
}

// C round(): half away from zero (the arguments here are never negative).
MCAV_AU_HD int round_half_away(double x) {
    MCAV_AU_NO_CONTRACT
    const double f = floor(x);
    return (int)f + (dsub(x, f) >= 0.5 ? 1 : 0);
}

// Pillow's hsv2rgb (Convert.c).
MCAV_AU_HD void hsv_to_rgb(int h8, int s8, int v8, int& r, int& g, int& b) {
    MCAV_AU_NO_CONTRACT
    if (s8 == 0) {
        r = g = b = v8;
        return;
    }
    const double h6 = ddiv(dmul((double)(float)h8, 6.0), 255.0);
    const int i = (int)floor(h6);
    const float f = (float)dsub(h6, (double)(float)i);
    const float fs = (float)ddiv((double)(float)s8, 255.0);
    const double v = (double)(float)v8;
    const int p = clip8(round_half_away(dmul(v, dsub(1.0, (double)fs))));
    const int q = clip8(round_half_away(dmul(v, dsub(1.0, (double)fmul(fs, f)))));
    const int t = clip8(round_half_away(dmul(v, dsub(1.0, dmul((double)fs, dsub(1.0, (double)f))))));
    switch (i % 6) {
        case 0: r = v8; g = t; b = p; break;
        case 1: r = q; g = v8; b = p; break;
        case 2: r = p; g = v8; b = t; break;
        case 3: r = p; g = q; b = v8; break;
        case 4: r = t; g = p; b = v8; break;
        default: r = v8; g = p; b = q; break;
    }
}

// torchvision F_pil.adjust_hue: HSV, H += shift with uint8 wrap-around, back to RGB.  shift = trunc(hue_factor * 255) mod 256.
MCAV_AU_HD void hue(int& r, int& g, int& b, int shift) {
    int h8, s8, v8;
    rgb_to_hsv(r, g, b, h8, s8, v8);
    hsv_to_rgb((h8 + shift) & 255, s8, v8, r, g, b);
}

// One pointwise operation (everything but contrast, whose degenerate image needs the frame's mean).
MCAV_AU_HD void pointwise(int op, float factor, int shift, int& r, int& g, int& b) {
    if (op == OP_BRIGHTNESS) {
        r = blend(0, r, factor);
        g = blend(0, g, factor);
        b = blend(0, b, factor);
    } else if (op == OP_SATURATION) {
        const int l = luma(r, g, b);
        r = blend(l, r, factor);
        g = blend(l, g, factor);
        b = blend(l, b, factor);
    } else if (op == OP_HUE) {
        hue(r, g, b, shift);
    }
}

// ImageEnhance.Contrast's degenerate grey: int(mean(L) + 0.5) with the mean S / n in float64 (ImageStat), S the exact integer sum.
MCAV_AU_HD int contrast_mean(uint64_t sum_l, uint64_t n) {
    MCAV_AU_NO_CONTRACT
    return (int)dadd(ddiv((double)sum_l, (double)n), 0.5);
}

MCAV_AU_HD void contrast(int m, float factor, int& r, int& g, int& b) {
    r = blend(m, r, factor);
    g = blend(m, g, factor);
    b = blend(m, b, factor);
}

}  // namespace au
}  // namespace mcav
