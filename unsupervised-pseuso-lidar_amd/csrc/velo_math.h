// Per-point arithmetic of the Velodyne -> sparse depth map projection (mcav_velo_depth_map, include/mcav_depth.h), shared by the HIP
// kernels (velo_depth.hip) and by the host-compiled check in tests/velo_hostcheck (never by the product).  The definition is
// tests/velo_ref.py: keep x >= 0, q = P (x, y, z, 1) in float64 in a fixed order, pixel = rint(q / q2) - 1 (half to even), depth q2 (or x),
// minimum per pixel through an order-preserving 32-bit key.  Every float64 operation is rounded on its own: contraction is switched off in
// the functions (clang) and for the host-compiled check (g++ -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MCAV_VD_HD __host__ __device__ __forceinline__
#else
#define MCAV_VD_HD inline
#endif
// HIP compiles with fp-contract=fast: a product and a sum that both allow it fuse into an FMA, one rounding instead of two.  Every
// function below that multiplies or adds switches contraction off for its body.
#if defined(__clang__)
#define MCAV_VD_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MCAV_VD_NO_CONTRACT
#endif

namespace mcav {
namespace vd {

// The key of a pixel that no point has reached.  A landing point's depth is never NaN (a NaN coordinate fails the x test or makes the
// pixel NaN, which fails the bounds test), so no depth has this key; +inf (a float64 depth above FLT_MAX) has a smaller one.
constexpr uint32_t EMPTY_KEY = 0xffffffffu;

// q_k = ((P[k,0] x + P[k,1] y) + P[k,2] z) + P[k,3], each product and sum rounded to float64 on its own
MCAV_VD_HD double project_row(const double* Pk, double x, double y, double z) {
    MCAV_VD_NO_CONTRACT
    const double a = Pk[0] * x;
    const double b = Pk[1] * y;
    const double c = Pk[2] * z;
    const double d = a + b;
    const double e = d + c;
    return e + Pk[3];
}

// np.round(q / q2) - 1: IEEE division, round half to even (rint in the default rounding mode), then the subtraction
MCAV_VD_HD double pixel_coord(double q, double q2) {
    MCAV_VD_NO_CONTRACT
    const double r = rint(q / q2);
    return r - 1.0;
}

// float32 bits -> a key whose unsigned order is the float order (-0.0 below +0.0); no NaN reaches it
MCAV_VD_HD uint32_t depth_key(float d) {
    uint32_t bits;
    memcpy(&bits, &d, 4);
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// The output value of a pixel's minimum key: +0.0 without a point and for a minimum with the sign bit set (monodepth2's depth[depth < 0] = 0)
MCAV_VD_HD float key_depth(uint32_t key) {
    if (key == EMPTY_KEY || !(key & 0x80000000u)) return 0.0f;
    const uint32_t bits = key & 0x7fffffffu;
    float d;
    memcpy(&d, &bits, 4);
    return d;
}

// One point of image (Hb, Wb): true when it lands, with the pixel (u, v) before any flip and the key of its float32 depth.
MCAV_VD_HD bool project_point(float x, float y, float z, const double* P, int Hb, int Wb, bool depth_from_x, int& u, int& v, uint32_t& key) {
    if (!(x >= 0.0f)) return false;                     // NaN fails, -0.0 passes
    const double X = (double)x, Y = (double)y, Z = (double)z;
    const double q0 = project_row(P, X, Y, Z);
    const double q1 = project_row(P + 4, X, Y, Z);
    const double q2 = project_row(P + 8, X, Y, Z);
    const double uf = pixel_coord(q0, q2), vf = pixel_coord(q1, q2);
    if (!(uf >= 0.0 && vf >= 0.0 && uf < (double)Wb && vf < (double)Hb)) return false;     // float64: NaN and +-inf fail
    u = (int)uf;
    v = (int)vf;
    key = depth_key((float)(depth_from_x ? X : q2));
    return true;
}

}  // namespace vd
}  // namespace mcav
