// The per-element formula of BatchNorm's backward, second pass (mcav_bn_bwd_apply):
//   dx = (gamma * invstd) * (g - s1 * inv_count - xhat * (s2 * inv_count)),  xhat = (x - mean) * invstd,
// g the (masked) incoming gradient, s1 / s2 the per-channel sums of g and g * xhat that mcav_bn_bwd_finalize leaves.
// One function for every kernel that evaluates it (bn_bwd_apply_kernel; the depth stem's weight gradient, which applies it to its dy tile on
// the way into LDS), written with explicit roundings so that contraction cannot differ between callers: the operations are the ones the
// compiler chose for bn_bwd_apply_kernel's expression under -ffp-contract=fast (both subtractions fused into the products that feed them).
#pragma once
#include "conv_gather.h"

namespace mcav {

// the two products that depend on the channel (and group) only: callers with fixed channels hoist them
__device__ __forceinline__ void bn_bwd_dx_coeffs(f32x4 gamma, f32x4 invstd, f32x4 s2, float inv_count, f32x4& gi, f32x4& t2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        gi[e] = __fmul_rn(gamma[e], invstd[e]);
        t2[e] = __fmul_rn(s2[e], inv_count);
    }
}

// gi = gamma * invstd, t2 = s2 * inv_count (bn_bwd_dx_coeffs)
__device__ __forceinline__ f32x4 bn_bwd_dx(f32x4 g, f32x4 x, f32x4 mean, f32x4 invstd, f32x4 gi, f32x4 s1, float inv_count, f32x4 t2) {
    f32x4 dx;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xh = __fmul_rn(__fsub_rn(x[e], mean[e]), invstd[e]);
        const float a = __fmaf_rn(-s1[e], inv_count, g[e]);           // g - s1 * inv_count, one rounding
        dx[e] = __fmul_rn(gi[e], __fmaf_rn(-xh, t2[e], a));           // ... - xhat * t2, one rounding
    }
    return dx;
}

}  // namespace mcav
