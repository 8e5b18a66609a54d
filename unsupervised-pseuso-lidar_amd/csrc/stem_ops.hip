// The depth encoder's stem around conv1 on gfx950: BatchNorm + ReLU + MaxPool 3x3 s2 p1 in one forward pass, and the max-pool backward,
// the ReLU mask and the BatchNorm backward in two passes, on the 64-channel NHWC map that is the largest activation of the network.
// Every kernel here is HBM-bound; what the fusion removes is bytes: the pool's re-read of the activated map, the
// unmasked gradient map that the separate max-pool backward writes for the two BatchNorm passes to read, and both reads of the activated
// map for a sign that the raw convolution output and the BatchNorm coefficients already determine.
// Per element the arithmetic is that of the kernels these replace (nn_ops.hip: bn_apply_kernel, maxpool_fwd_kernel, maxpool_bwd_kernel,
// bn_bwd_reduce_kernel, bn_bwd_apply_kernel), expression for expression and in the same order, so results are bit-identical to theirs
// (tests/test_stem_fused_gpu.py).
#include "conv_gather.h"

namespace mcav {

constexpr int STEM_C = 64, STEM_C4 = STEM_C / 4;      // channels of the stem; 16-byte chunks per pixel
constexpr int STEM_TILE = 4;                          // a workgroup owns STEM_TILE x STEM_TILE pooled outputs (16 outputs x 16 chunks = 256 threads)
constexpr int STEM_RED_BLOCKS = 1024;                 // per-group partial-sum blocks of the backward reduce (= BNR_BLOCKS: mcav_bn_bwd_workspace_bytes)

// bn_apply_kernel's expression (relu = 1, no residual)
__device__ __forceinline__ f32x4 stem_bn_relu(f32x4 x, f32x4 scale, f32x4 shift) {
    f32x4 v = x * scale + shift;
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    return v;
}

// ---------------------------------------------------------------------------------------------- forward
// A workgroup owns a 4 x 4 block of pooled outputs and the 9 x 9 band of input pixels under it; a thread owns one pooled output for four
// channels.  Each of its nine taps is read from x (the raw convolution output) and activated in registers; the band's first row and
// column belong to the neighbouring workgroups' windows too and are recomputed here (cache hits), while y is written once per pixel, by
// the thread whose window holds it at ky, kx >= 1 (pixel rows 2 oy, 2 oy + 1: every row r has r >> 1 < Ho).  The window scan is
// maxpool_fwd_kernel's: the first in-bounds element initialises, a later one wins when greater or NaN, taps in ky-major order.
__global__ __launch_bounds__(256) void stem_bn_relu_pool_fwd_kernel(const float* __restrict__ x, const f32x4* __restrict__ scale,
                                                                    const f32x4* __restrict__ shift, int H, int W, int Ho, int Wo, int tiles_y,
                                                                    int tiles_x, int img_per_group, float* __restrict__ y, float* __restrict__ pooled,
                                                                    uint8_t* __restrict__ idx) {
    const int c = threadIdx.x & (STEM_C4 - 1), t = threadIdx.x / STEM_C4;
    int tile = blockIdx.x;
    const int tx = tile % tiles_x; tile /= tiles_x;
    const int ty = tile % tiles_y;
    const int b = tile / tiles_y;
    const int oy = ty * STEM_TILE + t / STEM_TILE, ox = tx * STEM_TILE + t % STEM_TILE;
    if (oy >= Ho || ox >= Wo) return;
    const int ci = (b / img_per_group) * STEM_C4 + c;
    const f32x4 sc = scale[ci], sh = shift[ci];
    const float ninf = -__builtin_huge_valf();
    f32x4 best = {ninf, ninf, ninf, ninf};
    int bi[4] = {0, 0, 0, 0};
    bool first[4] = {true, true, true, true};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - 1 + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - 1 + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const size_t o = ((size_t)(b * H + iy) * W + ix) * STEM_C + c * 4;
            const f32x4 v = stem_bn_relu(*reinterpret_cast<const f32x4*>(x + o), sc, sh);
            if (ky >= 1 && kx >= 1) *reinterpret_cast<f32x4*>(y + o) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (first[e] || v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bi[e] = ky * 3 + kx; first[e] = false; }
            }
        }
    }
    const size_t po = ((size_t)(b * Ho + oy) * Wo + ox) * STEM_C + c * 4;
    *reinterpret_cast<f32x4*>(pooled + po) = best;
    uchar4 k;
    k.x = (uint8_t)bi[0]; k.y = (uint8_t)bi[1]; k.z = (uint8_t)bi[2]; k.w = (uint8_t)bi[3];
    *reinterpret_cast<uchar4*>(idx + po) = k;
}

// ---------------------------------------------------------------------------------------------- backward
// The gradient arriving at the BatchNorm's pre-activation output for one pixel and four channels: maxpool_bwd_kernel's gather of the (up to
// four) pooled gradients whose idx names this pixel, added to the gradient that reaches the activated map from elsewhere (the decoder's skip
// connection), then relu_mask() with the activation recomputed from x -- (x * scale + shift > 0) is the bit (y > 0) of the stored map.
__device__ __forceinline__ f32x4 stem_masked_grad(f32x4 dyv, const float* dpooled, const uint8_t* idx, f32x4 xv, f32x4 sc, f32x4 sh, int b, int iy,
                                                  int ix, int c, int Ho, int Wo) {
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    const int oy_lo = iy >> 1, oy_hi = (iy + 1) >> 1;
    const int ox_lo = ix >> 1, ox_hi = (ix + 1) >> 1;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        if (oy >= Ho) continue;
        const int ky = iy - (oy * 2 - 1);
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            if (ox >= Wo) continue;
            const int kx = ix - (ox * 2 - 1);
            const int tap = ky * 3 + kx;
            const unsigned o = ((unsigned)(b * Ho + oy) * Wo + ox) * STEM_C + c * 4;      // (stem_shape_ok: 32-bit offsets)
            const uchar4 k = *reinterpret_cast<const uchar4*>(idx + o);
            const f32x4 d = *reinterpret_cast<const f32x4*>(dpooled + o);
            if (k.x == tap) g.x += d.x;
            if (k.y == tap) g.y += d.y;
            if (k.z == tap) g.z += d.z;
            if (k.w == tap) g.w += d.w;
        }
    }
    g = dyv + g;
    const f32x4 v = xv * sc + sh;
    g.x = v.x > 0.f ? g.x : 0.f; g.y = v.y > 0.f ? g.y : 0.f; g.z = v.z > 0.f ? g.z : 0.f; g.w = v.w > 0.f ? g.w : 0.f;
    return g;
}

// Pass A: per-block partial sums of dz and dz * xhat, bn_bwd_reduce_kernel's partition and order (a block takes a contiguous run of a
// group's pixels, 16 pixel lanes x 16 channel chunks, partials through LDS in lane order; no atomics), with dz gathered and masked in
// registers.  kStore: dz is also left in dy (in place: a thread overwrites the element it has just read) for mcav_bn_bwd_apply to read.
// 8 waves per SIMD (64 registers): the 2 x 1024 blocks of a stacked pass are resident at once, as bn_bwd_reduce_kernel's are.
template <bool kStore>
__global__ __launch_bounds__(256, 8) void stem_pool_bn_bwd_reduce_kernel(float* dy, const float* __restrict__ dpooled, const uint8_t* __restrict__ idx,
                                                                      const float* __restrict__ x, const f32x4* __restrict__ scale,
                                                                      const f32x4* __restrict__ shift, const f32x4* __restrict__ mean,
                                                                      const f32x4* __restrict__ invstd, int H, int W, int Ho, int Wo,
                                                                      unsigned n_pix /* per group */, float* __restrict__ part /* [groups][blocks][2][C] */) {
    __shared__ f32x4 sh[2][256];
    constexpr int PL = 256 / STEM_C4;
    const int grp = blockIdx.y;
    const int cg = threadIdx.x % STEM_C4, pl = threadIdx.x / STEM_C4;
    part += (size_t)grp * gridDim.x * 2 * STEM_C;
    const unsigned per = (n_pix + gridDim.x - 1) / gridDim.x;
    const unsigned pb = blockIdx.x * per, pe = pb + per < n_pix ? pb + per : n_pix;
    const f32x4 sc = scale[grp * STEM_C4 + cg], sf = shift[grp * STEM_C4 + cg];
    const f32x4 mu = mean[grp * STEM_C4 + cg], is = invstd[grp * STEM_C4 + cg];
    const unsigned plane = (unsigned)(H * W);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    for (unsigned m = pb + pl; m < pe; m += PL) {
        const unsigned pix = grp * n_pix + m;
        const unsigned b = pix / plane, r = pix - b * plane;
        const int iy = (int)(r / (unsigned)W), ix = (int)(r - (unsigned)iy * (unsigned)W);
        const unsigned i = pix * STEM_C + cg * 4;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
        const f32x4 g = stem_masked_grad(*reinterpret_cast<const f32x4*>(dy + i), dpooled, idx, xv, sc, sf, (int)b, iy, ix, cg, Ho, Wo);
        if (kStore) *reinterpret_cast<f32x4*>(dy + i) = g;
        s1 += g;
        s2 += g * ((xv - mu) * is);
    }
    sh[0][threadIdx.x] = s1; sh[1][threadIdx.x] = s2;
    __syncthreads();
    if (threadIdx.x < STEM_C4) {
        f32x4 a = sh[0][threadIdx.x], b2 = sh[1][threadIdx.x];
        for (int k = 1; k < PL; ++k) { a += sh[0][threadIdx.x + k * STEM_C4]; b2 += sh[1][threadIdx.x + k * STEM_C4]; }
        float* o = part + (size_t)blockIdx.x * 2 * STEM_C;
        *reinterpret_cast<f32x4*>(o + threadIdx.x * 4) = a;
        *reinterpret_cast<f32x4*>(o + STEM_C + threadIdx.x * 4) = b2;
    }
}

// Pass B: the same gather and mask, then bn_bwd_apply_kernel's formula.
__global__ __launch_bounds__(256) void stem_pool_bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ dpooled,
                                                                     const uint8_t* __restrict__ idx, const float* __restrict__ x,
                                                                     const f32x4* __restrict__ scale, const f32x4* __restrict__ shift,
                                                                     const f32x4* __restrict__ gamma, const f32x4* __restrict__ mean,
                                                                     const f32x4* __restrict__ invstd, const f32x4* __restrict__ sums, int H, int W, int Ho,
                                                                     int Wo, unsigned n_pix /* all groups */, unsigned pix_per_group, float inv_count,
                                                                     float* __restrict__ dx) {
    constexpr int C4 = STEM_C4;
    const unsigned plane = (unsigned)(H * W);
    const size_t n4 = (size_t)n_pix * C4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        const unsigned pix = (unsigned)(i / C4);
        const int grp = (int)(pix / pix_per_group);
        const unsigned b = pix / plane, r = pix - b * plane;
        const int iy = (int)(r / (unsigned)W), ix = (int)(r - (unsigned)iy * (unsigned)W);
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i * 4);
        const f32x4 g = stem_masked_grad(*reinterpret_cast<const f32x4*>(dy + i * 4), dpooled, idx, xv, scale[grp * C4 + c], shift[grp * C4 + c],
                                         (int)b, iy, ix, c, Ho, Wo);
        const f32x4 is = invstd[grp * C4 + c];
        const f32x4 xh = (xv - mean[grp * C4 + c]) * is;
        const f32x4* sg = sums + (size_t)grp * 2 * C4;
        *reinterpret_cast<f32x4*>(dx + i * 4) = (gamma[c] * is) * (g - sg[c] * inv_count - xh * (sg[C4 + c] * inv_count));
    }
}

inline bool stem_shape_ok(int B, int H, int W, int C, int groups) {
    // (32-bit pixel and byte-offset arithmetic in the kernels: the whole map stays under 2^31 bytes)
    return B > 0 && H > 0 && W > 0 && C == STEM_C && groups >= 1 && B % groups == 0 && (size_t)B * H * W * STEM_C * sizeof(float) < ((size_t)1 << 31);
}

}  // namespace mcav

using namespace mcav;

MCAV_EXPORT int mcav_stem_bn_relu_pool_fwd(const float* x, const float* scale, const float* shift, int B, int H, int W, int C, int groups, float* y,
                                           float* pooled, uint8_t* idx, void* stream) {
    if (groups < 1) groups = 1;
    if (!x || !scale || !shift || !y || !pooled || !idx || !stem_shape_ok(B, H, W, C, groups)) return MCAV_E_INVALID;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int tiles_y = (Ho + STEM_TILE - 1) / STEM_TILE, tiles_x = (Wo + STEM_TILE - 1) / STEM_TILE;
    stem_bn_relu_pool_fwd_kernel<<<B * tiles_y * tiles_x, 256, 0, as_stream(stream)>>>(x, (const f32x4*)scale, (const f32x4*)shift, H, W, Ho, Wo, tiles_y,
                                                                                      tiles_x, B / groups, y, pooled, idx);
    return launch_status();
}

MCAV_EXPORT int mcav_stem_pool_bn_bwd_reduce(float* dy, const float* dpooled, const uint8_t* idx, const float* x, const float* scale, const float* shift,
                                             const float* save_mean, const float* save_invstd, int B, int H, int W, int C, int groups, int store_dz,
                                             float* dgamma, float* dbeta, int accumulate, float* sums, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    if (groups < 1) groups = 1;
    if (!dy || !dpooled || !idx || !x || !scale || !shift || !save_mean || !save_invstd || !sums || !workspace || !stem_shape_ok(B, H, W, C, groups))
        return MCAV_E_INVALID;
    const size_t pg = (size_t)(B / groups) * H * W;
    if (workspace_bytes < mcav_bn_bwd_workspace_bytes(pg * groups, C, groups)) return MCAV_E_WORKSPACE;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int blocks = (int)((pg + 31) / 32 < (size_t)STEM_RED_BLOCKS ? (pg + 31) / 32 : (size_t)STEM_RED_BLOCKS);
    float* part = reinterpret_cast<float*>(workspace);
    hipStream_t s = as_stream(stream);
    if (store_dz)
        stem_pool_bn_bwd_reduce_kernel<true><<<dim3(blocks, groups), 256, 0, s>>>(dy, dpooled, idx, x, (const f32x4*)scale, (const f32x4*)shift,
                                                                                 (const f32x4*)save_mean, (const f32x4*)save_invstd, H, W, Ho, Wo,
                                                                                 (unsigned)pg, part);
    else
        stem_pool_bn_bwd_reduce_kernel<false><<<dim3(blocks, groups), 256, 0, s>>>(dy, dpooled, idx, x, (const f32x4*)scale, (const f32x4*)shift,
                                                                                  (const f32x4*)save_mean, (const f32x4*)save_invstd, H, W, Ho, Wo,
                                                                                  (unsigned)pg, part);
    if (launch_status() != MCAV_OK) return MCAV_E_LAUNCH;
    return mcav_bn_bwd_finalize(part, blocks, C, dgamma, dbeta, accumulate, sums, groups, stream);
}

MCAV_EXPORT int mcav_stem_pool_bn_bwd_apply(const float* dy, const float* dpooled, const uint8_t* idx, const float* x, const float* scale,
                                            const float* shift, const float* gamma, const float* save_mean, const float* save_invstd, const float* sums,
                                            int B, int H, int W, int C, int groups, float* dx, void* stream) {
    if (groups < 1) groups = 1;
    if (!dy || !dpooled || !idx || !x || !scale || !shift || !gamma || !save_mean || !save_invstd || !sums || !dx || !stem_shape_ok(B, H, W, C, groups))
        return MCAV_E_INVALID;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const size_t n_pix = (size_t)B * H * W, pg = n_pix / groups;
    const size_t n4 = n_pix * STEM_C4;
    const size_t nb = (n4 + 255) / 256;
    stem_pool_bn_bwd_apply_kernel<<<(int)(nb < 4096 ? nb : 4096), 256, 0, as_stream(stream)>>>(
        dy, dpooled, idx, x, (const f32x4*)scale, (const f32x4*)shift, (const f32x4*)gamma, (const f32x4*)save_mean, (const f32x4*)save_invstd,
        (const f32x4*)sums, H, W, Ho, Wo, (unsigned)n_pix, (unsigned)pg, (float)(1.0 / (double)pg), dx);
    return launch_status();
}
