// monodepth2's training-time augmentation on the GPU (include/mcav_depth.h: mcav_image_preprocess_augment): the Pillow-exact resize of
// preprocess.hip, a per-frame horizontal flip and torchvision's ColorJitter as Pillow computes it, bit-exact (tests/augment_ref.py).
//   pass 1  preprocess.hip's horizontal resample pass                       src -> tmp [B][H0][w][3]
//   pass 2  the vertical pass, read mirrored for flipped frames: writes the plain output, keeps the resized bytes and adds up S, the
//           integer sum of L over the frame after the pointwise operations that precede contrast (one 64-bit atomic per workgroup)
//   pass 3  the drawn operations in registers (contrast's grey from S), normalised into the augmented output
// Grid: blockIdx.y is the frame, so a workgroup's sum belongs to one frame.  Integer sums only: outputs do not depend on arrival order.
#include <math.h>

#include "mcav_common.h"
#include "augment_math.h"

namespace mcav {

void pp_launch_horizontal(const uint8_t* src, int B, int H0, int W0, int w, const int* hbounds, const int* hkk, int hksize, uint8_t* tmp,
                          hipStream_t s);                      // preprocess.hip

namespace {

constexpr int AUG_BITS = 32 - 8 - 2;                           // preprocess.hip PP_BITS
constexpr int AUG_TPB = 256;

struct Norm {
    float m0, m1, m2, s0, s1, s2;
};

// The number of operations before contrast when the frame is coloured and its order holds contrast, else -1 (no sum needed).
__device__ __forceinline__ int ops_before_contrast(const mcav_augment_record& r) {
    if (!(r.flags & MCAV_AUG_COLOUR)) return -1;
    for (int k = 0; k < 4; ++k)
        if (r.order[k] == MCAV_AUG_OP_CONTRAST) return k;
    return -1;
}

__device__ __forceinline__ float factor_of(const mcav_augment_record& r, int op) {
    return op == MCAV_AUG_OP_BRIGHTNESS ? r.brightness : (op == MCAV_AUG_OP_CONTRAST ? r.contrast : r.saturation);
}

__device__ __forceinline__ void store_normalised(float* dst, size_t o, size_t plane, int v0, int v1, int v2, const Norm& nm) {
    dst[o] = ((float)v0 / 255.0f - nm.m0) / nm.s0;             // preprocess.hip's arithmetic
    dst[o + plane] = ((float)v1 / 255.0f - nm.m1) / nm.s1;
    dst[o + 2 * plane] = ((float)v2 / 255.0f - nm.m2) / nm.s2;
}

// tmp [B][H0][w][3] -> plain [B][3][h][w], rb [B][h * w] (r, g, b, 0), lsum[b] += L sums.  grid (blocks per frame, B).
__global__ __launch_bounds__(AUG_TPB) void aug_vertical_kernel(const uint8_t* __restrict__ tmp, int H0, int w, int h,
                                                               const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                               const mcav_augment_record* __restrict__ records, Norm nm,
                                                               float* __restrict__ plain, uchar4* __restrict__ rb,
                                                               unsigned long long* __restrict__ lsum) {
    const int b = blockIdx.y;
    const mcav_augment_record r = records[b];
    const bool flip = (r.flags & MCAV_AUG_FLIP) != 0;
    const int npre = ops_before_contrast(r);                   // uniform over the workgroup
    const int n = h * w;
    const size_t plane = (size_t)n;
    unsigned local = 0;
    for (int i = blockIdx.x * AUG_TPB + threadIdx.x; i < n; i += gridDim.x * AUG_TPB) {
        const int x = i % w, yy = i / w;
        const int xs = flip ? w - 1 - x : x;
        const int ymin = bounds[2 * yy], ymax = bounds[2 * yy + 1];
        const int* k = kk + (size_t)yy * ksize;
        const uint8_t* s = tmp + (((size_t)b * H0 + ymin) * w + xs) * 3;
        int a0 = 1 << (AUG_BITS - 1), a1 = a0, a2 = a0;
        for (int y = 0; y < ymax; ++y) {
            const int kv = k[y];
            const uint8_t* q = s + (size_t)y * w * 3;
            a0 += (int)q[0] * kv; a1 += (int)q[1] * kv; a2 += (int)q[2] * kv;
        }
        const int v0 = min(max(a0 >> AUG_BITS, 0), 255), v1 = min(max(a1 >> AUG_BITS, 0), 255), v2 = min(max(a2 >> AUG_BITS, 0), 255);
        store_normalised(plain, (size_t)b * 3 * plane + i, plane, v0, v1, v2, nm);
        rb[(size_t)b * n + i] = make_uchar4((unsigned char)v0, (unsigned char)v1, (unsigned char)v2, 0);
        if (npre >= 0) {
            int cr = v0, cg = v1, cb = v2;
            for (int j = 0; j < npre; ++j) {
                const int op = r.order[j];
                au::pointwise(op, factor_of(r, op), r.hue_shift & 255, cr, cg, cb);
            }
            local += (unsigned)au::luma(cr, cg, cb);
        }
    }
    if (npre < 0) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off, 64);
    __shared__ unsigned part[AUG_TPB / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int i = 0; i < AUG_TPB / 64; ++i) t += part[i];
        atomicAdd(lsum + b, t);
    }
}

// rb -> aug [B][3][h][w]: the frame's operations in order.  grid (blocks per frame, B).
__global__ __launch_bounds__(AUG_TPB) void aug_apply_kernel(const uchar4* __restrict__ rb, int h, int w,
                                                            const mcav_augment_record* __restrict__ records,
                                                            const unsigned long long* __restrict__ lsum, Norm nm, float* __restrict__ aug) {
    const int b = blockIdx.y;
    const mcav_augment_record r = records[b];
    const bool colour = (r.flags & MCAV_AUG_COLOUR) != 0;
    const int n = h * w;
    const size_t plane = (size_t)n;
    const int mean = ops_before_contrast(r) >= 0 ? au::contrast_mean(lsum[b], (uint64_t)n) : 0;
    for (int i = blockIdx.x * AUG_TPB + threadIdx.x; i < n; i += gridDim.x * AUG_TPB) {
        const uchar4 p = rb[(size_t)b * n + i];
        int cr = p.x, cg = p.y, cb = p.z;
        if (colour) {
            for (int j = 0; j < 4; ++j) {
                const int op = r.order[j];
                if (op == MCAV_AUG_OP_CONTRAST) au::contrast(mean, r.contrast, cr, cg, cb);
                else au::pointwise(op, factor_of(r, op), r.hue_shift & 255, cr, cg, cb);
            }
        }
        store_normalised(aug, (size_t)b * 3 * plane + i, plane, cr, cg, cb, nm);
    }
}

struct Layout {
    size_t tmp, rb, lsum, total;
};

Layout layout(int B, int H0, int h, int w) {
    Layout l;
    l.tmp = 0;
    l.rb = align_up((size_t)B * H0 * w * 3, 256);
    l.lsum = l.rb + align_up((size_t)B * h * w * 4, 256);
    l.total = l.lsum + align_up((size_t)B * 8, 256);
    return l;
}

}  // namespace
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_image_augment_workspace_bytes(int B, int H0, int h, int w) {
    return (B > 0 && H0 > 0 && h > 0 && w > 0) ? layout(B, H0, h, w).total : 0;
}

MCAV_EXPORT int mcav_image_preprocess_augment(const uint8_t* src, int B, int H0, int W0, int h, int w, const int* hbounds, const int* hkk,
                                              int hksize, const int* vbounds, const int* vkk, int vksize, const float* mean3,
                                              const float* std3, const mcav_augment_record* records, float* plain, float* aug,
                                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!src || !plain || !aug || !records || !hbounds || !hkk || !vbounds || !vkk || !mean3 || !std3 || !workspace || B <= 0 || B > 65535 ||
        H0 <= 0 || W0 <= 0 || h <= 0 || w <= 0 || hksize <= 0 || vksize <= 0 || (size_t)h * w > (size_t)INT32_MAX)
        return MCAV_E_INVALID;
    const Layout l = layout(B, H0, h, w);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    hipStream_t s = as_stream(stream);
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    uint8_t* tmp = ws + l.tmp;
    uchar4* rb = reinterpret_cast<uchar4*>(ws + l.rb);
    unsigned long long* lsum = reinterpret_cast<unsigned long long*>(ws + l.lsum);
    const Norm nm{mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]};
    const int n = h * w;
    const int gx = (n + 4 * AUG_TPB - 1) / (4 * AUG_TPB);     // ~4 pixels per thread: one atomic per 1024 pixels
    if (hipMemsetAsync(lsum, 0, (size_t)B * 8, s) != hipSuccess) return MCAV_E_LAUNCH;
    pp_launch_horizontal(src, B, H0, W0, w, hbounds, hkk, hksize, tmp, s);
    aug_vertical_kernel<<<dim3(gx, B), AUG_TPB, 0, s>>>(tmp, H0, w, h, vbounds, vkk, vksize, records, nm, plain, rb, lsum);
    aug_apply_kernel<<<dim3(gx, B), AUG_TPB, 0, s>>>(rb, h, w, records, lsum, nm, aug);
    return launch_status();
}
