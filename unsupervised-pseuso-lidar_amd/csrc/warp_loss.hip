// Loss stage of the training step on gfx950: fused inverse-warp -> bilinear sample -> L1 photometric ->
// second-order smoothness, forward and backward in one pass (K10 + K11), plus the standalone geometry
// entry points (inverse_warp, reconstruct, project, disp_to_depth, SSIM).
//
// HBM-bound streaming/gather work (52 B/pixel compulsory for the fused kernel): one thread per
// target pixel, 32x8 pixel tiles so that a wavefront covers two 32-pixel row segments (128-B coalesced plane
// reads), the tgt-depth tile (+2 halo) staged in LDS for the smoothness stencil, bilinear taps served from
// L1/L2 (neighbouring pixels sample neighbouring source texels), deterministic two-level reduction
// (wavefront shuffles -> LDS -> per-block slab -> fp64 finalize) for the 2 loss scalars and the 3x12 dP sums.
#include <stdlib.h>
#include <mutex>
#include <type_traits>
#include <vector>

#include "block_ops.h"
#include "kernel_timer.h"
#include "warp_math.h"

namespace mcav {

constexpr int TW = 32, TH = 8, HALO = 2, LW = TW + 2 * HALO, LH = TH + 2 * HALO;
constexpr int WL_SUB = 4, WLH = TH * WL_SUB, WL_LH = WLH + 2 * HALO;      // the fused loss kernel: 32 x 32 pixel tiles, 4 pixels per thread --
                                                                          // the 38-value block reduction is paid once per 4 pixels
constexpr int NACC = 38;        // loss_mam, loss_smooth, 3 x dP[12]
constexpr int SLAB = 40;        // floats per block in the slab (padded)

struct PrepConst {
    float Kf[9];
    SampleConst sc;
};

struct WLArgs {
    const float *tgt, *ref0, *ref1, *disp_t, *disp_r0, *poses;
    const void* K;                 // [B,3,3] fp64 (MCAV_WL_K_F64) or fp32
    const float* upstream;         // 2 floats on the device, or nullptr = (1, 1)
    float *d_disp_t, *d_disp_r0, *d_poses, *losses;
    float* slab;                   // [B][nblk][SLAB] per-workgroup partial sums
    double* sample_loss;           // [B][2]
    unsigned* tickets;             // [B + 1], zero between launches: workgroups done per sample; samples done
    int B, H, W;
    int G0, G1;                    // L1 kernel: workgroups per sample of pass 0 (warps 0, 1 + smoothness) / pass 1 (warp 2)
    unsigned flags;
    float tw[3];
    union {              // (one slot: the kernel argument block of the plain instantiations keeps its size and layout)
        float* dbg;          // test-only instantiation (mcav_warp_loss_debug_taps): [B][3 warps][WL_DBG planes][H][W]
        unsigned char* sel;  // masked modes (mcav_warp_loss_masked_fwd_bwd): [B][2][H][W] selection map, or nullptr
    };
};
constexpr int WL_DBG = 7;      // ix, iy, d loss / d ix, d loss / d iy, res[0..2]

// Masked modes: the kernels' MODE template argument (0 = the plain per-warp means).  Selection codes as in include/mcav_depth.h.
constexpr unsigned WL_M_MIN = 1u, WL_M_AUTO = 2u;
constexpr unsigned char SEL_IDENTITY = 2;

// Mono + stereo (mcav_warp_loss_stereo_fwd_bwd): a fourth warp, "s", maps the stereo frame into the target with depth(tgt), the same K and
// the fixed transform [I | (-b, 0, 0)].  It joins pass 0 beside warps 0 and 1 and has no pose gradient.  The stereo kernels are their own
// instantiations of the same bodies (MODE | WL_M_STEREO) with their own argument block: WLArgs and the kernels that take it are unchanged.
constexpr unsigned WL_M_STEREO = 4u;
constexpr unsigned char SEL_STEREO = 3;

struct WLStereoArgs : WLArgs {
    const float* stereo;           // [B,3,H,W]
    const float* baseline;         // [B] on the device: x of the stereo camera's centre in the target camera's frame (metres)
    float tws;                     // the stereo warp's term weight
};
// the stereo fields of an argument block (zero / null for WLArgs: the kernel bodies name them in code that only the stereo kernels instantiate)
template <class A> __device__ __forceinline__ const float* stereo_frame(const A& a) {
    if constexpr (std::is_same<A, WLStereoArgs>::value) return a.stereo; else return nullptr;
}
template <class A> __device__ __forceinline__ float stereo_weight(const A& a) {
    if constexpr (std::is_same<A, WLStereoArgs>::value) return a.tws; else return 0.f;
}

__device__ __forceinline__ void load_K(const void* K, bool f64, int b, double* Kd) {
    if (f64) {
        const double* p = reinterpret_cast<const double*>(K) + (size_t)b * 9;
        for (int i = 0; i < 9; ++i) Kd[i] = p[i];
    } else {
        const float* p = reinterpret_cast<const float*>(K) + (size_t)b * 9;
        for (int i = 0; i < 9; ++i) Kd[i] = (double)p[i];
    }
}

// mode 0: triplet (poses [B,2,6] -> w0 = pose0, w1 = pose1, w2 = inverse(pose0))
// mode 1: single pose [B,6] with `inv`  -> w0
// mode 2: explicit Tcw [B,4,4]          -> w0
// mode 3: intrinsics only (Kinv)
__global__ void pose_prepare_kernel(const float* poses, const void* K, const float* Tcw, int B, int mode, int inv,
                                    int k_f64, PrepConst* out, float* ones) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0 && ones) { ones[0] = 1.0f; ones[1] = 1.0f; reinterpret_cast<unsigned*>(ones)[2] = 0u; }      // [2]: the finalize kernel's ticket
    if (b >= B) return;
    double Kd[9], Ki[9];
    load_K(K, k_f64 != 0, b, Kd);
    invert3x3(Kd, Ki);
    PrepConst pc;
    for (int i = 0; i < 9; ++i) { pc.Kf[i] = (float)Kd[i]; pc.sc.Kinv[i] = (float)Ki[i]; }
    float R[9], t[3];
    if (mode == 0) {
        const float* p = poses + (size_t)b * 12;
        pose_to_Rt(p, false, R, t);      make_P(pc.Kf, R, t, pc.sc.w[0].P);
        pose_to_Rt(p + 6, false, R, t);  make_P(pc.Kf, R, t, pc.sc.w[1].P);
        pose_to_Rt(p, true, R, t);       make_P(pc.Kf, R, t, pc.sc.w[2].P);
    } else if (mode == 1) {
        pose_to_Rt(poses + (size_t)b * 6, inv != 0, R, t);
        make_P(pc.Kf, R, t, pc.sc.w[0].P);
        for (int i = 0; i < 12; ++i) { pc.sc.w[1].P[i] = 0.f; pc.sc.w[2].P[i] = 0.f; }
    } else if (mode == 2) {
        const float* T = Tcw + (size_t)b * 16;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) R[i * 3 + j] = T[i * 4 + j];
            t[i] = T[i * 4 + 3];
        }
        make_P(pc.Kf, R, t, pc.sc.w[0].P);
        for (int i = 0; i < 12; ++i) { pc.sc.w[1].P[i] = 0.f; pc.sc.w[2].P[i] = 0.f; }
    } else {   // mode 3: intrinsics only
        for (int w = 0; w < 3; ++w)
            for (int i = 0; i < 12; ++i) pc.sc.w[w].P[i] = 0.f;
    }
    out[b] = pc;
}

__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// Reduce N per-thread floats over a 256-thread block and store them at dst[0..N).
template <int N, bool AGENT = false>
__device__ __forceinline__ void block_reduce_store(float* acc, float* dst, float (*sred)[SLAB]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {                          // one exec-masked region for the N stores (not one per value)
#pragma unroll
        for (int k = 0; k < N; ++k) sred[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const float v = (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
        if constexpr (AGENT) __hip_atomic_store(dst + threadIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else dst[threadIdx.x] = v;
    }
}

// Branch-free bilinear gathers: an image (3 planes) is a raw buffer resource, a tap outside the image carries an out-of-range offset and
// reads as zero in hardware.  No exec-mask branch and no value merge sits between a load and its use, so the 36 gathers of a pixel's three
// warps are issued back to back behind one counted wait (the predicated form compiled to ~90 exec-masked regions, each with its own wait).
constexpr unsigned WL_OOB = 0x80000000u;

// (the base is wave-uniform by construction; said explicitly, because a 64-bit sample offset formed on the vector ALU made the compiler
//  treat the descriptor as divergent and wrap every gather in a waterfall loop)
__device__ __forceinline__ const float* uniform_ptr(const float* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t image_rsrc(const float* img, size_t plane) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(uniform_ptr(img)), 0, (unsigned)(3 * plane * sizeof(float)), 0x00020000);
}

struct TapOff { unsigned o[4]; };

__device__ __forceinline__ TapOff tap_offsets(const Tap& t, int W) {
    const int base = (t.y0 * W + t.x0) * 4;
    TapOff f;
    f.o[0] = t.in00 ? (unsigned)base : WL_OOB;
    f.o[1] = t.in01 ? (unsigned)(base + 4) : WL_OOB;
    f.o[2] = t.in10 ? (unsigned)(base + W * 4) : WL_OOB;
    f.o[3] = t.in11 ? (unsigned)(base + W * 4 + 4) : WL_OOB;
    return f;
}

__device__ __forceinline__ void gather_taps(__amdgpu_buffer_rsrc_t rs, const TapOff& f, int plane_bytes, float (*q)[4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) q[c][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)f.o[k], c * plane_bytes, 0));
}

// ---------------------------------------------------------------------------------------------- one launch: prologue and epilogue of the fused kernels
// Round 3 folds the two helper launches into the fused kernels (they were 13 of the loss stage's 83 us):
//   * prologue: every workgroup derives its sample's constants itself (lanes 0..2: Rodrigues, P = K [R|t], Q = P[:, :3] K^-1 for one warp each;
//     float64 inverse of K) into LDS, and every wavefront lifts them into scalar registers;
//   * epilogue: per-workgroup partial sums go to the slab; a per-sample ticket names the LAST workgroup of a sample, which sums that sample's
//     slab entries in float64 (fixed order: bit-reproducible), turns dP into the pose gradients and emits the sample's loss sums; a second
//     ticket names the last SAMPLE, which adds the samples up in index order.  Tickets are left at zero for the next launch.
struct alignas(16) SampleFast {
    WarpFast w[3];       // 12 floats each
    float Kinv[12];      // 9 used
};
struct alignas(16) SampleFastStereo {
    WarpFast w[4];       // w[3]: the stereo warp
    float Kinv[12];
};
template <unsigned MODE> using SampleFastOf = std::conditional_t<(MODE & WL_M_STEREO) != 0, SampleFastStereo, SampleFast>;

// Twelve wave-uniform floats from LDS as three 16-byte broadcast reads, NOT hoisted out of the pixel loop (volatile): held in registers for
// the whole loop the three warps' constants cost 45 registers -- as scalars they overflowed the scalar file and the buffer resources with them.
struct F12 { float v[12]; };
__device__ __forceinline__ F12 lds12(const float* p) {
    using f4 = __attribute__((ext_vector_type(4))) float;
    // LDS byte address of p (the low 32 bits of a generic pointer into LDS are its LDS offset); ds_read_b128 through inline asm keeps the
    // loads where they are written -- three per use, nothing held across the loop
    const unsigned addr = (unsigned)reinterpret_cast<unsigned long long>(p);
    F12 r;
    f4 t0, t1, t2;
    asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %3 offset:16\n\tds_read_b128 %2, %3 offset:32\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(t0), "=&v"(t1), "=&v"(t2) : "v"(addr) : "memory");
    r.v[0] = t0.x; r.v[1] = t0.y; r.v[2] = t0.z; r.v[3] = t0.w;
    r.v[4] = t1.x; r.v[5] = t1.y; r.v[6] = t1.z; r.v[7] = t1.w;
    r.v[8] = t2.x; r.v[9] = t2.y; r.v[10] = t2.z; r.v[11] = t2.w;
    return r;
}
__device__ __forceinline__ WarpFast lds_warp(const WarpFast& w) {
    const F12 r = lds12(w.Q);
    WarpFast u;
#pragma unroll
    for (int i = 0; i < 9; ++i) u.Q[i] = r.v[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) u.p3[i] = r.v[9 + i];
    return u;
}

template <class A, class SF>
__device__ __forceinline__ void block_prepare(const A& a, int b, SF* sf) {
    constexpr bool ST = std::is_same<SF, SampleFastStereo>::value;
    if (threadIdx.x < (ST ? 4 : 3)) {
        const int w = threadIdx.x;
        double Kd[9], Ki[9];
        load_K(a.K, (a.flags & MCAV_WL_K_F64) != 0, b, Kd);
        invert3x3(Kd, Ki);
        float Kf[9], Kinv[9], R[9], t[3], P[12];
        for (int i = 0; i < 9; ++i) { Kf[i] = (float)Kd[i]; Kinv[i] = (float)Ki[i]; }
        if constexpr (ST) {
            if (w == 3) {                                        // the stereo warp: R = I exactly, t = (-b, 0, 0), b read on the device
                for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
                t[0] = -a.baseline[b]; t[1] = 0.0f; t[2] = 0.0f;
            } else {
                pose_to_Rt(a.poses + (size_t)b * 12 + (w == 1 ? 6 : 0), w == 2, R, t);
            }
        } else {
            pose_to_Rt(a.poses + (size_t)b * 12 + (w == 1 ? 6 : 0), w == 2, R, t);
        }
        make_P(Kf, R, t, P);
        make_fast(P, Kinv, sf->w[w]);
        if (w == 0)
            for (int i = 0; i < 9; ++i) sf->Kinv[i] = Kinv[i];
    }
    __syncthreads();
}

__device__ __forceinline__ float uniform_of(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ WarpFast uniform_warp(const WarpFast& w) {
    WarpFast u;
#pragma unroll
    for (int i = 0; i < 9; ++i) u.Q[i] = uniform_of(w.Q[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) u.p3[i] = uniform_of(w.p3[i]);
    return u;
}

// What one workgroup writes for ANOTHER to read inside the same launch (slab entries, per-sample sums) follows the hand-off protocol of
// mcav_common.h: agent-scope (sc1) stores, an explicit s_waitcnt vmcnt(0) in every thread before the ticket, sc1 loads in the finisher.  The
// first version used __threadfence(), i.e. a write-back and invalidate of the XCD's whole L2 per workgroup: 660 (L1) / 3840 (SSIM) of those per
// launch took the gathers' cached lines with them and doubled the kernels' time.

constexpr int RED_LD = 256 + 8;      // one pad float per 32 threads: the transposed reads are conflict-free

// Sum N per-thread values over the 256 threads (fixed order) into out[slot(k)]: each value's 256 addends are written to LDS, 8 lanes
// take 32 of them each, three xor-shuffles finish.  ~N + 50 instructions per thread instead of 12 N for N wavefront butterflies.
template <int N, class Slot>
__device__ __forceinline__ void block_sum_to_slab(const float* acc, float (*sred)[RED_LD], float* out, Slot slot) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) sred[k][tid + (tid >> 5)] = acc[k];
    __syncthreads();
    const int k = tid >> 3, part = tid & 7;
    float s = 0.f;
    if (k < N) {
#pragma unroll
        for (int j = 0; j < 32; ++j) s += sred[k][part * 33 + j];
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (k < N && part == 0) handoff_store(out + slot(k), s);
}

// after the workgroup's slab entry is written: ticket, and the last workgroup of the sample finishes the sample
__device__ __forceinline__ void block_finish(const WLArgs& a, int b, int nblk, double (*s64)[SLAB], int* s_flag) {
    const int tid = threadIdx.x;
    if (!handoff_last([&] { return &a.tickets[b]; }, nblk, s_flag)) return;
    const float* slab = a.slab + (size_t)b * nblk * SLAB;
    constexpr int PARTS = 256 / SLAB;                            // 6 x 40 = 240 threads
    if (tid < PARTS * SLAB) {
        const int part = tid / SLAB, k = tid - part * SLAB;
        double sum = 0.0;
        for (int blk = part; blk < nblk; blk += PARTS)
            sum += (double)handoff_load(slab + (size_t)blk * SLAB + k);      // written by other workgroups
        s64[part][k] = sum;
    }
    __syncthreads();
    if (tid < SLAB) {
        double t = 0.0;
#pragma unroll
        for (int p = 0; p < PARTS; ++p) t += s64[p][tid];
        s64[0][tid] = t;
    }
    __syncthreads();
    if (tid < 3) {                                               // one warp's pose gradient per lane
        double Kd[9];
        load_K(a.K, (a.flags & MCAV_WL_K_F64) != 0, b, Kd);
        float Kf[9];
        for (int i = 0; i < 9; ++i) Kf[i] = (float)Kd[i];
        double g[6];
        pose_grad_from_dP(&s64[0][2 + 12 * tid], Kf, a.poses + (size_t)b * 12 + (tid == 1 ? 6 : 0), tid == 2, g);
        for (int i = 0; i < 6; ++i) s64[1 + tid][i] = g[i];
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 0; i < 6; ++i) {
            a.d_poses[(size_t)b * 12 + i] = (float)(s64[1][i] + s64[3][i]);      // pose[0]: warp 0 and (through its inverse) warp 2
            a.d_poses[(size_t)b * 12 + 6 + i] = (float)s64[2][i];
        }
        handoff_store(a.sample_loss + b * 2 + 0, s64[0][0]);
        handoff_store(a.sample_loss + b * 2 + 1, s64[0][1]);
        handoff_store(&a.tickets[b], 0u);
        handoff_release();
        if (handoff_ticket(&a.tickets[a.B]) == (unsigned)(a.B - 1)) {
            double l0 = 0.0, l1 = 0.0;
            for (int i = 0; i < a.B; ++i) {
                l0 += handoff_load(a.sample_loss + i * 2);
                l1 += handoff_load(a.sample_loss + i * 2 + 1);
            }
            a.losses[0] = (float)l0;
            a.losses[1] = (float)l1;
            handoff_store(&a.tickets[a.B], 0u);
        }
    }
}

// ---------------------------------------------------------------------------------------------- fused warp + L1 + smoothness (round 3)
// The kernel is bound by instruction issue, not by HBM (52 B/pixel against ~1100 vector instructions per pixel in round 2).  What changed:
//   * the per-pixel arithmetic (csrc/warp_math.h, "lean forms"): affine q, reciprocals, nested lerp -- about 500 instructions per pixel;
//   * ONE warp at a time: a workgroup of pass 0 runs warps 0 and 1 (both use depth(tgt) and the target's pixels) and the smoothness term,
//     a workgroup of pass 1 runs warp 2 (depth(ref0)): 26 / 13 running sums instead of 38, <= 128 registers, four wavefronts per SIMD;
//   * the 12 gathers of a warp are issued one unit AHEAD of their use (two register sets: pass 0 alternates the two warps of a pixel,
//     pass 1 the two pixels a thread owns in a tile), the target-aligned values one pixel ahead of that;
//   * a workgroup walks tiles g, g + G, ... of one sample (32 x 16 pixels, two per thread) and reduces its sums ONCE, through LDS;
//   * no helper launches (see above).
constexpr int T2H = 16, T2LH = T2H + 2 * HALO;
constexpr int RED_N0 = 26, RED_N1 = 13;
constexpr int WL_STAGE = 16;      // pixels per thread between two flushes of the staged disparity gradients (see the kernel)

// MODE (masked modes, include/mcav_depth.h): pass 0 holds warp 0's tap and derivative sums until warp 1's error and the identity errors
// (ref0 / ref1 read at the pixel: coalesced, and mostly in cache behind the gathers) are known, then chains only the selected warp's
// gradient; pass 1 does the same for warp 2 against its identity error.  The selection of a pixel's stage is staged in LDS next to the
// disparity gradient and written with it.  MODE 0 is the plain kernel: none of the masked code is instantiated in it.  The automask modes
// carry the identity values in flight as well: at three workgroups per CU (168 VGPRs) they spilled, so they run at two, without scratch.
template <bool DBG, unsigned MODE = 0>
__global__ __launch_bounds__(256, (MODE & WL_M_AUTO) ? 2 : 3) void warp_loss_l1_kernel(WLArgs a) {
#include "warp_loss_l1_body.h"
}

// Stereo: pass 0 holds a third warp's gathers in flight (12 floats and a tap more than the plain kernel, which already sits at 168 VGPRs
// with three workgroups per CU): every stereo instantiation runs at two per CU, without scratch.
template <unsigned MODE_>
__global__ __launch_bounds__(256, 2) void warp_loss_l1_stereo_kernel(WLStereoArgs a) {
    constexpr bool DBG = false;
    constexpr unsigned MODE = MODE_ | WL_M_STEREO;
#include "warp_loss_l1_body.h"
}

// ---------------------------------------------------------------------------------------------- SSIM + L1 photometric (MCAV_WL_SSIM)
// The north_star's photometric mix, 0.85 * SSIM distance + 0.15 * L1 (weights of losses.py:77, SSIM of losses.py:12-54), fused with
// the warp, forward and backward in one pass.  Per 32 x 32 tile and per warp the three warped channel planes and the three target
// planes of the tile + 2 halo are staged in LDS (values at padded positions -1 / H / W are the warp at the REFLECTED pixel, which is
// what ReflectionPad2d of the warped image holds); per channel the 3x3 window statistics are evaluated on tile + 1 halo and turned
// into three coefficient fields -- dS(p)/dx(q) = a(p) + b(p) x(q) + c(p) y(q) for every q in p's window -- so that the gradient at a
// pixel is a second 3x3 gather of (a, b, c) (plus the windows it enters through the reflection), no atomics.
constexpr int SS_P = WLH + 2;      // statistics region: tile + 1 halo

struct SsimPoint { float S, a, b, c; };

// x: 3x3 window of the warped image, y: of the target, row-major.  S = clamp((1 - SSIM) / 2, 0, 1); (a, b, c): see above.
__device__ __forceinline__ SsimPoint ssim_point(const float* x, const float* y) {
    // no fma contraction: SSIM(x, x) must cancel exactly, as in ssim_kernel and in the reference
#pragma clang fp contract(off)
    float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) { sx += x[i]; sy += y[i]; sxx += x[i] * x[i]; syy += y[i] * y[i]; sxy += x[i] * y[i]; }
    const float C1 = 1e-4f, C2 = 9e-4f, k = 1.0f / 9.0f;
    const float mx = sx * k, my = sy * k;
    const float mxy = mx * my, mxx = mx * mx, myy = my * my;
    const float vx = sxx * k - mxx, vy = syy * k - myy, vxy = sxy * k - mxy;
    const float A1 = 2.f * mxy + C1, A2 = 2.f * vxy + C2, B1 = mxx + myy + C1, B2 = vx + vy + C2;
    const float den = B1 * B2;
    const float ssim = (A1 * A2) / den;
    const float v = (1.0f - ssim) / 2.0f;
    SsimPoint o;
    o.S = fminf(fmaxf(v, 0.0f), 1.0f);
    const float m = (v >= 0.0f && v <= 1.0f) ? -0.5f * (2.0f / 9.0f) / den : 0.0f;       // d clamp((1 - ssim) / 2) / d ssim, times 2 / (9 den)
    o.a = m * (my * (A2 - A1) - ssim * mx * (B2 - B1));
    o.b = m * (-ssim * B1);
    o.c = m * A1;
    return o;
}

// Masked modes (MODE != 0).  A pixel's error needs its 3x3 window, so every candidate's error on tile + 1 halo is known before any warp's
// backward: per GROUP of warps (min-reprojection: {0, 1} and {2}; automask alone: {0}, {1}, {2}) the candidates -- identities first, then the
// reprojections, in tie order -- are staged one at a time into sX (the identity's tile is the unwarped source with its reflected halo) and
// their per-pixel errors (channel sums of 0.85 S + 0.15 |x - t|) folded into a running minimum.  The thread that evaluates a statistics pixel
// keeps that pixel's choice in a register (phase 2 of the backward gives it the same pixels), so only the tile's own codes go to LDS (sM,
// 1 KB: the L1 part of the gradient and the selection map).  Then each warp of the group runs phases 2-4 with its coefficient fields and
// its L1 term multiplied by the selection.  The group's last candidate is still in sX for the first backward; min-reprojection re-stages
// warp 0 once.  Chosen over keeping both warped tiles in LDS (+16 KB): 53 KB keeps three workgroups per CU, 69 KB would allow two.
constexpr int SS_N = SS_P * SS_P, SS_K = (SS_N + 255) / 256;      // statistics pixels of a tile; per thread

template <bool DBG, unsigned MODE = 0>
__global__ __launch_bounds__(256) void warp_loss_ssim_kernel(WLArgs a) {
#include "warp_loss_ssim_body.h"
}

template <unsigned MODE_>
__global__ __launch_bounds__(256) void warp_loss_ssim_stereo_kernel(WLStereoArgs a) {
    constexpr bool DBG = false;
    constexpr unsigned MODE = MODE_ | WL_M_STEREO;
#include "warp_loss_ssim_body.h"
}

// ---------------------------------------------------------------------------------------------- standalone warp
__global__ __launch_bounds__(256) void inverse_warp_fwd_kernel(const float* img, const float* depth, const PrepConst* pcs, int B, int H, int W, float* out) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * TW + (threadIdx.x & 31), y = blockIdx.y * TH + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    const PrepConst& pc = pcs[b];
    const Ray r = pixel_ray(pc.sc.Kinv, (float)x, (float)y);
    const Tap t = project_pixel(pc.sc.w[0].P, r, depth[(size_t)b * plane + pix], H, W);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((size_t)b * 3 + c) * plane + pix] = bilinear(img + ((size_t)b * 3 + c) * plane, W, t).v;
}

__global__ __launch_bounds__(256) void inverse_warp_bwd_kernel(const float* img, const float* depth, const PrepConst* pcs, const float* go,
                                                               int B, int H, int W, float* d_depth, float* slab) {
    __shared__ float sred[4][SLAB];
    const int b = blockIdx.z;
    const int x = blockIdx.x * TW + (threadIdx.x & 31), y = blockIdx.y * TH + (threadIdx.x >> 5);
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    if (x < W && y < H) {
        const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
        const PrepConst& pc = pcs[b];
        const Ray r = pixel_ray(pc.sc.Kinv, (float)x, (float)y);
        const Tap t = project_pixel(pc.sc.w[0].P, r, depth[(size_t)b * plane + pix], H, W);
        float gix = 0.f, giy = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const Sample s = bilinear(img + ((size_t)b * 3 + c) * plane, W, t);
            const float g = go[((size_t)b * 3 + c) * plane + pix];
            gix += g * s.dvdx;
            giy += g * s.dvdy;
        }
        d_depth[(size_t)b * plane + pix] = backproject_grad(pc.sc.w[0].P, r, t, gix, giy, H, W, acc);
    }
    const int nblk = gridDim.x * gridDim.y;
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    block_reduce_store<12>(acc, slab + ((size_t)b * nblk + blk) * SLAB, sred);
}

__global__ __launch_bounds__(64) void inverse_warp_bwd_finalize_kernel(const float* slab, int nblk, const PrepConst* pcs, const float* pose, int inv, float* d_pose) {
    __shared__ double s[4][12];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 48) {
        const int part = tid / 12, k = tid - part * 12;
        double sum = 0.0;
        for (int blk = part; blk < nblk; blk += 4) sum += (double)slab[((size_t)b * nblk + blk) * SLAB + k];
        s[part][k] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        double dP[12], g[6];
        for (int k = 0; k < 12; ++k) dP[k] = (s[0][k] + s[1][k]) + (s[2][k] + s[3][k]);
        pose_grad_from_dP(dP, pcs[b].Kf, pose + (size_t)b * 6, inv != 0, g);
        for (int i = 0; i < 6; ++i) d_pose[(size_t)b * 6 + i] = (float)g[i];
    }
}

__global__ __launch_bounds__(256) void reconstruct_kernel(const float* depth, const PrepConst* pcs, int B, int H, int W, float* pts) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * TW + (threadIdx.x & 31), y = blockIdx.y * TH + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    const Ray r = pixel_ray(pcs[b].sc.Kinv, (float)x, (float)y);
    const float D = depth[(size_t)b * plane + pix];
    pts[((size_t)b * 3 + 0) * plane + pix] = r.r0 * D;
    pts[((size_t)b * 3 + 1) * plane + pix] = r.r1 * D;
    pts[((size_t)b * 3 + 2) * plane + pix] = r.r2 * D;
}

__global__ __launch_bounds__(256) void project_kernel(const float* pts, const void* K, int k_f64, const float* Tcw, int B, int H, int W, float* grid) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * TW + (threadIdx.x & 31), y = blockIdx.y * TH + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    double Kd[9];
    load_K(K, k_f64 != 0, b, Kd);
    float Kf[9], R[9], t[3], P[12];
    for (int i = 0; i < 9; ++i) Kf[i] = (float)Kd[i];
    const float* T = Tcw + (size_t)b * 16;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = T[i * 4 + j];
        t[i] = T[i * 4 + 3];
    }
    make_P(Kf, R, t, P);
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    const float X0 = pts[((size_t)b * 3 + 0) * plane + pix], X1 = pts[((size_t)b * 3 + 1) * plane + pix], X2 = pts[((size_t)b * 3 + 2) * plane + pix];
    const float c0 = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3];
    const float c1 = P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7];
    const float c2 = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11];
    const float z = c2 + 1e-5f;
    grid[((size_t)b * plane + pix) * 2 + 0] = ((c0 / z) / (float)(W - 1) - 0.5f) * 2.0f;
    grid[((size_t)b * plane + pix) * 2 + 1] = ((c1 / z) / (float)(H - 1) - 0.5f) * 2.0f;
}

// The translation of the rigid inverse, t' = -R^T t, with Rodrigues (+1e-7f) in float64 and ONE rounding at the end.  Formed from the
// float32 rotation it inherits that rotation's absolute error (up to 8 u per entry near a half turn) times t, which is larger than t'
// itself wherever a column of R is small; this way every entry is within one rounding of the float64 value.  The standalone entry only:
// the fused kernels keep pose_to_Rt (csrc/warp_math.h), the reference's float32 chain.
__device__ __forceinline__ void inverse_translation_f64(const float* pose, float* t) {
    const double vx = pose[0], vy = pose[1], vz = pose[2];
    const double angle = sqrt(vx * vx + vy * vy + vz * vz);
    const double inv = 1.0 / (angle + (double)1e-7f);
    const double x = vx * inv, y = vy * inv, z = vz * inv;
    const double ca = cos(angle), sa = sin(angle), C = 1.0 - ca;
    const double R0[9] = {x * x * C + ca, x * y * C - z * sa, z * x * C + y * sa,
                          x * y * C + z * sa, y * y * C + ca, y * z * C - x * sa,
                          z * x * C - y * sa, y * z * C + x * sa, z * z * C + ca};
    for (int i = 0; i < 3; ++i)
        t[i] = (float)(-(R0[0 * 3 + i] * (double)pose[3] + R0[1 * 3 + i] * (double)pose[4] + R0[2 * 3 + i] * (double)pose[5]));
}

__global__ void pose_to_matrix_kernel(const float* pose, int B, int invert, float* T) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float R[9], t[3];
    pose_to_Rt(pose + (size_t)b * 6, invert != 0, R, t);
    if (invert) inverse_translation_f64(pose + (size_t)b * 6, t);
    float* o = T + (size_t)b * 16;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = R[i * 3 + j];
        o[i * 4 + 3] = t[i];
    }
    o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
}

__global__ void invert_pose_kernel(const float* T, int B, float* Ti) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* s = T + (size_t)b * 16;
    float* o = Ti + (size_t)b * 16;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = s[j * 4 + i];
        o[i * 4 + 3] = (-1.0f * s[0 * 4 + i]) * s[3] + (-1.0f * s[1 * 4 + i]) * s[7] + (-1.0f * s[2 * 4 + i]) * s[11];
    }
    o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
}

__global__ void disp_to_depth_kernel(const float* disp, float* depth, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        depth[i] = 1.0f / (10.0f * disp[i] + 0.01f);
}

__global__ void disp_to_depth_bwd_kernel(const float* disp, const float* dD, float* dd, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float D = 1.0f / (10.0f * disp[i] + 0.01f);
        dd[i] = dD[i] * (-10.0f * D * D);
    }
}


__global__ __launch_bounds__(256) void ssim_kernel(const float* xs, const float* ys, int N, int H, int W, float C1, float C2, float* out) {
    // no fma contraction in this kernel: SSIM(x, x) must cancel exactly (num == den), as it does in the reference
#pragma clang fp contract(off)
    const int n = blockIdx.z;
    const int x = blockIdx.x * TW + (threadIdx.x & 31), y = blockIdx.y * TH + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const float* px = xs + (size_t)n * H * W;
    const float* py = ys + (size_t)n * H * W;
    float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = reflect1(y + dy, H);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = reflect1(x + dx, W);
            const float a = px[(size_t)yy * W + xx], b = py[(size_t)yy * W + xx];
            sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
        }
    }
    const float k = 1.0f / 9.0f;
    const float mx = sx * k, my = sy * k;
    const float mxy = mx * my, mxx = mx * mx, myy = my * my;
    const float vx = sxx * k - mxx, vy = syy * k - myy, vxy = sxy * k - mxy;
    const float num = (2.f * mxy + C1) * (2.f * vxy + C2);
    const float den = (mxx + myy + C1) * (vx + vy + C2);
    float v = (1.0f - num / den) / 2.0f;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    out[(size_t)n * H * W + (size_t)y * W + x] = v;
}

// ---------------------------------------------------------------------------------------------- smoothness, one scale
__global__ __launch_bounds__(256) void smooth_kernel(const float* depth, int B, int H, int W, float weight, const float* upstream,
                                                     float* d_depth, int accumulate, float* slab) {
    __shared__ float sD[LH][LW + 1];
    __shared__ float sred[4][SLAB];
    const int b = blockIdx.z;
    const int bx0 = blockIdx.x * TW, by0 = blockIdx.y * TH;
    const size_t plane = (size_t)H * W;
    const float* dp = depth + (size_t)b * plane;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = by0 - HALO + ly, gx = bx0 - HALO + lx;
        sD[ly][lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? dp[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x = bx0 + tx, y = by0 + ty;
    float acc[1] = {0.f};
    if (x < W && y < H) {
        const int cy = ty + HALO, cx = tx + HALO;
        const float cxx = weight / (float)((size_t)B * H * (W - 2));
        const float cyy = weight / (float)((size_t)B * (H - 2) * W);
        const float cxy = 2.0f * weight / (float)((size_t)B * (H - 1) * (W - 1));
        auto DD = [&](int dy, int dx) { return sD[cy + dy][cx + dx]; };
        float gs = 0.f, ls = 0.f;
        smooth_terms(DD, x, y, H, W, cxx, cyy, cxy, ls, gs);
        acc[0] = ls;
        // The gradient is a sum of ten signed coefficients, 7 to 8 times the largest in magnitude: in float32 the rounding of weight / n and
        // of nine additions costs up to 19 u of the largest coefficient (measured).  The signs of each group are summed as small integers
        // (exact) and weighted in float64, so the element is rounded once.
        float nx = 0.f, ny = 0.f, nxy = 0.f, unused = 0.f;
        smooth_terms(DD, x, y, H, W, 1.0f, 0.0f, 0.0f, unused, nx);
        smooth_terms(DD, x, y, H, W, 0.0f, 1.0f, 0.0f, unused, ny);
        smooth_terms(DD, x, y, H, W, 0.0f, 0.0f, 1.0f, unused, nxy);
        const double w = (double)weight;
        const double gsd = (double)nx * (w / (double)((size_t)B * H * (W - 2))) + (double)ny * (w / (double)((size_t)B * (H - 2) * W)) +
                           (double)nxy * (2.0 * w / (double)((size_t)B * (H - 1) * (W - 1)));
        const double g = upstream ? (double)upstream[0] : 1.0;
        const size_t o = (size_t)b * plane + (size_t)y * W + x;
        d_depth[o] = (float)((accumulate ? (double)d_depth[o] : 0.0) + g * gsd);
        (void)gs;
    }
    const int nblk = gridDim.x * gridDim.y * gridDim.z;
    const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    (void)nblk;
    block_reduce_store<1>(acc, slab + (size_t)blk * SLAB, sred);
}

__global__ __launch_bounds__(256) void smooth_finalize_kernel(const float* slab, int nblk, float* loss_accum) {
    __shared__ double s[256];
    double sum = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) sum += (double)slab[(size_t)i * SLAB];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_accum[0] += (float)s[0];
}

struct WsLayout {
    size_t pc_off, tick_off, slab_off, sl_off, total;
    int nblk;
};

constexpr int WL_MAX_B = 4095;      // samples per launch of the fused kernels (ticket capacity)

inline WsLayout ws_layout(int B, int H, int W) {
    WsLayout l;
    l.nblk = ((W + TW - 1) / TW) * ((H + TH - 1) / TH);            // workgroups per sample of the standalone kernels (32 x 8 pixel tiles)
    const int cap = ((W + TW - 1) / TW) * 2 * ((H + T2H - 1) / T2H);      // >= the workgroups per sample of the fused kernels
    const int rows = l.nblk > cap ? l.nblk : cap;
    // The tickets sit at a FIXED place and size, whatever (B, H, W): a caller's cached workspace serves launches of different shapes, and a
    // ticket word that another shape's slab had used would not be zero.  Nothing else is ever written to this region.
    size_t o = 0;
    l.tick_off = o; o = align_up(o + sizeof(unsigned) * ((size_t)WL_MAX_B + 1), 256);
    l.pc_off = o;   o = align_up(o + sizeof(PrepConst) * (size_t)B, 256);
    l.slab_off = o; o = align_up(o + sizeof(float) * SLAB * (size_t)B * rows, 256);
    l.sl_off = o;   o = align_up(o + sizeof(double) * 2 * (size_t)B, 256);
    l.total = o;
    return l;
}

// workgroups per sample of the fused L1 kernel: pass 0 (warps 0, 1 + smoothness: ~2.7 units of work per tile) and pass 1 (warp 2: 1 unit), sized
// so that every workgroup of the launch is resident at once (CUs x workgroups per CU, asked of the runtime) and the two kinds take about the
// same time -- a second, partly filled generation would double the launch's duration
template <auto KERNEL>
inline int resident_slots() {
    static int slots = 0;
    if (slots == 0) {
        int dev = 0, cus = 256, per_cu = 3;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, 256, 0) != hipSuccess || per_cu < 1) per_cu = 3;
        (void)hipGetLastError();
        slots = cus * per_cu;
    }
    return slots;
}
template <unsigned MODE> inline int l1_slots() { return resident_slots<warp_loss_l1_kernel<false, MODE>>(); }
template <unsigned MODE> inline int l1_stereo_slots() { return resident_slots<warp_loss_l1_stereo_kernel<MODE>>(); }

// stereo: a pass-0 tile gathers three warps against pass 1's one.  Measured on MI355X (tools/loss_bench.py --stereo, 12 x 192x640, L1 plain /
// min-reprojection + automask): 1.5 -> 86.2 / 97.0 us, 2.0 -> 79.4 / 85.7, 2.7 -> 79.1 / 85.3, 3.4 -> 79.0 / 85.7, 4.0 -> 78.8 / 85.5: flat
// from 2.0 up; 2.7 kept.  MCAV_WL_RATIO_STEREO overrides (experiments).
inline void l1_grid(int B, int H, int W, int slots, int& G0, int& G1, bool stereo = false) {
    const int ntiles = ((W + TW - 1) / TW) * ((H + T2H - 1) / T2H);
    // tiles of a pass-1 workgroup per tile of a pass-0 workgroup.  Counted in instructions a pass-0 tile is 2.7 pass-1 tiles; measured on
    // MI355X (tools/loss_bench.py, network-like disparities, 12 x 192x640 / 12 x 320x1024): 1.0 -> 73.8 / 201 us, 2.0 -> 66.2 / 171, 2.7 -> 69.2 /
    // 172.  MCAV_WL_RATIO overrides (experiments).  Also measured and not kept: the smoothness tile's depths fetched a pixel ahead (68.4 us),
    // a three-stage pipeline with 24 .. 48 gathers in flight at two wavefronts per SIMD (68.6 .. 73 us).
    static const float ratio_mono = [] { const float r = MCAV_KNOB_FLOAT("MCAV_WL_RATIO", 2.0f); return r > 0.05f ? r : 2.0f; }();
    static const float ratio_stereo = [] { const float r = MCAV_KNOB_FLOAT("MCAV_WL_RATIO_STEREO", 2.7f); return r > 0.05f ? r : 2.7f; }();
    const float ratio = stereo ? ratio_stereo : ratio_mono;
    const int per_sample = slots / B > 0 ? slots / B : 1;
    int n0 = (int)((ntiles * (1.0f + 1.0f / ratio) + per_sample - 1) / per_sample);
    if (n0 < 1) n0 = 1;
    for (;; ++n0) {
        int n1 = (int)(ratio * n0 + 0.5f);
        if (n1 < 1) n1 = 1;
        G0 = (ntiles + n0 - 1) / n0;
        G1 = (ntiles + n1 - 1) / n1;
        if ((G0 + G1) * B <= slots || G0 + G1 <= 2) break;       // (rounding up twice can overshoot by a few workgroups)
    }
    // XCD-local sharing between the passes (round 4).  Tile t of a sample is walked by pass-0 workgroup t mod G0 and by pass-1 workgroup
    // t mod G1 at about the same time (the ratio above), and both read the target's and ref1's planes there.  Workgroups are dealt to the 8
    // XCDs round-robin by their linear index b (G0 + G1) + x: with G0 and G1 multiples of 8 both workgroups of a tile sit on XCD t mod 8 and
    // the second reader hits the first one's lines in that XCD's L2 -- otherwise the planes the passes share come from the fabric twice
    // (round 3 measured 93.5 MB per launch against 76.7 MB algorithmic).  Rounded up where the launch still fits one generation, else down.
    static const int xcd_align = MCAV_KNOB_INT("MCAV_WL_XCD", 1);
    if (xcd_align && G0 >= 8 && G1 >= 8) {
        int g0 = (G0 + 7) / 8 * 8, g1 = (G1 + 7) / 8 * 8;
        if ((g0 + g1) * B > slots) g1 = G1 / 8 * 8;
        if ((g0 + g1) * B > slots) g0 = G0 / 8 * 8;
        if (g0 >= 8 && g1 >= 8 && g0 <= ntiles && g1 <= ntiles && (g0 + g1) * B <= slots) { G0 = g0; G1 = g1; }
    }
}

inline dim3 pix_grid(int B, int H, int W) { return dim3((W + TW - 1) / TW, (H + TH - 1) / TH, B); }

}  // namespace mcav

using namespace mcav;

MCAV_EXPORT int mcav_abi_version(void) { return 1; }

MCAV_EXPORT size_t mcav_warp_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ws_layout(B, H, W).total;
}

// The fused kernels keep their completion tickets in the caller's workspace and leave them at zero (block_finish).  A launch that returned an
// error may not have run to that point: its workspace is remembered here and the NEXT launch on it zeroes the ticket region first (one
// 16 KB memset on the stream, only ever after a failure) -- otherwise no later launch on that cached workspace would elect a finisher and
// `losses` / `d_poses` would silently keep stale values.
static std::mutex g_suspect_mu;
static std::vector<void*> g_suspect_ws;
static bool take_suspect(void* ws) {
    std::lock_guard<std::mutex> lk(g_suspect_mu);
    for (size_t i = 0; i < g_suspect_ws.size(); ++i)
        if (g_suspect_ws[i] == ws) { g_suspect_ws.erase(g_suspect_ws.begin() + i); return true; }
    return false;
}
static void mark_suspect(void* ws) {
    std::lock_guard<std::mutex> lk(g_suspect_mu);
    for (void* p : g_suspect_ws) if (p == ws) return;
    g_suspect_ws.push_back(ws);
}

// one launch of the fused kernel of (photometric term, masked mode)
template <unsigned MODE>
static void launch_fused(const WLArgs& a0, hipStream_t s) {
    WLArgs a = a0;
    if (a.flags & MCAV_WL_SSIM) {
        const dim3 wl_grid((a.W + TW - 1) / TW, (a.H + WLH - 1) / WLH, a.B);
        timed_launch(warp_loss_ssim_kernel<false, MODE>, wl_grid, dim3(256), 0, s, a);
    } else {
        l1_grid(a.B, a.H, a.W, l1_slots<MODE>(), a.G0, a.G1);
        timed_launch(warp_loss_l1_kernel<false, MODE>, dim3(a.G0 + a.G1, a.B), dim3(256), 0, s, a);
    }
}

// one launch of the stereo kernel of (photometric term, masked mode)
template <unsigned MODE>
static void launch_stereo(const WLStereoArgs& a0, hipStream_t s) {
    WLStereoArgs a = a0;
    if (a.flags & MCAV_WL_SSIM) {
        const dim3 wl_grid((a.W + TW - 1) / TW, (a.H + WLH - 1) / WLH, a.B);
        timed_launch(warp_loss_ssim_stereo_kernel<MODE>, wl_grid, dim3(256), 0, s, a);
    } else {
        l1_grid(a.B, a.H, a.W, l1_stereo_slots<MODE>(), a.G0, a.G1, true);
        timed_launch(warp_loss_l1_stereo_kernel<MODE>, dim3(a.G0 + a.G1, a.B), dim3(256), 0, s, a);
    }
}

// stereo != nullptr: the stereo kernels (stereo [B,3,H,W], baseline [B] on the device, term_weights = 4 floats or nullptr)
static int warp_loss_launch(const float* tgt, const float* ref0, const float* ref1, const float* disp_t, const float* disp_r0,
                            const float* poses, const void* K, int B, int H, int W, unsigned flags, const float* upstream,
                            const float* term_weights, float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses,
                            void* workspace, size_t workspace_bytes, void* stream, float* dbg, unsigned mode = 0,
                            unsigned char* sel = nullptr, const float* stereo = nullptr, const float* baseline = nullptr) {
    if (!tgt || !ref0 || !ref1 || !disp_t || !disp_r0 || !poses || !K || !losses || !d_disp_t || !d_disp_r0 || !d_poses || !workspace)
        return MCAV_E_INVALID;
    if (B <= 0 || H < 3 || W < 3 || B > WL_MAX_B) return MCAV_E_INVALID;
    const WsLayout l = ws_layout(B, H, W);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t s = as_stream(stream);
    WLArgs a;
    a.tgt = tgt; a.ref0 = ref0; a.ref1 = ref1; a.disp_t = disp_t; a.disp_r0 = disp_r0; a.poses = poses;
    a.K = K; a.upstream = upstream; a.d_disp_t = d_disp_t; a.d_disp_r0 = d_disp_r0; a.d_poses = d_poses; a.losses = losses;
    a.slab = reinterpret_cast<float*>(ws + l.slab_off);
    a.sample_loss = reinterpret_cast<double*>(ws + l.sl_off);
    a.tickets = reinterpret_cast<unsigned*>(ws + l.tick_off);
    a.B = B; a.H = H; a.W = W; a.flags = flags; a.G0 = 0; a.G1 = 0;
    a.tw[0] = term_weights ? term_weights[0] : 0.25f;
    a.tw[1] = term_weights ? term_weights[1] : 0.25f;
    a.tw[2] = term_weights ? term_weights[2] : 0.5f;
    if (mode) a.sel = sel;
    else a.dbg = dbg;
    if (take_suspect(workspace) && hipMemsetAsync(a.tickets, 0, sizeof(unsigned) * ((size_t)WL_MAX_B + 1), s) != hipSuccess) {
        (void)hipGetLastError();
        mark_suspect(workspace);
        return MCAV_E_LAUNCH;
    }
    if (stereo) {
        WLStereoArgs st;
        static_cast<WLArgs&>(st) = a;
        st.sel = sel;                                            // (the plain stereo kernel never writes it)
        st.stereo = stereo;
        st.baseline = baseline;
        st.tw[0] = term_weights ? term_weights[0] : 1.0f / 6.0f;      // the target-view group is the mean of its three warps, warp 2 keeps half
        st.tw[1] = term_weights ? term_weights[1] : 1.0f / 6.0f;
        st.tw[2] = term_weights ? term_weights[2] : 0.5f;
        st.tws = term_weights ? term_weights[3] : 1.0f / 6.0f;
        if (mode == (WL_M_MIN | WL_M_AUTO)) launch_stereo<WL_M_MIN | WL_M_AUTO>(st, s);
        else if (mode == WL_M_MIN) launch_stereo<WL_M_MIN>(st, s);
        else if (mode == WL_M_AUTO) launch_stereo<WL_M_AUTO>(st, s);
        else launch_stereo<0>(st, s);
    } else if (mode == (WL_M_MIN | WL_M_AUTO)) launch_fused<WL_M_MIN | WL_M_AUTO>(a, s);
    else if (mode == WL_M_MIN) launch_fused<WL_M_MIN>(a, s);
    else if (mode == WL_M_AUTO) launch_fused<WL_M_AUTO>(a, s);
    else if (flags & MCAV_WL_SSIM) {
        const dim3 wl_grid((W + TW - 1) / TW, (H + WLH - 1) / WLH, B);
        if (dbg) timed_launch(warp_loss_ssim_kernel<true>, wl_grid, dim3(256), 0, s, a);
        else timed_launch(warp_loss_ssim_kernel<false>, wl_grid, dim3(256), 0, s, a);
    } else {
        l1_grid(B, H, W, l1_slots<0>(), a.G0, a.G1);
        const dim3 grid(a.G0 + a.G1, B);
        if (dbg) timed_launch(warp_loss_l1_kernel<true>, grid, dim3(256), 0, s, a);
        else timed_launch(warp_loss_l1_kernel<false>, grid, dim3(256), 0, s, a);
    }
    const int rc = launch_status();
    if (rc != MCAV_OK) mark_suspect(workspace);
    return rc;
}

MCAV_EXPORT int mcav_warp_loss_fwd_bwd(const float* tgt, const float* ref0, const float* ref1, const float* disp_t, const float* disp_r0,
                                       const float* poses, const void* K, int B, int H, int W, unsigned flags, const float* upstream,
                                       const float* term_weights, float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    return warp_loss_launch(tgt, ref0, ref1, disp_t, disp_r0, poses, K, B, H, W, flags, upstream, term_weights, losses, d_disp_t, d_disp_r0, d_poses,
                            workspace, workspace_bytes, stream, nullptr);
}

MCAV_EXPORT int mcav_warp_loss_masked_fwd_bwd(const float* tgt, const float* ref0, const float* ref1, const float* disp_t, const float* disp_r0,
                                              const float* poses, const void* K, int B, int H, int W, unsigned flags, const float* upstream,
                                              const float* term_weights, float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses,
                                              void* workspace, size_t workspace_bytes, void* stream, unsigned char* selection,
                                              size_t selection_bytes) {
    constexpr unsigned known = MCAV_WL_K_F64 | MCAV_WL_SKIP_IF_UNIT | MCAV_WL_NO_SMOOTH | MCAV_WL_INPUT_DEPTH | MCAV_WL_SSIM |
                               MCAV_WL_MIN_REPROJ | MCAV_WL_AUTOMASK;
    if (flags & ~known) return MCAV_E_INVALID;
    if (B <= 0 || H <= 0 || W <= 0) return MCAV_E_INVALID;
    const size_t sel_bytes = (size_t)B * 2 * H * W;
    if (selection && selection_bytes < sel_bytes) return MCAV_E_WORKSPACE;
    const unsigned mode = ((flags & MCAV_WL_MIN_REPROJ) ? WL_M_MIN : 0u) | ((flags & MCAV_WL_AUTOMASK) ? WL_M_AUTO : 0u);
    if (mode == 0 && selection) {       // the plain kernel keeps every warp everywhere
        const int rc = warp_loss_launch(tgt, ref0, ref1, disp_t, disp_r0, poses, K, B, H, W, flags, upstream, term_weights, losses, d_disp_t,
                                        d_disp_r0, d_poses, workspace, workspace_bytes, stream, nullptr);
        if (rc != MCAV_OK) return rc;
        return hipMemsetAsync(selection, 0, sel_bytes, as_stream(stream)) == hipSuccess ? MCAV_OK : MCAV_E_LAUNCH;
    }
    return warp_loss_launch(tgt, ref0, ref1, disp_t, disp_r0, poses, K, B, H, W, flags, upstream, term_weights, losses, d_disp_t, d_disp_r0,
                            d_poses, workspace, workspace_bytes, stream, nullptr, mode, selection);
}

MCAV_EXPORT int mcav_warp_loss_stereo_fwd_bwd(const float* tgt, const float* ref0, const float* ref1, const float* disp_t, const float* disp_r0,
                                              const float* poses, const void* K, int B, int H, int W, unsigned flags, const float* upstream,
                                              const float* term_weights, float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses,
                                              void* workspace, size_t workspace_bytes, void* stream, unsigned char* selection,
                                              size_t selection_bytes, const float* stereo, const float* stereo_baseline) {
    constexpr unsigned known = MCAV_WL_K_F64 | MCAV_WL_SKIP_IF_UNIT | MCAV_WL_NO_SMOOTH | MCAV_WL_INPUT_DEPTH | MCAV_WL_SSIM |
                               MCAV_WL_MIN_REPROJ | MCAV_WL_AUTOMASK;
    if (flags & ~known) return MCAV_E_INVALID;
    if (!stereo || !stereo_baseline || B <= 0 || H <= 0 || W <= 0) return MCAV_E_INVALID;
    const size_t sel_bytes = (size_t)B * 2 * H * W;
    if (selection && selection_bytes < sel_bytes) return MCAV_E_WORKSPACE;
    const unsigned mode = ((flags & MCAV_WL_MIN_REPROJ) ? WL_M_MIN : 0u) | ((flags & MCAV_WL_AUTOMASK) ? WL_M_AUTO : 0u);
    const int rc = warp_loss_launch(tgt, ref0, ref1, disp_t, disp_r0, poses, K, B, H, W, flags, upstream, term_weights, losses, d_disp_t,
                                    d_disp_r0, d_poses, workspace, workspace_bytes, stream, nullptr, mode, mode ? selection : nullptr, stereo,
                                    stereo_baseline);
    if (rc != MCAV_OK || mode != 0 || !selection) return rc;
    return hipMemsetAsync(selection, 0, sel_bytes, as_stream(stream)) == hipSuccess ? MCAV_OK : MCAV_E_LAUNCH;      // plain: every warp kept
}

// resident workgroups of the fused L1 instantiation of (masked mode, stereo): the same cached answers the launches above take
static int l1_slots_of(unsigned mode, bool stereo) {
    if (stereo) {
        if (mode == (WL_M_MIN | WL_M_AUTO)) return l1_stereo_slots<WL_M_MIN | WL_M_AUTO>();
        if (mode == WL_M_MIN) return l1_stereo_slots<WL_M_MIN>();
        if (mode == WL_M_AUTO) return l1_stereo_slots<WL_M_AUTO>();
        return l1_stereo_slots<0>();
    }
    if (mode == (WL_M_MIN | WL_M_AUTO)) return l1_slots<WL_M_MIN | WL_M_AUTO>();
    if (mode == WL_M_MIN) return l1_slots<WL_M_MIN>();
    if (mode == WL_M_AUTO) return l1_slots<WL_M_AUTO>();
    return l1_slots<0>();
}

// The planner of the fused L1 launches as a query: l1_grid itself, nothing launched (the precedent is mcav_igemm_route).
MCAV_EXPORT int mcav_warp_loss_l1_grid(int B, int H, int W, unsigned flags, int stereo, int slots, int* G0, int* G1) {
    constexpr unsigned known = MCAV_WL_K_F64 | MCAV_WL_SKIP_IF_UNIT | MCAV_WL_NO_SMOOTH | MCAV_WL_INPUT_DEPTH | MCAV_WL_SSIM |
                               MCAV_WL_MIN_REPROJ | MCAV_WL_AUTOMASK;
    if (!G0 || !G1 || slots < 0 || (flags & ~known) || (flags & MCAV_WL_SSIM)) return MCAV_E_INVALID;
    if (B <= 0 || H < 3 || W < 3 || B > WL_MAX_B) return MCAV_E_INVALID;
    const unsigned mode = ((flags & MCAV_WL_MIN_REPROJ) ? WL_M_MIN : 0u) | ((flags & MCAV_WL_AUTOMASK) ? WL_M_AUTO : 0u);
    if (slots == 0) slots = l1_slots_of(mode, stereo != 0);
    l1_grid(B, H, W, slots, *G0, *G1, stereo != 0);
    return MCAV_OK;
}

// Diagnostic twin of mcav_warp_loss_fwd_bwd: the same kernel bodies instantiated with their per-pixel dump on.
MCAV_EXPORT int mcav_warp_loss_debug_taps(const float* tgt, const float* ref0, const float* ref1, const float* disp_t, const float* disp_r0,
                                          const float* poses, const void* K, int B, int H, int W, unsigned flags, const float* term_weights,
                                          float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses, void* workspace,
                                          size_t workspace_bytes, float* taps, size_t taps_floats, void* stream) {
    if (!taps || (flags & MCAV_WL_SKIP_IF_UNIT) || B <= 0 || H <= 0 || W <= 0) return MCAV_E_INVALID;
    if (taps_floats < (size_t)B * 3 * WL_DBG * H * W) return MCAV_E_WORKSPACE;
    return warp_loss_launch(tgt, ref0, ref1, disp_t, disp_r0, poses, K, B, H, W, flags, nullptr, term_weights, losses, d_disp_t, d_disp_r0, d_poses,
                            workspace, workspace_bytes, stream, taps);
}

MCAV_EXPORT int mcav_inverse_warp_fwd(const float* img, const float* depth, const float* pose, const void* K, int B, int H, int W, int pose_inv,
                                      unsigned flags, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!img || !depth || !pose || !K || !out || !workspace || B <= 0 || H < 2 || W < 2 || B > 65535) return MCAV_E_INVALID;
    const WsLayout l = ws_layout(B, H, W);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    PrepConst* pc = reinterpret_cast<PrepConst*>(reinterpret_cast<char*>(workspace) + l.pc_off);
    hipStream_t s = as_stream(stream);
    pose_prepare_kernel<<<(B + 63) / 64, 64, 0, s>>>(pose, K, nullptr, B, 1, pose_inv, (flags & MCAV_WL_K_F64) ? 1 : 0, pc, nullptr);
    inverse_warp_fwd_kernel<<<pix_grid(B, H, W), 256, 0, s>>>(img, depth, pc, B, H, W, out);
    return launch_status();
}

MCAV_EXPORT int mcav_inverse_warp_bwd(const float* img, const float* depth, const float* pose, const void* K, const float* grad_out, int B, int H,
                                      int W, int pose_inv, unsigned flags, float* d_depth, float* d_pose, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    if (!img || !depth || !pose || !K || !grad_out || !d_depth || !d_pose || !workspace || B <= 0 || H < 2 || W < 2 || B > 65535)
        return MCAV_E_INVALID;
    const WsLayout l = ws_layout(B, H, W);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    PrepConst* pc = reinterpret_cast<PrepConst*>(ws + l.pc_off);
    float* slab = reinterpret_cast<float*>(ws + l.slab_off);
    hipStream_t s = as_stream(stream);
    pose_prepare_kernel<<<(B + 63) / 64, 64, 0, s>>>(pose, K, nullptr, B, 1, pose_inv, (flags & MCAV_WL_K_F64) ? 1 : 0, pc, nullptr);
    inverse_warp_bwd_kernel<<<pix_grid(B, H, W), 256, 0, s>>>(img, depth, pc, grad_out, B, H, W, d_depth, slab);
    inverse_warp_bwd_finalize_kernel<<<B, 64, 0, s>>>(slab, l.nblk, pc, pose, pose_inv, d_pose);
    return launch_status();
}

MCAV_EXPORT int mcav_reconstruct(const float* depth, const void* K, int B, int H, int W, unsigned flags, float* points, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!depth || !K || !points || !workspace || B <= 0 || H <= 0 || W <= 0 || B > 65535) return MCAV_E_INVALID;
    const WsLayout l = ws_layout(B, H, W);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    PrepConst* pc = reinterpret_cast<PrepConst*>(reinterpret_cast<char*>(workspace) + l.pc_off);
    hipStream_t s = as_stream(stream);
    pose_prepare_kernel<<<(B + 63) / 64, 64, 0, s>>>(nullptr, K, nullptr, B, 3, 0, (flags & MCAV_WL_K_F64) ? 1 : 0, pc, nullptr);
    reconstruct_kernel<<<pix_grid(B, H, W), 256, 0, s>>>(depth, pc, B, H, W, points);
    return launch_status();
}

MCAV_EXPORT int mcav_project(const float* points, const void* K, const float* Tcw, int B, int H, int W, unsigned flags, float* grid, void* stream) {
    if (!points || !K || !Tcw || !grid || B <= 0 || H < 2 || W < 2 || B > 65535) return MCAV_E_INVALID;
    project_kernel<<<pix_grid(B, H, W), 256, 0, as_stream(stream)>>>(points, K, (flags & MCAV_WL_K_F64) ? 1 : 0, Tcw, B, H, W, grid);
    return launch_status();
}

MCAV_EXPORT int mcav_pose_to_matrix(const float* pose, int B, int invert, float* T, void* stream) {
    if (!pose || !T || B <= 0) return MCAV_E_INVALID;
    pose_to_matrix_kernel<<<(B + 63) / 64, 64, 0, as_stream(stream)>>>(pose, B, invert, T);
    return launch_status();
}

MCAV_EXPORT int mcav_invert_pose(const float* T, int B, float* Tinv, void* stream) {
    if (!T || !Tinv || B <= 0) return MCAV_E_INVALID;
    invert_pose_kernel<<<(B + 63) / 64, 64, 0, as_stream(stream)>>>(T, B, Tinv);
    return launch_status();
}

MCAV_EXPORT int mcav_disp_to_depth(const float* disp, float* depth, size_t n, void* stream) {
    if (!disp || !depth) return MCAV_E_INVALID;
    if (n == 0) return MCAV_OK;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    disp_to_depth_kernel<<<blocks, 256, 0, as_stream(stream)>>>(disp, depth, n);
    return launch_status();
}

MCAV_EXPORT int mcav_disp_to_depth_bwd(const float* disp, const float* d_depth, float* d_disp, size_t n, void* stream) {
    if (!disp || !d_depth || !d_disp) return MCAV_E_INVALID;
    if (n == 0) return MCAV_OK;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    disp_to_depth_bwd_kernel<<<blocks, 256, 0, as_stream(stream)>>>(disp, d_depth, d_disp, n);
    return launch_status();
}

MCAV_EXPORT int mcav_ssim_fwd(const float* x, const float* y, int N, int H, int W, float C1, float C2, float* out, void* stream) {
    if (!x || !y || !out || N <= 0 || H < 2 || W < 2 || N > 65535) return MCAV_E_INVALID;
    ssim_kernel<<<pix_grid(N, H, W), 256, 0, as_stream(stream)>>>(x, y, N, H, W, C1, C2, out);
    return launch_status();
}

MCAV_EXPORT size_t mcav_smooth_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ws_layout(B, H, W).total;
}

MCAV_EXPORT int mcav_smooth_loss_fwd_bwd(const float* depth, int B, int H, int W, float weight, const float* upstream, float* loss_accum,
                                         float* d_depth, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    if (!depth || !loss_accum || !d_depth || !workspace || B <= 0 || H < 3 || W < 3 || B > 65535) return MCAV_E_INVALID;
    const WsLayout l = ws_layout(B, H, W);
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    float* slab = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + l.slab_off);
    hipStream_t s = as_stream(stream);
    smooth_kernel<<<pix_grid(B, H, W), 256, 0, s>>>(depth, B, H, W, weight, upstream, d_depth, accumulate, slab);
    smooth_finalize_kernel<<<1, 256, 0, s>>>(slab, l.nblk * B, loss_accum);
    return launch_status();
}
