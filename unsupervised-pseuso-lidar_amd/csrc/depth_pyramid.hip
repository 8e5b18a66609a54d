// The depth pyramid of the multi-scale loss: every coarse disparity map of both depth passes -> full-resolution depth, in ONE launch, and
// the adjoint in ONE launch (include/mcav_depth.h: mcav_depth_pyramid_fwd / _bwd).  Replaces, per coarse scale and per pass, one
// mcav_disp_to_depth and one mcav_resize_bilinear_fwd launch forward and the same again backward.
//
// Forward: one thread per 4 consecutive outputs of one level (16-byte stores); the coarse maps are small and stay in cache.
// Backward: the bilinear adjoint is separable.  A workgroup owns TY x TX coarse pixels of one level and sample.  It walks the
// full-resolution rows that touch them in chunks of RC rows: stage the chunk in LDS (16-byte loads), reduce every staged row along x onto
// the tile's TX columns, then reduce those row sums along y into one register per coarse pixel.  Every sum runs in ascending index order
// and nothing is shared between workgroups: no atomics, bit-identical from run to run.  About 2 / scale + 2 terms per axis instead of
// their product.
#include "mcav_common.h"
#include "pyramid_math.h"

namespace mcav {

struct PyrLevels {
    mcav_pyr_level v[MCAV_PYR_MAX_LEVELS];
};

// the records arrive in the kernel-argument segment; a select chain on the (workgroup-uniform) level keeps them in scalar registers
__device__ __forceinline__ mcav_pyr_level pyr_pick(const PyrLevels& L, int l) { return l == 0 ? L.v[0] : (l == 1 ? L.v[1] : L.v[2]); }

typedef float pyr_v4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__global__ __launch_bounds__(256) void depth_pyramid_fwd_kernel(PyrLevels L, int B, int H, int W, unsigned flags, float* __restrict__ out) {
    const int l = blockIdx.y;
    const mcav_pyr_level lv = pyr_pick(L, l);
    const int h = lv.h, w = lv.w;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const bool rtd = (flags & MCAV_PYR_RESIZE_THEN_DEPTH) != 0;
    constexpr int V = VEC ? 4 : 1;
    const int Wv = W / V;                                   // VEC: W % 4 == 0
    const size_t total = (size_t)B * H * Wv;
    float* o = out + (size_t)l * B * H * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int xv = (int)(i % Wv);
        const size_t r = i / Wv;
        const int oy = (int)(r % H);
        const int b = (int)(r / H);
        int y0, y1;
        float ly;
        pyr::bil_src(oy, sy, h, y0, y1, ly);
        const float* p = lv.disp + (size_t)b * h * w;
        float res[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            int x0, x1;
            float lx;
            pyr::bil_src(xv * V + k, sx, w, x0, x1, lx);
            res[k] = pyr::fwd_value(p, w, y0, y1, ly, x0, x1, lx, rtd);
        }
        if (VEC) {
            const pyr_v4 v = {res[0], res[V > 1 ? 1 : 0], res[V > 2 ? 2 : 0], res[V > 3 ? 3 : 0]};
            reinterpret_cast<pyr_v4*>(o)[i] = v;
        } else {
            o[i] = res[0];
        }
    }
}

constexpr int PYR_TX = 32, PYR_TY = 8;      // coarse tile: one pixel per thread in the y reduction
constexpr int PYR_RC = 16;                  // full-resolution rows staged at a time (two per thread in the x reduction)
constexpr int PYR_XC = 288;                 // columns staged at a time: a 32-column tile at ratio 8 needs 33 * 8 + alignment
constexpr int PYR_XS = PYR_XC + 4;          // row stride in LDS: 16-byte aligned rows that do not all start on one bank

template <bool VEC>
__global__ __launch_bounds__(256) void depth_pyramid_bwd_kernel(PyrLevels L, int B, int H, int W, unsigned flags, const float* __restrict__ out,
                                                                const float* __restrict__ d_out) {
    __shared__ __attribute__((aligned(16))) float G[PYR_RC][PYR_XS];
    __shared__ float XR[PYR_RC][PYR_TX];
    const int l = blockIdx.y;
    const mcav_pyr_level lv = pyr_pick(L, l);
    const int h = lv.h, w = lv.w;
    const int tiles_x = (w + PYR_TX - 1) / PYR_TX, tiles_y = (h + PYR_TY - 1) / PYR_TY;
    const size_t tiles = (size_t)B * tiles_y * tiles_x;
    if ((size_t)blockIdx.x >= tiles) return;                // (the grid is sized for the level with the most tiles)
    const int tx = (int)(blockIdx.x % tiles_x), ty = (int)((blockIdx.x / tiles_x) % tiles_y), b = (int)(blockIdx.x / ((size_t)tiles_x * tiles_y));
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const bool rtd = (flags & MCAV_PYR_RESIZE_THEN_DEPTH) != 0;
    const int tid = threadIdx.x;
    const int c0 = tx * PYR_TX, r0 = ty * PYR_TY;
    const int c1 = (c0 + PYR_TX < w ? c0 + PYR_TX : w) - 1, r1 = (r0 + PYR_TY < h ? r0 + PYR_TY : h) - 1;
    // the full-resolution region that touches the tile (windows are nested in order: lo and hi never decrease with the source index)
    int Xlo, Xhi, Ylo, Yhi, unused;
    pyr::adjoint_window(c0, sx, w, W, Xlo, unused);
    pyr::adjoint_window(c1, sx, w, W, unused, Xhi);
    pyr::adjoint_window(r0, sy, h, H, Ylo, unused);
    pyr::adjoint_window(r1, sy, h, H, unused, Yhi);
    // this thread's coarse pixel (y reduction) and its column and row pair (x reduction)
    const int cc = tid % PYR_TX, rg = tid / PYR_TX;
    const int ix = c0 + cc, iy = r0 + rg;
    const bool col_ok = ix < w, pix_ok = col_ok && iy < h;
    int xlo = 0, xhi = -1, ylo = 0, yhi = -1;
    if (col_ok) pyr::adjoint_window(ix, sx, w, W, xlo, xhi);
    if (pix_ok) pyr::adjoint_window(iy, sy, h, H, ylo, yhi);
    const size_t plane = ((size_t)l * B + b) * H * W;
    const int Xa = VEC ? (Xlo & ~3) : Xlo;                  // VEC: W % 4 == 0 and the bases are 16-byte aligned
    float acc = 0.f;
    for (int yc = Ylo; yc <= Yhi; yc += PYR_RC) {
        const int nr = Yhi - yc + 1 < PYR_RC ? Yhi - yc + 1 : PYR_RC;
        float xs0 = 0.f, xs1 = 0.f;                          // rows yc + rg and yc + rg + 8 reduced onto column ix
        for (int xc = Xa; xc <= Xhi; xc += PYR_XC) {
            const int nx = Xhi - xc + 1 < PYR_XC ? Xhi - xc + 1 : PYR_XC;
            __syncthreads();                                 // the previous chunk's readers are done with G
            if (VEC) {
                const int nq = (nx + 3) / 4;                 // xc % 4 == 0 and W % 4 == 0: the last quad ends inside the row
                for (int i = tid; i < nr * nq; i += 256) {
                    const int rr = i / nq, q = i - rr * nq;
                    const size_t at = plane + (size_t)(yc + rr) * W + xc + 4 * q;
                    pyr_v4 g = *reinterpret_cast<const pyr_v4*>(d_out + at);
                    if (rtd) {                               // d depth / d (resized disparity) at the stored depth
                        const pyr_v4 D = *reinterpret_cast<const pyr_v4*>(out + at);
                        g.x *= pyr::depth_slope(D.x); g.y *= pyr::depth_slope(D.y); g.z *= pyr::depth_slope(D.z); g.w *= pyr::depth_slope(D.w);
                    }
                    *reinterpret_cast<pyr_v4*>(&G[rr][4 * q]) = g;
                }
            } else {
                for (int i = tid; i < nr * nx; i += 256) {
                    const int rr = i / nx, q = i - rr * nx;
                    const size_t at = plane + (size_t)(yc + rr) * W + xc + q;
                    float g = d_out[at];
                    if (rtd) g *= pyr::depth_slope(out[at]);
                    G[rr][q] = g;
                }
            }
            __syncthreads();
            const int a = xlo > xc ? xlo : xc, e = xhi < xc + nx - 1 ? xhi : xc + nx - 1;
            float p0 = 0.f, p1 = 0.f;                        // (rows at or past nr hold stale values: summed, never read back)
            for (int ox = a; ox <= e; ++ox) {
                const float wgt = pyr::tap_weight(ox, ix, sx, w);
                p0 += wgt * G[rg][ox - xc];
                p1 += wgt * G[rg + 8][ox - xc];
            }
            xs0 += p0;
            xs1 += p1;
        }
        XR[rg][cc] = xs0;
        XR[rg + 8][cc] = xs1;
        __syncthreads();
        const int a = ylo > yc ? ylo : yc, e = yhi < yc + nr - 1 ? yhi : yc + nr - 1;
        for (int oy = a; oy <= e; ++oy) acc += pyr::tap_weight(oy, iy, sy, h) * XR[oy - yc][cc];
        // (XR is rewritten only after the next chunk's two barriers)
    }
    if (pix_ok) {
        const size_t at = ((size_t)b * h + iy) * w + ix;
        if (!rtd) acc *= pyr::depth_slope(pyr::depth_of(lv.disp[at]));      // disp_to_depth's derivative at the coarse pixel
        lv.d_disp[at] = acc;
    }
}

inline bool pyr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int pyr_check(const mcav_pyr_level* levels, int nlevels, int B, int H, int W, unsigned flags, bool backward, PyrLevels& L) {
    if (!levels || nlevels < 1 || nlevels > MCAV_PYR_MAX_LEVELS || B <= 0 || H <= 0 || W <= 0) return MCAV_E_INVALID;
    if (flags & ~(unsigned)MCAV_PYR_RESIZE_THEN_DEPTH) return MCAV_E_INVALID;
    if ((size_t)B * H > 0x7fffffffu / (size_t)W) return MCAV_E_INVALID;        // one level's outputs are indexed within 2^31 rows x columns
    for (int l = 0; l < MCAV_PYR_MAX_LEVELS; ++l) {
        L.v[l] = levels[l < nlevels ? l : 0];
        if (l >= nlevels) continue;
        const mcav_pyr_level& v = levels[l];
        if (v.h < 1 || v.w < 1 || v.h > H || v.w > W) return MCAV_E_INVALID;   // upsampling only, as mcav_resize_bilinear_bwd
        if (backward ? !v.d_disp || (!(flags & MCAV_PYR_RESIZE_THEN_DEPTH) && !v.disp) : !v.disp) return MCAV_E_INVALID;
    }
    return MCAV_OK;
}

}  // namespace mcav

using namespace mcav;

MCAV_EXPORT int mcav_depth_pyramid_fwd(const mcav_pyr_level* levels, int nlevels, int B, int H, int W, unsigned flags, float* out, void* stream) {
    PyrLevels L;
    if (!out) return MCAV_E_INVALID;
    const int rc = pyr_check(levels, nlevels, B, H, W, flags, false, L);
    if (rc != MCAV_OK) return rc;
    const bool vec = (W % 4 == 0) && pyr_aligned16(out);
    const size_t items = (size_t)B * H * (vec ? W / 4 : W);
    const size_t blocks = (items + 255) / 256;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192), (unsigned)nlevels);
    if (vec) depth_pyramid_fwd_kernel<true><<<grid, 256, 0, as_stream(stream)>>>(L, B, H, W, flags, out);
    else depth_pyramid_fwd_kernel<false><<<grid, 256, 0, as_stream(stream)>>>(L, B, H, W, flags, out);
    return launch_status();
}

MCAV_EXPORT int mcav_depth_pyramid_bwd(const mcav_pyr_level* levels, int nlevels, int B, int H, int W, unsigned flags, const float* out,
                                       const float* d_out, void* stream) {
    PyrLevels L;
    if (!d_out || ((flags & MCAV_PYR_RESIZE_THEN_DEPTH) && !out)) return MCAV_E_INVALID;
    const int rc = pyr_check(levels, nlevels, B, H, W, flags, true, L);
    if (rc != MCAV_OK) return rc;
    size_t tiles = 0;
    for (int l = 0; l < nlevels; ++l) {
        const size_t t = (size_t)B * ((L.v[l].h + PYR_TY - 1) / PYR_TY) * ((L.v[l].w + PYR_TX - 1) / PYR_TX);
        tiles = t > tiles ? t : tiles;
    }
    if (tiles > 0x7fffffffu) return MCAV_E_INVALID;
    const bool vec = (W % 4 == 0) && pyr_aligned16(d_out) && (!(flags & MCAV_PYR_RESIZE_THEN_DEPTH) || pyr_aligned16(out));
    const dim3 grid((unsigned)tiles, (unsigned)nlevels);
    if (vec) depth_pyramid_bwd_kernel<true><<<grid, 256, 0, as_stream(stream)>>>(L, B, H, W, flags, out, d_out);
    else depth_pyramid_bwd_kernel<false><<<grid, 256, 0, as_stream(stream)>>>(L, B, H, W, flags, out, d_out);
    return launch_status();
}
