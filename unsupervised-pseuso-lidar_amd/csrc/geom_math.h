// Per-pixel arithmetic of the depth geometry-consistency term (SC-SfMLearner, Bian et al. 2019), shared by the HIP kernels
// (geom_consistency.hip) and by the host-compiled check in tests/geom_hostcheck (never by the product).  The definition is
// tests/geom_consistency_ref.py and include/mcav_depth.h (mcav_geom_consistency_fwd).  For a pixel p = (x, y) of frame a with depth D_a:
//   c      = P [K^-1 [x y 1]^T D_a ; 1],  P = K [R|t]                (make_fast / project_fast of warp_math.h: the fused loss kernel's cell)
//   D_proj = c2,   D_samp = bilinear sample of D_b at (ix, iy), zero padding
//   valid  = 0 <= ix <= W-1 && 0 <= iy <= H-1 && D_proj >= 1e-3     (NaN: invalid)
//   diff   = |D_proj - D_samp| / (D_proj + D_samp)                   (|.|' at 0 is 0)
// SC-SfMLearner clamps D_proj at 1e-3 where this term drops the pixel: a clamped pixel has no gradient through D_proj either, and a depth
// behind the camera says nothing about D_b.
#pragma once
#include <math.h>
#include <stdint.h>

#include "warp_math.h"

namespace mcav {
namespace gc {

constexpr float MIN_DEPTH = 1e-3f;
// The scatter's fixed point: a tap's contribution w_tap * d diff / d D_samp, clamped to [-FIX_CLAMP, FIX_CLAMP], times 2^FIX_SHIFT, as a
// 64-bit integer.  |d diff / d D_samp| <= 1 / (2 D_samp): depths from disp_to_depth are >= 0.0999, so the bound is 5.005 and the clamp
// never acts; with MCAV_WL_INPUT_DEPTH it needs depth > 1/16.  FIX_CLAMP is the float just below 8: a texel receives at most one tap
// from each of the H*W <= 2^24 pixels of a, so |sum| <= FIX_CLAMP * 2^36 * 2^24 < 2^63 strictly -- a destination cannot overflow.
constexpr int FIX_SHIFT = 36;
constexpr float FIX_CLAMP = 7.99999952316284f;       // 8 - 2^-21
constexpr float FIX_ONE = 68719476736.0f;             // 2^36
constexpr double FIX_INV = 1.0 / 68719476736.0;

// One direction's per-sample constants, formed exactly as the fused loss kernel's prologue forms them (float64 inverse of K, fp32
// Rodrigues and P = K [R|t], Q = P[:, :3] K^-1 in float64): direction 0 is its warp 0, direction 1 its warp 2.
struct Dir {
    WarpFast wf;
    float Kinv[9];
    float Kf[9];
};

MCAV_HD void make_dir(const double* Kd, const float* pose, bool invert, Dir& d) {
    double Ki[9];
    invert3x3(Kd, Ki);
    float R[9], t[3], P[12];
    for (int i = 0; i < 9; ++i) { d.Kf[i] = (float)Kd[i]; d.Kinv[i] = (float)Ki[i]; }
    pose_to_Rt(pose, invert, R, t);
    make_P(d.Kf, R, t, P);
    make_fast(P, d.Kinv, d.wf);
}

MCAV_HD float depth_of(float v, bool in_depth) { return in_depth ? v : rcp_nr(fmaf(10.0f, v, 0.01f)); }

struct Pixel {
    FTap t;
    float Dp;          // D_proj = c2
    bool valid;
};

// live: false for the pixels of a ragged tile past the image edge (never valid, every tap out of the image)
MCAV_HD Pixel project(const WarpFast& f, float x, float y, float D, int H, int W, bool live = true) {
    Pixel p;
    p.t = project_fast(f, x, y, D, H, W, live);
    p.Dp = fmaf(D, p.t.q2, f.p3[2]);                   // the c2 project_fast divides by
    p.valid = live && p.t.ix >= 0.0f && p.t.ix <= (float)(W - 1) && p.t.iy >= 0.0f && p.t.iy <= (float)(H - 1) && p.Dp >= MIN_DEPTH;
    return p;
}

struct Eval {
    float diff;        // |D_proj - D_samp| / (D_proj + D_samp)
    float gp, gs;      // d diff / d D_proj, d diff / d D_samp
};

MCAV_HD Eval evaluate(float Dp, float Ds) {
    const float s = Dp + Ds, r = Dp - Ds;
    const float is = rcp_nr(s);
    const float k = (2.0f * sgn_exact(r)) * (is * is);
    Eval e;
    e.diff = fabsf(r) * is;
    e.gp = k * Ds;
    e.gs = -(k * Dp);
    return e;
}

// d D_samp / d texel: nw, ne, sw, se
MCAV_HD void tap_weights(const FTap& t, float* w4) {
    const float wx0 = 1.0f - t.wx1, wy0 = 1.0f - t.wy1;
    w4[0] = wx0 * wy0; w4[1] = t.wx1 * wy0; w4[2] = wx0 * t.wy1; w4[3] = t.wx1 * t.wy1;
}

MCAV_HD long long to_fixed(float g) {
    const float c = fminf(fmaxf(g, -FIX_CLAMP), FIX_CLAMP);      // (NaN -> -FIX_CLAMP: the conversion below is always defined)
    return llrintf(c * FIX_ONE);
}

MCAV_HD void camera_point(const float* Kinv, float x, float y, float D, float* X) {
    X[0] = fmaf(Kinv[0], x, fmaf(Kinv[1], y, Kinv[2])) * D;
    X[1] = fmaf(Kinv[3], x, fmaf(Kinv[4], y, Kinv[5])) * D;
    X[2] = fmaf(Kinv[6], x, fmaf(Kinv[7], y, Kinv[8])) * D;
}

// d diff / d c (3 floats, d diff / d D_proj included in dc[2]) and the return value d diff / d D_a: through D_proj and through the
// sampling position.
MCAV_HD float backward(const Pixel& p, const Sample& s, const Eval& e, int H, int W, float* dc) {
    const float dD = backproject_dc(p.t, e.gs * s.dvdx, e.gs * s.dvdy, H, W, dc);
    dc[2] += e.gp;
    return fmaf(e.gp, p.t.q2, dD);
}

// One pixel of frame a: everything both kernels need.  texel(i) -> D_b at flat index i (a depth).
struct Result {
    Pixel p;
    Eval e;
    float dD;          // d diff / d D_a (0 where invalid)
    float dc[3];       // (0 where invalid)
    float tap[4];      // w_tap * d diff / d D_samp (0 where invalid or the tap is outside the image)
    int idx[4];        // flat index of each tap (meaningful where tap != 0)
};

template <class Tex>
MCAV_HD Result pixel(const WarpFast& f, int x, int y, float D, int H, int W, bool live, Tex texel) {
    Result r;
    r.p = project(f, (float)x, (float)y, D, H, W, live);
    const FTap& t = r.p.t;
    const int base = t.y0 * W + t.x0;
    r.idx[0] = base; r.idx[1] = base + 1; r.idx[2] = base + W; r.idx[3] = base + W + 1;
    const bool in[4] = {t.in00, t.in01, t.in10, t.in11};
    float q[4];
    for (int k = 0; k < 4; ++k) q[k] = in[k] ? texel(r.idx[k]) : 0.0f;
    const Sample s = bilinear_lerp(q[0], q[1], q[2], q[3], t.wx1, t.wy1);
    r.e = evaluate(r.p.Dp, s.v);
    float dc[3], w4[4];
    const float dD = backward(r.p, s, r.e, H, W, dc);
    tap_weights(t, w4);
    const bool v = r.p.valid;
    r.dD = v ? dD : 0.0f;
    for (int i = 0; i < 3; ++i) r.dc[i] = v ? dc[i] : 0.0f;
    for (int k = 0; k < 4; ++k) r.tap[k] = (v && in[k]) ? w4[k] * r.e.gs : 0.0f;
    return r;
}

// E_d and the gradient factor of one direction from its sums: n valid pixels, S = sum of diff over them.
MCAV_HD double direction_loss(double n, double S, int min_valid) { return n > (double)min_valid ? S / n : 0.0; }
MCAV_HD double direction_scale(double n, int min_valid) { return n > (double)min_valid ? 0.5 / n : 0.0; }

}  // namespace gc
}  // namespace mcav
