// Arithmetic of oriented 3-D boxes (include/mcav_depth.h: mcav_box_iou, mcav_box_nms): validity, the sine and cosine of a heading, the
// prepared form of a box, the bird's-eye-view intersection of two of them by polygon clipping, both overlaps, and the order of the
// candidates of the greedy suppression.  Shared by the HIP kernels (box.hip) and by the host-compiled check in tests/box_hostcheck (never
// by the product on the host, apart from the argument checks and the workspace layout).  The definition is tests/box_ref.py.  float32 with
// every operation rounded on its own and fmaf where the definition says fmaf: the device build switches contraction off below (as
// pl_math.h), the host build is compiled with -ffp-contract=off; the division and the square root are the correctly rounded ones.
//
// A box is 7 float32 (x, y, z, dx, dy, dz, heading): the centre, dx along the heading, the heading a rotation about +z, counter-clockwise
// (OpenPCDet's LiDAR frame).  What stands on this header next: anchor decoding, KITTI AP, target assignment, points in boxes.
#pragma once
#include "pillar_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcav {
namespace box {

constexpr int COLS = 7;
constexpr int MODE_BEV = 0, MODE_3D = 1;
constexpr int MAX_VERTS = 8;                       // a quadrilateral cut by four half-planes
constexpr int REFUSED = -1, SHORT_WORKSPACE = -2;  // MCAV_E_INVALID, MCAV_E_WORKSPACE
constexpr int NMS_MAX_CANDIDATES = 4096;           // MCAV_NMS_MAX_CANDIDATES: 64 lanes x 64 bits of the scan's "removed" set
constexpr int MAX_IMAGES = 65535, MAX_IOU_ROWS = 65535 * 64;

// A box is valid when all seven are finite, MIN_EXTENT <= dx, dy, dz <= MAX_EXTENT and |heading| <= MAX_HEADING (above 8 pi: a regressed
// heading that was never wrapped).  The lower limit keeps every area and volume a normal number.
constexpr float MIN_EXTENT = 1e-3f, MAX_EXTENT = 1024.0f, MAX_HEADING = 32.0f;
// centres further apart than the sum of the half-diagonals (with this slack on the squared sum: the test is conservative) do not overlap
constexpr float CIRCLE_SLACK = 1.0001f;

// A product and a sum that stay a product and a sum: written here, under the pragma above, so that the device compiler cannot contract
// one into the other (ev::mul_rn and ev::add_rn are plain operators of a header compiled with contraction allowed: a product of the
// first that feeds the second becomes a fused multiply-add on the device).
MCAV_PIL_HD float mul_rn(float a, float b) { return a * b; }
MCAV_PIL_HD float add_rn(float a, float b) { return a + b; }

MCAV_PIL_HD bool valid(const float* b) {
    for (int k = 0; k < COLS; ++k)
        if (!pil::finite(b[k])) return false;
    for (int k = 3; k < 6; ++k)
        if (!(b[k] >= MIN_EXTENT && b[k] <= MAX_EXTENT)) return false;
    return fabsf(b[6]) <= MAX_HEADING;
}

// ---------------------------------------------------------------------------------------------- box_sincos
// sin(h) and cos(h) in float32 for |h| <= MAX_HEADING from fmaf, float32 sums and integer arithmetic alone, so that the host and the
// device give the same bits.  k = the nearest integer to h 2/pi (the 1.5 * 2^23 trick), r = ((h - k HI) - k MID) - k LO (Cody-Waite:
// HI has 19 bits, |k| <= 21, so k HI and the first difference are exact), the two polynomials of degree 7 and 6 in r on [-pi/4, pi/4],
// then the quadrant k mod 4.
// BOX_SINCOS_MAX_ULP bounds |s - sin(h)| in units of the last place of sin(h), and the same for the cosine, over EVERY float32 h with
// |h| <= MAX_HEADING (2 214 592 514 arguments, both signs of zero among them), measured against the float64 functions by
// tests/box_hostcheck (`box_hostcheck --sincos-ulp`): the maximum found is 1.552836 ulp, at h = 0x1.9f8aaep+4.
constexpr float BOX_SINCOS_MAX_ULP = 1.5625f;
constexpr float SC_TWO_OVER_PI = 0.6366197466850281f, SC_ROUND = 12582912.0f;
constexpr float SC_PIO2_HI = 1.5707969665527344f, SC_PIO2_MID = -6.397578431460715e-07f, SC_PIO2_LO = 5.390302953474238e-15f;
constexpr float SC_S1 = -1.6666654611e-1f, SC_S2 = 8.3321608736e-3f, SC_S3 = -1.9515295891e-4f;
constexpr float SC_C1 = 4.166664568298827e-2f, SC_C2 = -1.388731625493765e-3f, SC_C3 = 2.443315711809948e-5f;

MCAV_PIL_HD void box_sincos(float h, float& sn, float& cs) {
    const float kf = add_rn(ev::fma_rn(h, SC_TWO_OVER_PI, SC_ROUND), -SC_ROUND);
    float r = ev::fma_rn(kf, -SC_PIO2_HI, h);
    r = ev::fma_rn(kf, -SC_PIO2_MID, r);
    r = ev::fma_rn(kf, -SC_PIO2_LO, r);
    const float z = mul_rn(r, r);
    float p = ev::fma_rn(SC_S3, z, SC_S2);
    p = ev::fma_rn(p, z, SC_S1);
    const float s = ev::fma_rn(mul_rn(r, z), p, r);
    float q = ev::fma_rn(SC_C3, z, SC_C2);
    q = ev::fma_rn(q, z, SC_C1);
    const float c = ev::fma_rn(mul_rn(z, z), q, ev::fma_rn(z, -0.5f, 1.0f));
    const int k = (int)kf & 3;                              // two's complement: -1 & 3 = 3
    sn = k == 0 ? s : k == 1 ? c : k == 2 ? -s : -c;
    cs = k == 0 ? c : k == 1 ? -s : k == 2 ? -c : s;
}

// ---------------------------------------------------------------------------------------------- the prepared box
// What a pair needs of one box, computed once per box: 20 float32, 80 bytes.  px, py: the corners about the box's own centre, counter-
// clockwise from (+dx/2, +dy/2).  An invalid box is all zeros.
struct Prep {
    float cx, cy, zlo, zhi;
    float px[4];
    float py[4];
    float area, vol, r, ok;
    float c, s, hx, hy;
};
static_assert(sizeof(Prep) == 80, "five 16-byte words");

MCAV_PIL_HD Prep prepare(const float* b) {
    Prep p;
    if (!valid(b)) {
        p.cx = p.cy = p.zlo = p.zhi = p.area = p.vol = p.r = p.ok = p.c = p.s = p.hx = p.hy = 0.0f;
        for (int k = 0; k < 4; ++k) p.px[k] = p.py[k] = 0.0f;
        return p;
    }
    box_sincos(b[6], p.s, p.c);
    p.cx = b[0];
    p.cy = b[1];
    p.hx = mul_rn(b[3], 0.5f);
    p.hy = mul_rn(b[4], 0.5f);
    const float hz = mul_rn(b[5], 0.5f);
    p.zlo = add_rn(b[2], -hz);
    p.zhi = add_rn(b[2], hz);
    const float a = mul_rn(p.hx, p.c), bb = mul_rn(p.hy, p.s), d = mul_rn(p.hx, p.s), e = mul_rn(p.hy, p.c);
    p.px[0] = add_rn(a, -bb);
    p.py[0] = add_rn(d, e);
    p.px[3] = add_rn(a, bb);
    p.py[3] = add_rn(d, -e);
    p.px[1] = -p.px[3];
    p.py[1] = -p.py[3];
    p.px[2] = -p.px[0];
    p.py[2] = -p.py[0];
    p.area = mul_rn(b[3], b[4]);
    p.vol = mul_rn(p.area, b[5]);
    p.r = sqrtf(ev::fma_rn(p.hy, p.hy, mul_rn(p.hx, p.hx)));
    p.ok = 1.0f;
    return p;
}

// ---------------------------------------------------------------------------------------------- the intersection
// which side of the line from (q0x, q0y) along (ex, ey) a point lies on: >= 0 is inside (the left of a counter-clockwise edge)
MCAV_PIL_HD float side(float ex, float ey, float q0x, float q0y, float x, float y) {
    return ev::fma_rn(ex, add_rn(y, -q0y), -mul_rn(ey, add_rn(x, -q0x)));
}

// Area of A's quadrilateral inside B's, in A's frame of reference (B's centre minus A's first): Sutherland-Hodgman against B's edges
// 0-1, 1-2, 2-3, 3-0 in that order; a vertex is inside an edge when side >= 0, an edge of the polygon crosses when its ends' sides have
// strictly opposite signs, at t = sp / (sp - sq) from the first end; a vertex beyond the eighth is dropped.  Half the shoelace sum from
// vertex 0, clamped to [0, min(area A, area B)].  +0.0 for an invalid box and when the circle test fails.
MCAV_PIL_HD float inter_bev(const Prep& A, const Prep& B) {
    if (!(A.ok > 0.0f && B.ok > 0.0f)) return 0.0f;
    const float tx = add_rn(B.cx, -A.cx), ty = add_rn(B.cy, -A.cy);
    const float d2 = ev::fma_rn(ty, ty, mul_rn(tx, tx)), rr = add_rn(A.r, B.r);
    if (!(d2 <= mul_rn(mul_rn(rr, rr), CIRCLE_SLACK))) return 0.0f;
    float qx[4], qy[4], x[MAX_VERTS], y[MAX_VERTS], nx[MAX_VERTS], ny[MAX_VERTS], sd[MAX_VERTS];
    for (int k = 0; k < 4; ++k) {
        qx[k] = add_rn(B.px[k], tx);
        qy[k] = add_rn(B.py[k], ty);
        x[k] = A.px[k];
        y[k] = A.py[k];
    }
    int n = 4;
    for (int k = 0; k < 4; ++k) {
        const float q0x = qx[k], q0y = qy[k];
        const float ex = add_rn(qx[(k + 1) & 3], -q0x), ey = add_rn(qy[(k + 1) & 3], -q0y);
        for (int i = 0; i < n; ++i) sd[i] = side(ex, ey, q0x, q0y, x[i], y[i]);
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int h = i == 0 ? n - 1 : i - 1;
            const float sp = sd[h], sq = sd[i];
            if ((sp > 0.0f && sq < 0.0f) || (sp < 0.0f && sq > 0.0f)) {
                const float t = ev::div_rn(sp, add_rn(sp, -sq));
                if (m < MAX_VERTS) {
                    nx[m] = ev::fma_rn(t, add_rn(x[i], -x[h]), x[h]);
                    ny[m] = ev::fma_rn(t, add_rn(y[i], -y[h]), y[h]);
                    ++m;
                }
            }
            if (sq >= 0.0f && m < MAX_VERTS) {
                nx[m] = x[i];
                ny[m] = y[i];
                ++m;
            }
        }
        n = m;
        for (int i = 0; i < n; ++i) {
            x[i] = nx[i];
            y[i] = ny[i];
        }
        if (n < 3) return 0.0f;
    }
    float acc = 0.0f;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        acc = add_rn(acc, ev::fma_rn(x[i], y[j], -mul_rn(x[j], y[i])));
    }
    const float area = mul_rn(acc, 0.5f);
    if (!(area > 0.0f)) return 0.0f;
    return fminf(area, fminf(A.area, B.area));
}

MCAV_PIL_HD float iou_bev(const Prep& A, const Prep& B) {
    const float inter = inter_bev(A, B);
    if (!(inter > 0.0f)) return 0.0f;
    return ev::div_rn(inter, add_rn(add_rn(A.area, B.area), -inter));
}

MCAV_PIL_HD float iou_3d(const Prep& A, const Prep& B) {
    const float inter = inter_bev(A, B);
    if (!(inter > 0.0f)) return 0.0f;
    const float h = add_rn(fminf(A.zhi, B.zhi), -fmaxf(A.zlo, B.zlo));
    if (!(h > 0.0f)) return 0.0f;
    const float i3 = fminf(mul_rn(inter, h), fminf(A.vol, B.vol));          // as the area: never above 1
    if (!(i3 > 0.0f)) return 0.0f;
    return ev::div_rn(i3, add_rn(add_rn(A.vol, B.vol), -i3));
}

MCAV_PIL_HD float iou(const Prep& A, const Prep& B, int mode) { return mode == MODE_3D ? iou_3d(A, B) : iou_bev(A, B); }

// ---------------------------------------------------------------------------------------------- the candidates' order
// A row is a candidate when score >= score_thresh (a NaN is not) and its box is valid.  Ascending order_key is descending score, -0.0
// as +0.0; the candidates are walked by (order_key, anchor index) ascending.  No candidate's key is 0xffffffff (that is a NaN's).
MCAV_PIL_HD bool score_passes(float score, float score_thresh) { return score >= score_thresh; }
MCAV_PIL_HD uint32_t order_key(float score) { return ~ev::float_key(add_rn(score, 0.0f)); }
MCAV_PIL_HD unsigned long long order_pair(uint32_t key, uint32_t index) { return ((unsigned long long)key << 32) | index; }

// ---------------------------------------------------------------------------------------------- the calls' arguments (host)
// Workspace of mcav_box_nms: the images' candidate counts; per image pre_max anchor indices in the order walked, their classes, their
// prepared boxes; and pre_max rows of ceil(pre_max / 64) 64-bit words of the suppression mask.  Each piece rounded up to 256 bytes.
struct Layout {
    size_t count, order, cls, prep, mask, total;
    int words;
};

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline bool layout(int B, long long A, int pre_max, Layout& l) {
    if (B < 1 || B > MAX_IMAGES || A < 1 || pre_max < 1 || pre_max > NMS_MAX_CANDIDATES) return false;
    if ((long long)B * A > 0x7fffffffll) return false;
    const size_t rows = (size_t)B * (size_t)pre_max;
    l.words = (pre_max + 63) / 64;
    l.count = 0;
    l.order = l.count + round_up(sizeof(int) * (size_t)B, 256);
    l.cls = l.order + round_up(sizeof(int) * rows, 256);
    l.prep = l.cls + round_up(sizeof(int) * rows, 256);
    l.mask = l.prep + round_up(sizeof(Prep) * rows, 256);
    l.total = l.mask + round_up(sizeof(unsigned long long) * rows * (size_t)l.words, 256);
    return true;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool mode_ok(int mode) { return mode == MODE_BEV || mode == MODE_3D; }

// 0, or the code mcav_box_iou returns without launching anything
inline int iou_refusal(const float* a, long long na, const float* b, long long nb, int mode, const float* out) {
    if (!a || !b || !out || !mode_ok(mode)) return REFUSED;
    if (na < 0 || nb < 0 || na > MAX_IOU_ROWS || nb > MAX_IOU_ROWS) return REFUSED;
    if (!aligned(a, 4) || !aligned(b, 4) || !aligned(out, 4)) return REFUSED;
    return 0;
}

// 0, or the code mcav_box_nms returns without launching anything
inline int nms_refusal(const float* boxes, const float* scores, const int* classes, int B, long long A, float score_thresh, float iou_thresh,
                       int mode, int pre_max, int post_max, const int* keep, const int* num, const float* out_boxes, const float* out_scores,
                       const void* workspace, size_t workspace_bytes) {
    Layout l;
    if (!boxes || !scores || !keep || !num || !workspace || !mode_ok(mode)) return REFUSED;
    if (!layout(B, A, pre_max, l) || post_max < 1 || post_max > pre_max) return REFUSED;
    if (score_thresh != score_thresh || iou_thresh != iou_thresh) return REFUSED;
    if (!aligned(boxes, 4) || !aligned(scores, 4) || !aligned(classes, 4) || !aligned(keep, 4) || !aligned(num, 4) || !aligned(out_boxes, 4) ||
        !aligned(out_scores, 4) || !aligned(workspace, 16))
        return REFUSED;
    return workspace_bytes < l.total ? SHORT_WORKSPACE : 0;
}

}  // namespace box
}  // namespace mcav
