// TEST INFRASTRUCTURE (CPU): drives the per-pixel math of csrc/geom_math.h -- the functions the geometry-consistency kernels
// (csrc/geom_consistency.hip) call -- with plain host loops, in the kernels' arithmetic: fp32 per pixel (no FMA contraction: build with
// -ffp-contract=off), float64 sums, the 64-bit fixed-point scatter, the combine pass.  Single-threaded.  Built by
// tests/test_geom_consistency_cpu.py with g++, as a shared object and, with -DGEOM_HOSTCHECK_MAIN, as a stand-alone program for the
// sanitizers; never loaded by the product.
#include <cstddef>
#include <cstdio>
#include <vector>

#include "geom_math.h"

using namespace mcav;

// disp_t, disp_r0 [B,1,H,W]; poses [B,2,6]; K [B,3,3] float64; flags: 8 = the maps are depths.  Outputs: loss = weight * loss_gc,
// n_out[2], diff_out [B,2,H,W] (-1 where invalid), d_disp_t, d_disp_r0 [B,1,H,W], d_poses [B,2,6] (overwritten).
extern "C" int geom_hostcheck(const float* disp_t, const float* disp_r0, const float* poses, const double* K, int B, int H, int W,
                              unsigned flags, int min_valid, float weight, float upstream, double* loss, double* n_out, float* diff_out,
                              float* d_disp_t, float* d_disp_r0, float* d_poses) {
    if (B <= 0 || H < 2 || W < 2 || min_valid < 0) return -1;
    const bool in_depth = (flags & 8u) != 0;
    const size_t plane = (size_t)H * W;
    std::vector<long long> acc(2 * (size_t)B * plane, 0);
    std::vector<float> direct(2 * (size_t)B * plane, 0.f);
    std::vector<double> dP(2 * (size_t)B * 12, 0.0);
    double n[2] = {0.0, 0.0}, S[2] = {0.0, 0.0};
    for (int d = 0; d < 2; ++d)
        for (int b = 0; b < B; ++b) {
            gc::Dir dir;
            gc::make_dir(K + (size_t)b * 9, poses + (size_t)b * 12, d == 1, dir);
            const float* Da = (d == 0 ? disp_t : disp_r0) + b * plane;
            const float* Db = (d == 0 ? disp_r0 : disp_t) + b * plane;
            auto texel = [&](int i) { return gc::depth_of(Db[i], in_depth); };
            long long* dst = acc.data() + ((size_t)d * B + b) * plane;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const size_t q = (size_t)y * W + x;
                    const float D = gc::depth_of(Da[q], in_depth);
                    const gc::Result r = gc::pixel(dir.wf, x, y, D, H, W, true, texel);
                    diff_out[((size_t)b * 2 + d) * plane + q] = r.p.valid ? r.e.diff : -1.0f;
                    direct[((size_t)d * B + b) * plane + q] = r.dD;
                    if (!r.p.valid) continue;
                    n[d] += 1.0;
                    S[d] += (double)r.e.diff;
                    float X[3], pix[12] = {0};
                    gc::camera_point(dir.Kinv, (float)x, (float)y, D, X);
                    apply_dc(r.dc, 1.0f, X, pix);
                    for (int k = 0; k < 12; ++k) dP[((size_t)b * 2 + d) * 12 + k] += (double)pix[k];
                    for (int j = 0; j < 4; ++j) {
                        const long long f = gc::to_fixed(r.tap[j]);
                        if (f == 0) continue;
                        if (r.idx[j] < 0 || (size_t)r.idx[j] >= plane) return -2;      // a tap with weight outside the image: a bug
                        dst[r.idx[j]] += f;
                    }
                }
        }
    n_out[0] = n[0]; n_out[1] = n[1];
    *loss = (double)weight * 0.5 * (gc::direction_loss(n[0], S[0], min_valid) + gc::direction_loss(n[1], S[1], min_valid));
    const double up = (double)upstream * (double)weight;
    const double kd[2] = {up * gc::direction_scale(n[0], min_valid), up * gc::direction_scale(n[1], min_valid)};
    const bool on[2] = {n[0] > (double)min_valid, n[1] > (double)min_valid};
    for (int m = 0; m < 2; ++m)
        for (int b = 0; b < B; ++b)
            for (size_t i = 0; i < plane; ++i) {
                const float dv = direct[((size_t)m * B + b) * plane + i];
                const float sv = (float)((double)acc[((size_t)(1 - m) * B + b) * plane + i] * gc::FIX_INV);
                float g = (on[m] ? (float)kd[m] * dv : 0.f) + (on[1 - m] ? (float)kd[1 - m] * sv : 0.f);
                if (!in_depth) {
                    const float D = gc::depth_of((m == 0 ? disp_t : disp_r0)[b * plane + i], false);
                    g *= -10.0f * D * D;
                }
                (m == 0 ? d_disp_t : d_disp_r0)[b * plane + i] = g;
            }
    for (int b = 0; b < B; ++b) {
        double g[2][6];
        for (int d = 0; d < 2; ++d) {
            gc::Dir dir;
            gc::make_dir(K + (size_t)b * 9, poses + (size_t)b * 12, d == 1, dir);
            double s[12];
            for (int k = 0; k < 12; ++k) s[k] = on[d] ? kd[d] * dP[((size_t)b * 2 + d) * 12 + k] : 0.0;
            pose_grad_from_dP(s, dir.Kf, poses + (size_t)b * 12, d == 1, g[d]);
        }
        for (int i = 0; i < 6; ++i) {
            d_poses[b * 12 + i] = (float)(g[0][i] + g[1][i]);
            d_poses[b * 12 + 6 + i] = 0.f;
        }
    }
    return 0;
}

#ifdef GEOM_HOSTCHECK_MAIN
// Stand-alone run for -fsanitize=address,undefined: the closed forms, a moving case and a many-to-one case (every tap of the image lands
// in a few texels), on odd sizes.  Exit status 0 = every call returned 0 and the closed forms hold.
static int run_case(int B, int H, int W, float tz, float rot, float dr_scale, int min_valid, double* loss, double* n, float* gmax) {
    const size_t plane = (size_t)H * W;
    std::vector<float> dt(B * plane), dr(B * plane), poses(B * 12, 0.f), diff(2 * B * plane), gt(B * plane), gr(B * plane), gp(B * 12);
    std::vector<double> K(B * 9, 0.0);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
    for (size_t i = 0; i < B * plane; ++i) {
        dt[i] = rot != 0.f || tz != 0.f ? 0.05f + 0.55f * rnd() : 0.3f;
        dr[i] = rot != 0.f || tz != 0.f ? 0.05f + 0.55f * rnd() : 0.3f * dr_scale;
    }
    for (int b = 0; b < B; ++b) {
        // powers of two: K K^-1 = I exactly, so under a zero pose a border pixel projects onto itself and stays valid
        K[b * 9 + 0] = 16.0; K[b * 9 + 2] = 0.5 * (W - 1); K[b * 9 + 4] = 32.0; K[b * 9 + 5] = 0.5 * (H - 1); K[b * 9 + 8] = 1.0;
        poses[b * 12 + 1] = rot; poses[b * 12 + 2] = -rot; poses[b * 12 + 3] = 0.05f * (tz != 0.f); poses[b * 12 + 5] = tz;
    }
    const int rc = geom_hostcheck(dt.data(), dr.data(), poses.data(), K.data(), B, H, W, dr_scale != 1.f && tz == 0.f && rot == 0.f ? 8u : 0u,
                                  min_valid, 1.0f, 1.0f, loss, n, diff.data(), gt.data(), gr.data(), gp.data());
    *gmax = 0.f;
    for (size_t i = 0; i < B * plane; ++i) { *gmax = fmaxf(*gmax, fabsf(gt[i])); *gmax = fmaxf(*gmax, fabsf(gr[i])); }
    for (int i = 0; i < B * 12; ++i) *gmax = fmaxf(*gmax, fabsf(gp[i]));
    return rc;
}

int main() {
    double loss, n[2];
    float g;
    int bad = 0;
    if (run_case(2, 7, 11, 0.f, 0.f, 1.f, 0, &loss, n, &g) != 0 || loss != 0.0 || g != 0.f || n[0] != 154.0 || n[1] != 154.0) { printf("identity case: loss %g g %g n %g %g\n", loss, g, n[0], n[1]); ++bad; }
    if (run_case(2, 7, 11, 0.f, 0.f, 2.f, 0, &loss, n, &g) != 0 || fabs(loss - 1.0 / 3.0) > 1e-4 || n[0] != 154.0 || n[1] != 154.0) { printf("double case: loss %g n %g %g\n", loss, n[0], n[1]); ++bad; }
    if (run_case(2, 7, 11, 0.f, 0.f, 2.f, 1000, &loss, n, &g) != 0 || loss != 0.0 || g != 0.f) { printf("min_valid case: loss %g g %g\n", loss, g); ++bad; }
    if (run_case(2, 23, 37, 0.1f, 0.02f, 1.f, 0, &loss, n, &g) != 0 || !(loss > 0.0) || !(g > 0.f)) { printf("moving case: loss %g g %g\n", loss, g); ++bad; }
    if (run_case(1, 23, 37, 20.f, 0.01f, 1.f, 0, &loss, n, &g) != 0 || !(n[0] > 0.0)) { printf("many-to-one case: loss %g n %g %g\n", loss, n[0], n[1]); ++bad; }
    printf("geom_hostcheck: %s\n", bad ? "FAILED" : "ok");
    return bad;
}
#endif
