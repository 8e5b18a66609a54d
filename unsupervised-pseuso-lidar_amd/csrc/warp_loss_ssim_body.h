// The body of the fused SSIM kernels (csrc/warp_loss.hip: warp_loss_ssim_kernel, warp_loss_ssim_stereo_kernel), included INTO each kernel's
// braces, for the reason given in warp_loss_l1_body.h.  In scope there: DBG, MODE and the argument block `a`.
    static_assert(!(DBG && MODE), "the per-pixel dump is a plain-mode diagnostic");
    constexpr bool ST = (MODE & WL_M_STEREO) != 0;
    // stereo: warp 3 samples the stereo frame with depth(tgt) against the target, like warps 0 and 1
    auto twof = [&](int w) { if constexpr (ST) return w == 3 ? stereo_weight(a) : a.tw[w]; else return a.tw[w]; };
    float g0 = 1.0f, g1 = 1.0f;
    if (a.upstream) {
        g0 = a.upstream[0];
        g1 = a.upstream[1];
        if ((a.flags & MCAV_WL_SKIP_IF_UNIT) && g0 == 1.0f && g1 == 1.0f) return;
    }
    __shared__ float sD[WL_LH][LW + 1];
    __shared__ float sX[3][WL_LH][LW + 1];
    __shared__ float sT[3][WL_LH][LW + 1];
    __shared__ __attribute__((aligned(16))) float sC[3][SS_P][SS_P + 1];
    // LDS budget: 52.2 KB = THREE workgroups per CU.  The per-sample constants live where the block reduction's scratch will be (the
    // reduction runs after the last use of the constants), the float64 finalize scratch on top of the coefficient fields (free by then):
    // as separate arrays they added 2.1 KB, 163 KB for three workgroups, and the kernel ran at two per CU (0.62 -> 1.0 ms at 320x1024).
    __shared__ __attribute__((aligned(16))) float s_red_sf[4 * SLAB];
    float (*const sred)[SLAB] = reinterpret_cast<float (*)[SLAB]>(s_red_sf);
    SampleFastOf<MODE>& s_sf = *reinterpret_cast<SampleFastOf<MODE>*>(s_red_sf);
    static_assert(sizeof(SampleFastOf<MODE>) <= sizeof(float) * 4 * SLAB, "constants fit the reduction scratch");
    double (*const s64)[SLAB] = reinterpret_cast<double (*)[SLAB]>(&sC[0][0][0]);
    static_assert(sizeof(double) * (256 / SLAB) * SLAB <= sizeof(float) * 3 * SS_P * (SS_P + 1), "finalize scratch fits the coefficient fields");
    __shared__ int s_flag;
    const int H = a.H, W = a.W, b = blockIdx.z;
    const int bx0 = blockIdx.x * TW, by0 = blockIdx.y * WLH;
    const size_t plane = (size_t)H * W;
    const bool in_depth = (a.flags & MCAV_WL_INPUT_DEPTH) != 0;
    const float* dt = a.disp_t + (size_t)b * plane;
    const float* dr = a.disp_r0 + (size_t)b * plane;
    for (int i = threadIdx.x; i < WL_LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = by0 - HALO + ly, gx = bx0 - HALO + lx;
        float D = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float v = dt[(size_t)gy * W + gx];
            D = in_depth ? v : rcp_nr(fmaf(10.0f, v, 0.01f));
        }
        sD[ly][lx] = D;
    }
    block_prepare(a, b, &s_sf);
    const float* img_t = a.tgt + (size_t)b * 3 * plane;
    const float* img_r0 = a.ref0 + (size_t)b * 3 * plane;
    const float* img_r1 = a.ref1 + (size_t)b * 3 * plane;
    const float* img_st = nullptr;
    if constexpr (ST) img_st = stereo_frame(a) + (size_t)b * 3 * plane;
    const int tx = threadIdx.x & 31, ty0 = threadIdx.x >> 5;
    const int x = bx0 + tx;
    const float invN = 1.0f / (float)((size_t)a.B * 3 * plane);
    const float WS = 0.85f, WL1 = 0.15f;              // losses.py:77
    constexpr int NONE = -(1 << 30);
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
    float dDt[WL_SUB], dDr[WL_SUB], Dr[WL_SUB];
#pragma unroll
    for (int sub = 0; sub < WL_SUB; ++sub) {
        dDt[sub] = 0.f; dDr[sub] = 0.f; Dr[sub] = 0.f;
        const int y = by0 + sub * TH + ty0;
        if (x < W && y < H) {
            const float vr = dr[(size_t)y * W + x];
            Dr[sub] = in_depth ? vr : rcp_nr(fmaf(10.0f, vr, 0.01f));
        }
    }

    if constexpr ((MODE & (WL_M_MIN | WL_M_AUTO)) != 0) {
        constexpr bool AUTO = (MODE & WL_M_AUTO) != 0, MINR = (MODE & WL_M_MIN) != 0;
        __shared__ unsigned char sM[WLH][TW];              // the selection code of the tile's own pixels
        // ---- phase 1: sX <- warp w's warped source (or, ident, its unwarped source) on tile + 2 halo; sT <- its target when with_target
        // stereo: warp w's source picked on the bits of w -- compared with 0 / 1 / 2 / 3 the compiler kept the three plain sources in a scratch
        // table indexed by w
        auto stereo_source = [&](int w) {
            const uintptr_t lo = (w & 1) ? (uintptr_t)img_r1 : (uintptr_t)img_r0, hi = (w & 1) ? (uintptr_t)img_st : (uintptr_t)img_t;
            return reinterpret_cast<const float*>((w & 2) ? hi : lo);
        };
        auto stage = [&](int w, bool ident, bool with_target) {
            const float* src = w == 0 ? img_r0 : (w == 1 ? img_r1 : img_t);
            if constexpr (ST) src = stereo_source(w);
            const float* tar = w == 2 ? img_r1 : img_t;
            const WarpFast wf = lds_warp(s_sf.w[w]);
            for (int i = threadIdx.x; i < WL_LH * LW; i += 256) {
                const int ly = i / LW, lx = i - ly * LW;
                const int gy = by0 - HALO + ly, gx = bx0 - HALO + lx;
                float xv[3] = {0.f, 0.f, 0.f}, tv[3] = {0.f, 0.f, 0.f};
                if (gy >= -1 && gy <= H && gx >= -1 && gx <= W) {
                    const int ry = reflect1(gy, H), rx = reflect1(gx, W);
                    if (ident) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) xv[c] = src[c * plane + (size_t)ry * W + rx];
                    } else {
                        float D;
                        if (ST ? w != 2 : w < 2) D = sD[ry - by0 + HALO][rx - bx0 + HALO];
                        else {
                            const float v = dr[(size_t)ry * W + rx];
                            D = in_depth ? v : rcp_nr(fmaf(10.0f, v, 0.01f));
                        }
                        const FTap t = project_fast(wf, (float)rx, (float)ry, D, H, W);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            float q4[4];
                            texels_of(src + c * plane, W, t, q4);
                            xv[c] = bilinear_lerp(q4[0], q4[1], q4[2], q4[3], t.wx1, t.wy1).v;
                        }
                    }
                    if (with_target) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) tv[c] = tar[c * plane + (size_t)ry * W + rx];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sX[c][ly][lx] = xv[c];
                    if (with_target) sT[c][ly][lx] = tv[c];
                }
            }
            __syncthreads();
        };
        // the staged candidate's error at this thread's statistics pixels (tile + 1 halo), folded into (best, code): it wins only if smaller
        auto fold = [&](float (&best)[SS_K], unsigned& codes, unsigned code, bool first) {
#pragma unroll
            for (int k = 0; k < SS_K; ++k) {
                const int i = threadIdx.x + 256 * k;
                const int py = i / SS_P, px = i - py * SS_P;
                const int gy = by0 - 1 + py, gx = bx0 - 1 + px;
                float e = 0.f;
                if (i < SS_N && gy >= 0 && gy < H && gx >= 0 && gx < W) {
#pragma unroll 1
                    for (int c = 0; c < 3; ++c) {
                        float xw[9], yw[9];
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx) { xw[dy * 3 + dx] = sX[c][py + dy][px + dx]; yw[dy * 3 + dx] = sT[c][py + dy][px + dx]; }
                        e += WS * ssim_point(xw, yw).S + WL1 * fabsf(xw[4] - yw[4]);
                    }
                }
                if (first || e < best[k]) {
                    best[k] = e;
                    codes = (codes & ~(3u << (2 * k))) | (code << (2 * k));
                }
            }
        };
        // phases 2-4 of warp w (staged in sX) with its coefficient fields and L1 term multiplied by the selection (code `mine` of the group);
        // single: the group has no other candidate -- every pixel is kept and the loss is accumulated here, as in the plain kernel
        auto backward = [&](int w, unsigned codes, unsigned mine, bool single, float lw) {
            const float* src = w == 0 ? img_r0 : (w == 1 ? img_r1 : img_t);
            if constexpr (ST) src = stereo_source(w);
            const WarpFast wf = lds_warp(s_sf.w[w]);
            const float gw = g0 * lw;
            float gp0[WL_SUB], gp1[WL_SUB], gp2[WL_SUB], dP[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) dP[i] = 0.f;
#pragma unroll 1
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int k = 0; k < SS_K; ++k) {
                    const int i = threadIdx.x + 256 * k;
                    if (i >= SS_N) continue;
                    const int py = i / SS_P, px = i - py * SS_P;
                    const int gy = by0 - 1 + py, gx = bx0 - 1 + px;
                    SsimPoint o;
                    o.S = 0.f; o.a = 0.f; o.b = 0.f; o.c = 0.f;
                    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                        float xw[9], yw[9];
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx) { xw[dy * 3 + dx] = sX[c][py + dy][px + dx]; yw[dy * 3 + dx] = sT[c][py + dy][px + dx]; }
                        o = ssim_point(xw, yw);
                        if (single) {
                            if (py >= 1 && py <= WLH && px >= 1 && px <= TW) acc[0] += lw * (WS * o.S + WL1 * fabsf(xw[4] - yw[4]));
                        } else if (((codes >> (2 * k)) & 3u) != mine) {
                            o.a = 0.f; o.b = 0.f; o.c = 0.f;
                        }
                    }
                    sC[0][py][px] = o.a; sC[1][py][px] = o.b; sC[2][py][px] = o.c;
                }
                __syncthreads();
#pragma unroll
                for (int sub = 0; sub < WL_SUB; ++sub) {
                    const int ty = sub * TH + ty0, y = by0 + ty;
                    if (c == 0) gp0[sub] = 0.f; else if (c == 1) gp1[sub] = 0.f; else gp2[sub] = 0.f;
                    if (!(x < W && y < H)) continue;
                    float SA = 0.f, SB = 0.f, SC = 0.f;
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) { SA += sC[0][ty + dy][tx + dx]; SB += sC[1][ty + dy][tx + dx]; SC += sC[2][ty + dy][tx + dx]; }
                    if (y == 1 || y == H - 2 || x == 1 || x == W - 2) {      // the reflected windows, as in the plain kernel
                        for (int yi = 0; yi < 3; ++yi) {
                            const int yc = yi == 0 ? y : (yi == 1 ? (y == 1 ? -1 : NONE) : (y == H - 2 ? H : NONE));
                            if (yc == NONE) continue;
                            for (int xi = (yi == 0 ? 1 : 0); xi < 3; ++xi) {
                                const int xc = xi == 0 ? x : (xi == 1 ? (x == 1 ? -1 : NONE) : (x == W - 2 ? W : NONE));
                                if (xc == NONE) continue;
                                for (int dy = -1; dy <= 1; ++dy) {
                                    const int qy = yc + dy;
                                    if (qy < 0 || qy >= H) continue;
                                    for (int dx = -1; dx <= 1; ++dx) {
                                        const int qx = xc + dx;
                                        if (qx < 0 || qx >= W) continue;
                                        SA += sC[0][qy - by0 + 1][qx - bx0 + 1];
                                        SB += sC[1][qy - by0 + 1][qx - bx0 + 1];
                                        SC += sC[2][qy - by0 + 1][qx - bx0 + 1];
                                    }
                                }
                            }
                        }
                    }
                    const float xq = sX[c][ty + HALO][tx + HALO], tq = sT[c][ty + HALO][tx + HALO];
                    const float l1 = (single || sM[ty][tx] == mine) ? WL1 : 0.f;
                    const float gv = gw * (l1 * sgn(xq - tq) + WS * (SA + xq * SB + tq * SC));
                    if (c == 0) gp0[sub] = gv; else if (c == 1) gp1[sub] = gv; else gp2[sub] = gv;
                }
                __syncthreads();
            }
            // ---- phase 4: as in the plain kernel
#pragma unroll
            for (int sub = 0; sub < WL_SUB; ++sub) {
                const int ty = sub * TH + ty0, y = by0 + ty;
                if (!(x < W && y < H)) continue;
                const bool on_tgt = ST ? w != 2 : w < 2;              // (the stereo warp uses depth(tgt))
                const float Dp = on_tgt ? sD[ty + HALO][tx + HALO] : Dr[sub];
                const FTap t = project_fast(wf, (float)x, (float)y, Dp, H, W);
                float gix = 0.f, giy = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float q4[4];
                    texels_of(src + c * plane, W, t, q4);
                    const Sample sm = bilinear_lerp(q4[0], q4[1], q4[2], q4[3], t.wx1, t.wy1);
                    const float gv = c == 0 ? gp0[sub] : (c == 1 ? gp1[sub] : gp2[sub]);
                    gix += gv * sm.dvdx;
                    giy += gv * sm.dvdy;
                }
                const F12 k = lds12(s_sf.Kinv);
                const float fx = (float)x, fy = (float)y;
                const float X[3] = {fmaf(k.v[0], fx, fmaf(k.v[1], fy, k.v[2])) * Dp, fmaf(k.v[3], fx, fmaf(k.v[4], fy, k.v[5])) * Dp,
                                    fmaf(k.v[6], fx, fmaf(k.v[7], fy, k.v[8])) * Dp};
                const float d = backproject_fast(t, X, gix, giy, H, W, dP);
                if (on_tgt) dDt[sub] += d; else dDr[sub] += d;
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) {                       // (w is not a constant here: the running sums are selected, not indexed)
                acc[2 + i] += w == 0 ? dP[i] : 0.f;
                acc[14 + i] += w == 1 ? dP[i] : 0.f;
                acc[26 + i] += w == 2 ? dP[i] : 0.f;
            }
        };
        // one group: candidates, selection (loss, sM, the map), then the backward of every warp in it
        // stereo: the group of the target view is warps {0, 1, 3} -- warp 3 is its third member, with selection code SEL_STEREO
        auto wof = [&](int wfirst, int j) { return (ST && wfirst == 0 && j == 2) ? 3 : wfirst + j; };
        auto cof = [&](int wfirst, int j) { return (ST && wof(wfirst, j) == 3) ? (unsigned)SEL_STEREO : (unsigned)j; };
        auto group = [&](int wfirst, int nw, int plane_out) {
            float lw = 0.f;
            for (int j = 0; j < nw; ++j) lw += (ST ? twof(wof(wfirst, j)) : a.tw[wfirst + j]) * invN;
            const bool single = !AUTO && nw == 1;
            unsigned codes = 0;
            if (!single) {
                float best[SS_K];
                // candidates in tie order: the identities (AUTO), then the reprojections, warp by warp
#pragma unroll 1
                for (int j = 0; j < (AUTO ? 2 : 1) * nw; ++j) {
                    const bool ident = AUTO && j < nw;
                    const int wj = ident ? j : j - (AUTO ? nw : 0);
                    if (j > 0) __syncthreads();                  // the previous candidate's readers are done
                    stage(ST ? wof(wfirst, wj) : wfirst + wj, ident, j == 0);
                    fold(best, codes, ident ? (unsigned)SEL_IDENTITY : (ST ? cof(wfirst, wj) : (unsigned)wj), j == 0);
                }
#pragma unroll
                for (int k = 0; k < SS_K; ++k) {
                    const int i = threadIdx.x + 256 * k;
                    const int py = i / SS_P, px = i - py * SS_P;
                    if (i < SS_N && py >= 1 && py <= WLH && px >= 1 && px <= TW) {
                        sM[py - 1][px - 1] = (unsigned char)((codes >> (2 * k)) & 3u);
                        if (by0 - 1 + py < H && bx0 - 1 + px < W) acc[0] += lw * best[k];
                    }
                }
            } else {
                stage(wfirst, false, true);
                for (int i = threadIdx.x; i < WLH * TW; i += 256) sM[i / TW][i % TW] = 0;
            }
            __syncthreads();
            if (a.sel && plane_out < 2) {
#pragma unroll
                for (int sub = 0; sub < WL_SUB; ++sub) {
                    const int ty = sub * TH + ty0, y = by0 + ty;
                    if (x < W && y < H) a.sel[((size_t)b * 2 + plane_out) * plane + (size_t)y * W + x] = sM[ty][tx];
                }
            }
#pragma unroll 1
            for (int j = nw - 1; j >= 0; --j) {                  // the last candidate staged is the group's last warp
                if (j != nw - 1) stage(ST ? wof(wfirst, j) : wfirst + j, false, false);
                backward(ST ? wof(wfirst, j) : wfirst + j, codes, ST ? cof(wfirst, j) : (unsigned)j, single, lw);
            }
            __syncthreads();                                     // sM / sX are rewritten by the next group
        };
        __syncthreads();                                         // sD is filled
        // groups: min-reprojection {0, 1} -> plane 0, {2} -> plane 1; automask alone {0} -> plane 0, {1} -> not stored, {2} -> plane 1
        // (stereo: min-reprojection {0, 1, 3} -> plane 0; automask alone {3} -> not stored, after {1})
#pragma unroll 1
        for (int gi = 0; gi < (MINR ? 2 : (ST ? 4 : 3)); ++gi) {
            if constexpr (MINR) group(2 * gi, gi == 0 ? (ST ? 3 : 2) : 1, gi);
            else if constexpr (ST) group(gi == 2 ? 3 : (gi == 3 ? 2 : gi), 1, gi == 0 ? 0 : (gi == 3 ? 1 : 2));
            else group(gi, 1, gi == 0 ? 0 : (gi == 1 ? 2 : 1));
        }
    } else {
        // stereo: warps in the order 0, 1, 3, 2 -- warp 3 shares the target planes staged for warps 0 and 1
#pragma unroll
        for (int wi = 0; wi < (ST ? 4 : 3); ++wi) {
            const int w = ST ? (wi == 2 ? 3 : (wi == 3 ? 2 : wi)) : wi;
            const float* src = w == 0 ? img_r0 : (w == 1 ? img_r1 : img_t);
            if constexpr (ST) src = w == 3 ? img_st : src;
            const float* tar = w == 2 ? img_r1 : img_t;
            const bool on_tgt = ST ? w != 2 : w < 2, new_target = ST ? (w == 0 || w == 2) : w != 1;
            const WarpFast wf = lds_warp(s_sf.w[w]);
            const float lw = twof(w) * invN, gw = g0 * lw;
            __syncthreads();                       // sD is filled (w == 0) / the previous warp's readers are done
            // ---- phase 1: warped and target planes on tile + 2 halo
            for (int i = threadIdx.x; i < WL_LH * LW; i += 256) {
                const int ly = i / LW, lx = i - ly * LW;
                const int gy = by0 - HALO + ly, gx = bx0 - HALO + lx;
                float xv[3] = {0.f, 0.f, 0.f}, tv[3] = {0.f, 0.f, 0.f};
                if (gy >= -1 && gy <= H && gx >= -1 && gx <= W) {
                    const int ry = reflect1(gy, H), rx = reflect1(gx, W);
                    float D;
                    if (on_tgt) D = sD[ry - by0 + HALO][rx - bx0 + HALO];
                    else {
                        const float v = dr[(size_t)ry * W + rx];
                        D = in_depth ? v : rcp_nr(fmaf(10.0f, v, 0.01f));
                    }
                    const FTap t = project_fast(wf, (float)rx, (float)ry, D, H, W);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float q4[4];
                        texels_of(src + c * plane, W, t, q4);
                        xv[c] = bilinear_lerp(q4[0], q4[1], q4[2], q4[3], t.wx1, t.wy1).v;
                    }
                    if (new_target) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) tv[c] = tar[c * plane + (size_t)ry * W + rx];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sX[c][ly][lx] = xv[c];
                    if (new_target) sT[c][ly][lx] = tv[c];     // warps 0 and 1 share the target
                }
            }
            __syncthreads();
            float gp0[WL_SUB], gp1[WL_SUB], gp2[WL_SUB];        // d loss / d warped value at the thread's own pixels, per channel
#pragma unroll 1
            for (int c = 0; c < 3; ++c) {
                // ---- phase 2: window statistics -> S and the gradient coefficient fields on tile + 1 halo
                for (int i = threadIdx.x; i < SS_P * SS_P; i += 256) {
                    const int py = i / SS_P, px = i - py * SS_P;
                    const int gy = by0 - 1 + py, gx = bx0 - 1 + px;
                    SsimPoint o;
                    o.S = 0.f; o.a = 0.f; o.b = 0.f; o.c = 0.f;
                    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                        float xw[9], yw[9];
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx) { xw[dy * 3 + dx] = sX[c][py + dy][px + dx]; yw[dy * 3 + dx] = sT[c][py + dy][px + dx]; }
                        o = ssim_point(xw, yw);
                        if (py >= 1 && py <= WLH && px >= 1 && px <= TW) acc[0] += lw * (WS * o.S + WL1 * fabsf(xw[4] - yw[4]));
                    }
                    sC[0][py][px] = o.a; sC[1][py][px] = o.b; sC[2][py][px] = o.c;
                }
                __syncthreads();
                // ---- phase 3: gather the coefficient fields of every window the thread's own pixels take part in
#pragma unroll
                for (int sub = 0; sub < WL_SUB; ++sub) {
                    const int ty = sub * TH + ty0, y = by0 + ty;
                    if (c == 0) gp0[sub] = 0.f; else if (c == 1) gp1[sub] = 0.f; else gp2[sub] = 0.f;
                    if (!(x < W && y < H)) continue;
                    float SA = 0.f, SB = 0.f, SC = 0.f;
                    // the pixel's own 3x3 neighbourhood: always inside the statistics region, zero outside the image
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) { SA += sC[0][ty + dy][tx + dx]; SB += sC[1][ty + dy][tx + dx]; SC += sC[2][ty + dy][tx + dx]; }
                    if (y == 1 || y == H - 2 || x == 1 || x == W - 2) {
                        // one pixel in from the border: the pixel is also the reflection at padded row -1 / H or column -1 / W
                        for (int yi = 0; yi < 3; ++yi) {
                            const int yc = yi == 0 ? y : (yi == 1 ? (y == 1 ? -1 : NONE) : (y == H - 2 ? H : NONE));
                            if (yc == NONE) continue;
                            for (int xi = (yi == 0 ? 1 : 0); xi < 3; ++xi) {
                                const int xc = xi == 0 ? x : (xi == 1 ? (x == 1 ? -1 : NONE) : (x == W - 2 ? W : NONE));
                                if (xc == NONE) continue;
                                for (int dy = -1; dy <= 1; ++dy) {
                                    const int qy = yc + dy;
                                    if (qy < 0 || qy >= H) continue;
                                    for (int dx = -1; dx <= 1; ++dx) {
                                        const int qx = xc + dx;
                                        if (qx < 0 || qx >= W) continue;
                                        SA += sC[0][qy - by0 + 1][qx - bx0 + 1];
                                        SB += sC[1][qy - by0 + 1][qx - bx0 + 1];
                                        SC += sC[2][qy - by0 + 1][qx - bx0 + 1];
                                    }
                                }
                            }
                        }
                    }
                    const float xq = sX[c][ty + HALO][tx + HALO], tq = sT[c][ty + HALO][tx + HALO];
                    const float gv = gw * (WL1 * sgn(xq - tq) + WS * (SA + xq * SB + tq * SC));
                    if (c == 0) gp0[sub] = gv; else if (c == 1) gp1[sub] = gv; else gp2[sub] = gv;
                }
                __syncthreads();                   // sC is rewritten by the next channel
            }
            // ---- phase 4: chain through the bilinear sample to the sampling position, the depth and P
#pragma unroll
            for (int sub = 0; sub < WL_SUB; ++sub) {
                const int ty = sub * TH + ty0, y = by0 + ty;
                if (!(x < W && y < H)) continue;
                const float Dp = on_tgt ? sD[ty + HALO][tx + HALO] : Dr[sub];
                const FTap t = project_fast(wf, (float)x, (float)y, Dp, H, W);
                float gix = 0.f, giy = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float q4[4];
                    texels_of(src + c * plane, W, t, q4);
                    const Sample sm = bilinear_lerp(q4[0], q4[1], q4[2], q4[3], t.wx1, t.wy1);
                    const float gv = c == 0 ? gp0[sub] : (c == 1 ? gp1[sub] : gp2[sub]);
                    gix += gv * sm.dvdx;
                    giy += gv * sm.dvdy;
                }
                const F12 k = lds12(s_sf.Kinv);
                const float fx = (float)x, fy = (float)y;
                const float X[3] = {fmaf(k.v[0], fx, fmaf(k.v[1], fy, k.v[2])) * Dp, fmaf(k.v[3], fx, fmaf(k.v[4], fy, k.v[5])) * Dp,
                                    fmaf(k.v[6], fx, fmaf(k.v[7], fy, k.v[8])) * Dp};
                float d;
                if (ST && w == 3) {                              // the stereo warp: d / d D only (its transform is fixed: no dP)
                    float dc[3];
                    d = backproject_dc(t, gix, giy, H, W, dc);
                } else {
                    d = backproject_fast(t, X, gix, giy, H, W, acc + 2 + 12 * w);
                }
                if (on_tgt) dDt[sub] += d; else dDr[sub] += d;
                if constexpr (DBG) {      // (the residual planes of the dump stay zero: the mix's value-level kinks are judged on the oracle's margins)
                    const float v[WL_DBG] = {t.ix, t.iy, gix, giy, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < WL_DBG; ++k) a.dbg[(((size_t)b * 3 + w) * WL_DBG + k) * plane + (size_t)y * W + x] = v[k];
                }
            }
        }
    }

#pragma unroll
    for (int sub = 0; sub < WL_SUB; ++sub) {
        const int ty = sub * TH + ty0, y = by0 + ty;
        if (!(x < W && y < H)) continue;
        const int cy = ty + HALO, cx = tx + HALO;
        const size_t pix = (size_t)y * W + x;
        const float Dt = sD[cy][cx];
        float d = dDt[sub];
        if (!(a.flags & MCAV_WL_NO_SMOOTH)) {
            const float cxx = 1.0f / (float)((size_t)a.B * H * (W - 2));
            const float cyy = 1.0f / (float)((size_t)a.B * (H - 2) * W);
            const float cxy = 2.0f / (float)((size_t)a.B * (H - 1) * (W - 1));
            float gs = 0.f, ls = 0.f;
            smooth_terms([&](int dy, int dx) { return sD[cy + dy][cx + dx]; }, x, y, H, W, cxx, cyy, cxy, ls, gs);
            acc[1] += ls;
            d += g1 * gs;
        }
        a.d_disp_t[(size_t)b * plane + pix] = in_depth ? d : d * (-10.0f * Dt * Dt);
        a.d_disp_r0[(size_t)b * plane + pix] = in_depth ? dDr[sub] : dDr[sub] * (-10.0f * Dr[sub] * Dr[sub]);
    }
    const int nblk = gridDim.x * gridDim.y;
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    float* const slab = a.slab + ((size_t)b * nblk + blk) * SLAB;
    __syncthreads();                                   // every reader of the constants (and of sC) is done: their LDS is re-used below
    block_reduce_store<NACC, true>(acc, slab, sred);
    if (threadIdx.x >= NACC && threadIdx.x < SLAB) handoff_store(slab + threadIdx.x, 0.f);
    block_finish(a, b, nblk, s64, &s_flag);
