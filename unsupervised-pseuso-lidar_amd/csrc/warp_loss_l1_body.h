// The body of the fused L1 kernels (csrc/warp_loss.hip: warp_loss_l1_kernel, warp_loss_l1_stereo_kernel), included INTO each kernel's braces.
// In scope there: DBG, MODE (WL_M_* bits) and the argument block `a` (WLArgs, or WLStereoArgs with WL_M_STEREO).  A shared body in a
// __device__ function would be the plain way; called from the kernels it changed the existing instantiations' code (instruction order), and
// those must stay as they were.  No include guard: included once per kernel.
    static_assert(!(DBG && MODE), "the per-pixel dump is a plain-mode diagnostic");
    constexpr bool MASKED = (MODE & (WL_M_MIN | WL_M_AUTO)) != 0, AUTO = (MODE & WL_M_AUTO) != 0, MINR = (MODE & WL_M_MIN) != 0;
    constexpr bool ST = (MODE & WL_M_STEREO) != 0;
    float g0 = 1.0f, g1 = 1.0f;
    if (a.upstream) {
        g0 = a.upstream[0];
        g1 = a.upstream[1];
        if ((a.flags & MCAV_WL_SKIP_IF_UNIT) && g0 == 1.0f && g1 == 1.0f) return;
    }
    __shared__ SampleFastOf<MODE> s_sf;
    __shared__ float sD[T2LH][LW + 1];
    __shared__ __attribute__((aligned(16))) float sred[RED_N0][RED_LD];
    __shared__ int s_flag;
    const int H = a.H, W = a.W, b = blockIdx.y, tid = threadIdx.x;
    const bool pass1 = (int)blockIdx.x >= a.G0;
    const int g = pass1 ? (int)blockIdx.x - a.G0 : (int)blockIdx.x, G = pass1 ? a.G1 : a.G0;
    const int ntx = (W + TW - 1) / TW, nty = (H + T2H - 1) / T2H, ntiles = ntx * nty;
    const int nmine = (ntiles - g + G - 1) / G;                  // tiles g, g + G, ... of this sample (the host keeps G <= ntiles)
    const float inv_ntx = 1.0f / (float)ntx;
    block_prepare(a, b, &s_sf);

    // Scalar-register budget: only the GATHERED images are buffer resources (a tap outside the image = an out-of-range offset that reads
    // zero); the pixel-aligned reads and the gradient stores are plain global accesses under the pixel's in-image predicate.  With all seven
    // tensors as resources plus three warps' constants the descriptors spilled into vector registers and every load became a waterfall loop.
    const size_t plane = (size_t)H * W;
    const int pb = (int)(plane * sizeof(float));
    const bool in_depth = (a.flags & MCAV_WL_INPUT_DEPTH) != 0;
    const float invN = 1.0f / (float)((size_t)a.B * 3 * plane);
    const int tx = tid & 31, ty0 = tid >> 5;

    // j-th pixel of this thread: tile j >> 1 of the workgroup's list, upper / lower half of its 16 rows
    auto pixel = [&](int j, int& x, int& y, unsigned& off) {
        const int t = g + (j >> 1) * G;
        const int tyi = (int)(((float)t + 0.5f) * inv_ntx), txi = t - tyi * ntx;
        x = txi * TW + tx;
        y = tyi * T2H + (j & 1) * TH + ty0;
        off = ((j >> 1) < nmine && x < W && y < H) ? (unsigned)((y * W + x) * 4) : WL_OOB;
    };
    auto depth_of = [&](float v) { return in_depth ? v : rcp_nr(fmaf(10.0f, v, 0.01f)); };
    struct Set { FTap t; float q[3][4]; };
    auto issue = [&](const WarpFast& wlds, __amdgpu_buffer_rsrc_t src, int x, int y, float D, bool live, Set& s) {
        s.t = project_fast(lds_warp(wlds), (float)x, (float)y, D, H, W, live);
        TapOff f;
        const int base = (s.t.y0 * W + s.t.x0) * 4;
        f.o[0] = s.t.in00 ? (unsigned)base : WL_OOB;
        f.o[1] = s.t.in01 ? (unsigned)(base + 4) : WL_OOB;
        f.o[2] = s.t.in10 ? (unsigned)(base + W * 4) : WL_OOB;
        f.o[3] = s.t.in11 ? (unsigned)(base + W * 4 + 4) : WL_OOB;
        gather_taps(src, f, pb, s.q);
    };
    auto camera_point = [&](int x, int y, float D, float* X) {
        const F12 k = lds12(s_sf.Kinv);
        const float fx = (float)x, fy = (float)y;
        X[0] = fmaf(k.v[0], fx, fmaf(k.v[1], fy, k.v[2])) * D;
        X[1] = fmaf(k.v[3], fx, fmaf(k.v[4], fy, k.v[5])) * D;
        X[2] = fmaf(k.v[6], fx, fmaf(k.v[7], fy, k.v[8])) * D;
    };
    auto dump = [&](int w, unsigned off, const float* v) {
        if (off == WL_OOB) return;
#pragma unroll
        for (int k = 0; k < WL_DBG; ++k) a.dbg[(((size_t)b * 3 + w) * WL_DBG + k) * plane + (off >> 2)] = v[k];
    };
    float acc[RED_N0];
#pragma unroll
    for (int k = 0; k < RED_N0; ++k) acc[k] = 0.f;
    // d loss / d disparity of a pixel is STAGED in LDS and written out every WL_STAGE pixels.  On gfx9-family parts stores share vmcnt with
    // loads and complete out of order with them, so with a store pending every wait for an older load becomes vmcnt(0): one global store per
    // pixel drained the gather pipeline once per pixel (the next unit's gathers, just issued, had to land before the current unit's could be
    // used).  Staged, that full drain happens once per 16 pixels.  The stage borrows the block reduction's scratch (used after the loop).
    static_assert(sizeof(float) * WL_STAGE * 256 <= sizeof(float) * RED_N0 * RED_LD, "gradient stage fits the reduction scratch");
    float* const stage = &sred[0][0];
    static_assert(WL_STAGE * 256 * (sizeof(float) + 1) <= sizeof(float) * RED_N0 * RED_LD, "selection stage fits the reduction scratch");
    unsigned char* const sstage = reinterpret_cast<unsigned char*>(stage + WL_STAGE * 256);      // masked modes: the pixels' selection codes
    auto flush = [&](int j_first, int count, float* dst) {
        for (int k = 0; k < count; ++k) {
            int fx, fy;
            unsigned foff;
            pixel(j_first + k, fx, fy, foff);
            if (foff != WL_OOB) dst[foff >> 2] = stage[k * 256 + tid];
        }
    };
    auto flush_sel = [&](int j_first, int count, int pl) {      // (the optional selection map: plane 0 = warps 0 / 1, plane 1 = warp 2)
        if (!a.sel) return;
        unsigned char* const dst = a.sel + ((size_t)b * 2 + pl) * plane;
        for (int k = 0; k < count; ++k) {
            int fx, fy;
            unsigned foff;
            pixel(j_first + k, fx, fy, foff);
            if (foff != WL_OOB) dst[foff >> 2] = sstage[k * 256 + tid];
        }
    };
    const int npix = 2 * nmine;
    float* const slab = a.slab + ((size_t)b * (a.G0 + a.G1) + blockIdx.x) * SLAB;

    if (!pass1) {
        // ---- pass 0: warps 0 (ref0 -> tgt) and 1 (ref1 -> tgt) with depth(tgt); the smoothness term; d loss / d disp(tgt)
        const float gw0 = g0 * a.tw[0] * invN, gw1 = g0 * a.tw[1] * invN, lw0 = a.tw[0] * invN, lw1 = a.tw[1] * invN;
        const float cxx = 1.0f / (float)((size_t)a.B * H * (W - 2));
        const float cyy = 1.0f / (float)((size_t)a.B * (H - 2) * W);
        const float cxy = 2.0f / (float)((size_t)a.B * (H - 1) * (W - 1));   // dxdy and dydx are the same field
        const bool smooth = !(a.flags & MCAV_WL_NO_SMOOTH);
        const WarpFast &w0 = s_sf.w[0], &w1 = s_sf.w[1];
        const __amdgpu_buffer_rsrc_t rs_r0 = image_rsrc(a.ref0 + (size_t)b * 3 * plane, plane), rs_r1 = image_rsrc(a.ref1 + (size_t)b * 3 * plane, plane);
        // stereo: the fourth warp's constants, term weights and frame (unused, and not instantiated, without WL_M_STEREO)
        const WarpFast& wst = s_sf.w[ST ? 3 : 0];
        float gws = 0.f, lws = 0.f;
        const float* stp = nullptr;
        if constexpr (ST) {
            gws = g0 * stereo_weight(a) * invN;
            lws = stereo_weight(a) * invN;
            stp = stereo_frame(a) + (size_t)b * 3 * plane;
        }
        const float* const dtp = a.disp_t + (size_t)b * plane;
        const float* const tgp = a.tgt + (size_t)b * 3 * plane;
        float* const gtp = a.d_disp_t + (size_t)b * plane;
        auto fetch = [&](unsigned off, float (&v)[4]) {          // disparity and the target's three channels at a pixel (zeros past the image)
            v[0] = v[1] = v[2] = v[3] = 0.f;
            if (off != WL_OOB) {
                const unsigned i = off >> 2;
                v[0] = dtp[i];
#pragma unroll
                for (int c = 0; c < 3; ++c) v[1 + c] = tgp[c * plane + i];
            }
        };
        const float* const r0p = a.ref0 + (size_t)b * 3 * plane;
        const float* const r1p = a.ref1 + (size_t)b * 3 * plane;
        constexpr int NID = ST ? 9 : 6;
        auto fetch_src = [&](unsigned off, float (&v)[NID]) {    // automask: ref0's and ref1's (and the stereo frame's) channels at the pixel
#pragma unroll
            for (int c = 0; c < NID; ++c) v[c] = 0.f;
            if (off != WL_OOB) {
                const unsigned i = off >> 2;
#pragma unroll
                for (int c = 0; c < 3; ++c) { v[c] = r0p[c * plane + i]; v[3 + c] = r1p[c * plane + i]; }
                if constexpr (ST) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[6 + c] = stp[c * plane + i];
                }
            }
        };
        // min-reprojection: warps 0 and 1 (and s) are one term of weight tw[0] + tw[1] (+ tws)
        const float lw01 = ST ? lw0 + lw1 + lws : lw0 + lw1, gw01 = ST ? gw0 + gw1 + gws : gw0 + gw1;
        int x, y, xn, yn;
        unsigned off, offn;
        float cur[4], nxt[4], idn[AUTO ? NID : 1], i0 = 0.f, i1 = 0.f, is = 0.f;      // automask: the current pixel's identity errors
        auto identity = [&](const float* t) {
            i0 = 0.f; i1 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) { i0 += fabsf(idn[c] - t[c]); i1 += fabsf(idn[3 + c] - t[c]); }
            if constexpr (ST) {
                is = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) is += fabsf(idn[6 + c] - t[c]);
            }
        };
        // stereo: the warp's error and its (unweighted) d loss / d D -- no dP: the transform is fixed
        auto stereo_eval = [&](const Set& s, float& e, float& dd) {
            float gx, gy, dc[3];
            warp_eval_fast(s.q, cur + 1, s.t, e, gx, gy);
            dd = backproject_dc(s.t, gx, gy, H, W, dc);
        };
        Set s0, s1, s2;
        pixel(0, x, y, off);
        fetch(off, cur);
        if constexpr (AUTO) { fetch_src(off, idn); identity(cur + 1); }
        float D = depth_of(cur[0]);
        issue(w0, rs_r0, x, y, D, off != WL_OOB, s0);
        for (int j = 0; j < npix; ++j) {
            pixel(j + 1, xn, yn, offn);
            fetch(offn, nxt);                                    // the next pixel's aligned values fly during this pixel's work
            issue(w1, rs_r1, x, y, D, off != WL_OOB, s1);        // warp 1's gathers fly while warp 0 is consumed
            if constexpr (ST) issue(wst, image_rsrc(stp, plane), x, y, D, off != WL_OOB, s2);      // (and the stereo warp's)
            float X[3], dDt = 0.f, labs = 0.f, dbg[DBG ? WL_DBG : 1];
            camera_point(x, y, D, X);
            float Dn;
            if constexpr (AUTO && !MINR) {                       // automask alone: each warp against its own identity error, in the plain order
                const float ic0 = i0, ic1 = i1, ics = is;
                fetch_src(offn, idn);                            // the next pixel's sources fly during this pixel's work
                float e, gx, gy;
                warp_eval_fast(s0.q, cur + 1, s0.t, e, gx, gy);
                const float k0 = e < ic0 ? gw0 : 0.f;
                acc[0] = fmaf(e < ic0 ? e : ic0, lw0, acc[0]);
                sstage[(j & (WL_STAGE - 1)) * 256 + tid] = e < ic0 ? 0 : SEL_IDENTITY;      // (warp 1's choice is not stored)
                dDt += backproject_fast(s0.t, X, gx * k0, gy * k0, H, W, acc + 2);
                Dn = depth_of(nxt[0]);
                issue(w0, rs_r0, xn, yn, Dn, offn != WL_OOB, s0);
                warp_eval_fast(s1.q, cur + 1, s1.t, e, gx, gy);
                const float k1 = e < ic1 ? gw1 : 0.f;
                acc[0] = fmaf(e < ic1 ? e : ic1, lw1, acc[0]);
                dDt += backproject_fast(s1.t, X, gx * k1, gy * k1, H, W, acc + 14);
                if constexpr (ST) {
                    float es, dds;
                    stereo_eval(s2, es, dds);
                    acc[0] = fmaf(es < ics ? es : ics, lws, acc[0]);
                    dDt = fmaf(es < ics ? gws : 0.f, dds, dDt);
                }
            } else if constexpr (MINR) {
                const float ic0 = i0, ic1 = i1, ics = is;
                if constexpr (AUTO) fetch_src(offn, idn);
                float e0, gx0, gy0, e1, gx1, gy1, dc0[3], es = 0.f, dds = 0.f;
                warp_eval_fast(s0.q, cur + 1, s0.t, e0, gx0, gy0);
                const float dd0 = backproject_dc(s0.t, gx0, gy0, H, W, dc0);      // warp 0's derivative is held, unweighted, until warp 1's
                Dn = depth_of(nxt[0]);                                            // error is known
                issue(w0, rs_r0, xn, yn, Dn, offn != WL_OOB, s0);
                if constexpr (ST) stereo_eval(s2, es, dds);                       // (the stereo warp's d / d D is held as well: one float)
                warp_eval_fast(s1.q, cur + 1, s1.t, e1, gx1, gy1);
                // candidates in tie order -- identities (warp 0 first), then reprojections (warp 0 first) -- a later one wins only if smaller
                float m = e0;
                unsigned char code = 0;
                if constexpr (AUTO) {
                    m = ic0;
                    code = SEL_IDENTITY;
                    if (ic1 < m) m = ic1;
                    if constexpr (ST) { if (ics < m) m = ics; }
                    if (e0 < m) { m = e0; code = 0; }
                }
                if (e1 < m) { m = e1; code = 1; }
                if constexpr (ST) { if (es < m) { m = es; code = SEL_STEREO; } }
                acc[0] = fmaf(m, lw01, acc[0]);
                const float k0 = code == 0 ? gw01 : 0.f, k1 = code == 1 ? gw01 : 0.f;
                apply_dc(dc0, k0, X, acc + 2);
                dDt = fmaf(k0, dd0, dDt);
                dDt += backproject_fast(s1.t, X, gx1 * k1, gy1 * k1, H, W, acc + 14);
                if constexpr (ST) dDt = fmaf(code == SEL_STEREO ? gw01 : 0.f, dds, dDt);
                sstage[(j & (WL_STAGE - 1)) * 256 + tid] = code;
            } else {
                warp_unit_fast(s0.q, cur + 1, s0.t, X, H, W, gw0, labs, dDt, acc + 2, DBG ? dbg : nullptr);
                acc[0] = fmaf(labs, lw0, acc[0]);
                if constexpr (DBG) dump(0, off, dbg);
                Dn = depth_of(nxt[0]);
                issue(w0, rs_r0, xn, yn, Dn, offn != WL_OOB, s0);    // the next pixel's warp 0 flies while warp 1 and the smoothness term are worked
                labs = 0.f;
                warp_unit_fast(s1.q, cur + 1, s1.t, X, H, W, gw1, labs, dDt, acc + 14, DBG ? dbg : nullptr);
                acc[0] = fmaf(labs, lw1, acc[0]);
                if constexpr (DBG) dump(1, off, dbg);
                if constexpr (ST) {
                    float es, dds;
                    stereo_eval(s2, es, dds);
                    acc[0] = fmaf(es, lws, acc[0]);
                    dDt = fmaf(gws, dds, dDt);
                }
            }
            if (smooth) {
                if (!(j & 1)) {                                  // first pixel of a tile: publish its depth tile (+ 2 halo)
                    const int by0 = y - ty0, bx0 = x - tx;
                    __syncthreads();                             // the previous tile's readers are done
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        const int i = tid + 256 * m, ly = i / LW, lx = i - ly * LW;
                        const int gy = by0 - HALO + ly, gx = bx0 - HALO + lx;
                        if (i < T2LH * LW) sD[ly][lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? depth_of(dtp[gy * W + gx]) : 0.f;
                    }
                    __syncthreads();
                }
                if (off != WL_OOB) {
                    const int cy = (j & 1) * TH + ty0 + HALO, cx = tx + HALO;
                    float gs = 0.f, ls = 0.f;
                    smooth_terms_sel([&](int dy, int dx) { return sD[cy + dy][cx + dx]; }, x, y, H, W, cxx, cyy, cxy, ls, gs);
                    acc[1] += ls;
                    dDt = fmaf(g1, gs, dDt);
                }
            }
            stage[(j & (WL_STAGE - 1)) * 256 + tid] = in_depth ? dDt : dDt * (-10.0f * D * D);
            if ((j & (WL_STAGE - 1)) == WL_STAGE - 1 || j + 1 == npix) {
                flush(j & ~(WL_STAGE - 1), (j & (WL_STAGE - 1)) + 1, gtp);
                if constexpr (MASKED) flush_sel(j & ~(WL_STAGE - 1), (j & (WL_STAGE - 1)) + 1, 0);
            }
            x = xn; y = yn; off = offn; D = Dn;
#pragma unroll
            for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
            if constexpr (AUTO) identity(cur + 1);
        }
        __syncthreads();                                         // (sD and sred do not alias, but every wavefront must be out of the loop's barriers)
        block_sum_to_slab<RED_N0>(acc, sred, slab, [](int k) { return k; });
        if (tid >= RED_N0 && tid < SLAB) handoff_store(slab + tid, 0.f);      // warp 2's slots
    } else {
        // ---- pass 1: warp 2 (tgt sampled with depth(ref0) and the inverted pose[0], compared with ref1: losses.py:203-207); d loss / d disp(ref0)
        const float gw2 = g0 * a.tw[2] * invN, lw2 = a.tw[2] * invN;
        const WarpFast& w2 = s_sf.w[2];
        const __amdgpu_buffer_rsrc_t rs_t = image_rsrc(a.tgt + (size_t)b * 3 * plane, plane);
        const float* const drp = a.disp_r0 + (size_t)b * plane;
        const float* const r1p = a.ref1 + (size_t)b * 3 * plane;
        float* const grp = a.d_disp_r0 + (size_t)b * plane;
        auto fetch = [&](unsigned off, float (&v)[4]) {          // disparity of ref0 and ref1's three channels at a pixel (zeros past the image)
            v[0] = v[1] = v[2] = v[3] = 0.f;
            if (off != WL_OOB) {
                const unsigned i = off >> 2;
                v[0] = drp[i];
#pragma unroll
                for (int c = 0; c < 3; ++c) v[1 + c] = r1p[c * plane + i];
            }
        };
        const float* const tgp = a.tgt + (size_t)b * 3 * plane;
        auto fetch_src = [&](unsigned off, float (&v)[3]) {      // automask: tgt's channels at the pixel (warp 2's identity error)
            v[0] = v[1] = v[2] = 0.f;
            if (off != WL_OOB) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = tgp[c * plane + (off >> 2)];
            }
        };
        auto identity = [&](const float* iv, const float* cv) {
            float i2 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) i2 += fabsf(iv[c] - cv[c]);
            return i2;
        };
        // automask: warp 2 at one pixel against its identity error i2 -> the selection code; loss and the kept gradient as warp_unit_fast
        auto masked_unit = [&](const Set& s, const float* cv, float i2, const float* X, float& labs, float& dD) -> unsigned char {
            float e, gx, gy;
            warp_eval_fast(s.q, cv, s.t, e, gx, gy);
            const bool keep = e < i2;
            labs += keep ? e : i2;
            const float k = keep ? gw2 : 0.f;
            dD += backproject_fast(s.t, X, gx * k, gy * k, H, W, acc + 1);
            return keep ? 0 : SEL_IDENTITY;
        };
        int xa, ya, xb, yb, xna, yna, xnb, ynb;
        unsigned offa, offb, offna, offnb;
        float ca[4], cb[4], na[4], nb[4], ina[AUTO ? 3 : 1], inb[AUTO ? 3 : 1], i2a = 0.f, i2b = 0.f;
        Set s0, s1;
        pixel(0, xa, ya, offa);
        pixel(1, xb, yb, offb);
        fetch(offa, ca);
        fetch(offb, cb);
        if constexpr (AUTO) {
            fetch_src(offa, ina);
            fetch_src(offb, inb);
            i2a = identity(ina, ca + 1);
            i2b = identity(inb, cb + 1);
        }
        float Da = depth_of(ca[0]), Db = depth_of(cb[0]);
        issue(w2, rs_t, xa, ya, Da, offa != WL_OOB, s0);
        for (int j = 0; j < npix; j += 2) {
            pixel(j + 2, xna, yna, offna);
            pixel(j + 3, xnb, ynb, offnb);
            fetch(offna, na);
            fetch(offnb, nb);
            if constexpr (AUTO) { fetch_src(offna, ina); fetch_src(offnb, inb); }
            issue(w2, rs_t, xb, yb, Db, offb != WL_OOB, s1);
            float X[3], dDr = 0.f, labs = 0.f, dbg[DBG ? WL_DBG : 1];
            camera_point(xa, ya, Da, X);
            if constexpr (AUTO) sstage[(j & (WL_STAGE - 1)) * 256 + tid] = masked_unit(s0, ca + 1, i2a, X, labs, dDr);
            else warp_unit_fast(s0.q, ca + 1, s0.t, X, H, W, gw2, labs, dDr, acc + 1, DBG ? dbg : nullptr);
            if constexpr (MINR && !AUTO) sstage[(j & (WL_STAGE - 1)) * 256 + tid] = 0;
            if constexpr (DBG) dump(2, offa, dbg);
            stage[(j & (WL_STAGE - 1)) * 256 + tid] = in_depth ? dDr : dDr * (-10.0f * Da * Da);
            const float Dna = depth_of(na[0]), Dnb = depth_of(nb[0]);
            issue(w2, rs_t, xna, yna, Dna, offna != WL_OOB, s0);
            dDr = 0.f;
            camera_point(xb, yb, Db, X);
            if constexpr (AUTO) sstage[((j + 1) & (WL_STAGE - 1)) * 256 + tid] = masked_unit(s1, cb + 1, i2b, X, labs, dDr);
            else warp_unit_fast(s1.q, cb + 1, s1.t, X, H, W, gw2, labs, dDr, acc + 1, DBG ? dbg : nullptr);
            if constexpr (MINR && !AUTO) sstage[((j + 1) & (WL_STAGE - 1)) * 256 + tid] = 0;
            if constexpr (DBG) dump(2, offb, dbg);
            stage[((j + 1) & (WL_STAGE - 1)) * 256 + tid] = in_depth ? dDr : dDr * (-10.0f * Db * Db);
            if (((j + 1) & (WL_STAGE - 1)) == WL_STAGE - 1 || j + 2 >= npix) {
                flush(j & ~(WL_STAGE - 1), ((j + 1) & (WL_STAGE - 1)) + 1, grp);
                if constexpr (MASKED) flush_sel(j & ~(WL_STAGE - 1), ((j + 1) & (WL_STAGE - 1)) + 1, 1);
            }
            acc[0] = fmaf(labs, lw2, acc[0]);
            xa = xna; ya = yna; offa = offna; Da = Dna;
            xb = xnb; yb = ynb; offb = offnb; Db = Dnb;
#pragma unroll
            for (int k = 0; k < 4; ++k) { ca[k] = na[k]; cb[k] = nb[k]; }
            if constexpr (AUTO) {
                i2a = identity(ina, ca + 1);
                i2b = identity(inb, cb + 1);
            }
        }
        __syncthreads();                                         // (the stage and sred alias)
        block_sum_to_slab<RED_N1>(acc, sred, slab, [](int k) { return k == 0 ? 0 : 25 + k; });      // loss share; dP of warp 2 -> slots 26..37
        if (tid >= 1 && tid < 26) handoff_store(slab + tid, 0.f);
        if (tid >= 38 && tid < SLAB) handoff_store(slab + tid, 0.f);
    }
    block_finish(a, b, a.G0 + a.G1, reinterpret_cast<double (*)[SLAB]>(&sred[0][0]), &s_flag);
