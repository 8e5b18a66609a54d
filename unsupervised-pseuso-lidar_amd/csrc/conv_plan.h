// The dispatch of the convolution entries, on the host: which kernel family a descriptor takes and with which launch parameters.
// mcav_igemm / mcav_igemm_mtiles / mcav_igemm_route read ONE IgemmRoute; mcav_wgrad / mcav_wgrad_deferred / mcav_wgrad_workspace_bytes /
// mcav_wgrad_uses_bf16 / mcav_wgrad_route read ONE WgradRoute.  plan_igemm and plan_wgrad_route are the only places that spell the order
// in which the families are asked; every family's acceptance test is written here once.
//
// Plain C++17 on include/mcav_conv.h alone (no HIP header, no HIP call): tests/conv_plan_hostcheck compiles it with g++.  The kernels include
// it through conv_gather.h, so the sizes a predicate reads (tile shapes, patch pixels, table capacities) are the kernels' own definitions.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include "../../include/mcav_conv.h"

#ifndef MCAV_OK                 // (include/mcav_depth.h's values)
#define MCAV_OK 0
#define MCAV_E_INVALID (-1)
#endif
#ifndef MCAV_KNOB_INT           // (mcav_common.h's definition: compile-time defaults; -DMCAV_TUNE_ENV experiment builds read the environment)
#ifdef MCAV_TUNE_ENV
#define MCAV_KNOB_INT(name, dflt) ([] { const char* e = getenv(name); return e ? atoi(e) : (dflt); }())
#else
#define MCAV_KNOB_INT(name, dflt) (dflt)
#endif
#endif

namespace mcav {

// ------------------------------------------------------------------------------------------------ sizes shared with the kernels
constexpr int CK = 16;           // K-tile depth: 16 input channels of one filter tap
constexpr int KP = 32;           // pixels per K-tile of the fp32 wgrad GEMM
constexpr int KPB = 64;          // ... of the bf16 wgrad GEMM
constexpr int TAB_TAPS = 32;     // 3x3 filters, the 4x4 stride-2 form of the pooled upsample adjoint, PoseNet's 5x5
constexpr int WG_TABCAP = 2048;
constexpr int HT_H = 8, HT_W = 32;      // conv_halo.hip: output tile
constexpr int ST_TW = 32;               // conv_stem.hip: output tile width (one MFMA row block)
constexpr int ST_TH_DEPTH = 8, ST_TH_POSE = 4;      // ... output rows per tile (StemDepth::TH, StemPose::TH)
constexpr int SW_TH = 4;                // ... output rows per tile of the stem's weight gradient
// patch pixels of the patch-in-LDS kernels, (TH + 2)(TW + 2) <= PIX: 4 x 16 -> 108, 3 x 20 -> 110 (8 x 8 -> 100, 6 x 10 -> 96); 8 x 16 -> 180, 6 x 20 -> 176
constexpr int patch_pix(int tmb) { return tmb == 1 ? 110 : 180; }      // PatchCfg<TMB>::PIX
constexpr int P3_SUBS = 3, P3_PIX = 110;
constexpr int WGP_PIX = 110;
static_assert(P3_PIX == patch_pix(1) && WGP_PIX == patch_pix(1), "the 64-pixel block shape of patch_plan serves every 64-pixel form");

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }
inline int kstride_of(int taps, int Kp) { return round_up(taps * Kp, CK); }

// tile-config ids of mcav_igemm_desc.tile / mcav_wgrad_desc.tile (conv_shared.h's Tile<> aliases; conv_igemm.hip asserts the two agree)
constexpr void tile_dims(int id, int& BM, int& BN) {
    switch (id) {
        case 1: BM = 128; BN = 64; break;
        case 2: BM = 64; BN = 64; break;
        case 3: BM = 256; BN = 32; break;
        case 4: BM = 256; BN = 16; break;
        case 5: BM = 128; BN = 128; break;
        case 7: BM = 128; BN = 32; break;
        case 8: BM = 128; BN = 64; break;
        case 9: BM = 128; BN = 128; break;
        case 10: BM = 64; BN = 64; break;
        case 11: BM = 64; BN = 64; break;
        case 12: BM = 32; BN = 64; break;
        default: BM = 64; BN = 16; break;
    }
}
constexpr int tile_bm(int id) { int BM = 0, BN = 0; tile_dims(id, BM, BN); return BM; }
constexpr int tile_bn(int id) { int BM = 0, BN = 0; tile_dims(id, BM, BN); return BN; }
constexpr int tile_kd(int id) { return (id >= 8 && id <= 10) || id == 12 ? 32 : (id == 11 ? 64 : 16); }      // Tile<>::KD: channels of one tap per K-tile
constexpr int tile_arows(int id) { return tile_bm(id) * tile_kd(id) / 1024; }                                // Tile<>::AROWS: A rows per thread per K-tile

// ------------------------------------------------------------------------------------------------ parameter blocks of the kernels
struct GatherSrc {
    const float* x1;
    const float* x2;
    int B, Hs, Ws, C1, C2, up1;
    int mode, stride, sign, offset, pad_mode;
};

struct IgemmParams {
    GatherSrc g;
    const float* w;
    int kh, kw, Kp, Kstride, taps;
    float* y;
    int Hd, Wd, Cd, n_begin, n_count, y_choff;
    const float* bias;
    int act;
    const float* dact_aux;
    int dact;
    const float* addend;
    int pool;
    float* stats;
    const float *stats_x, *stats_mean, *stats_invstd;      // BatchNorm-backward form of the statistics (mcav_igemm_desc.stats_x)
    int M;           // rows of the GEMM (incl. class / group padding)
    int Mc, McP;     // ADJ_STRIDE2: pixels per parity class and its BM-padded size; groups > 1: rows per group and padded size
    int groups;
    int mtiles, ntiles;
    int no_tab;      // desc.tile bit 8: force the general kernel (A/B timing and parity of both paths)
    const float* wm; // merged-tap filter copy (mcav_pack_weights_upmerge)
    int Np_all;      // packed filter rows (desc.Np)
    int bm;          // rows per tile of the chosen config (UPM row order: tiles of the four classes of one region are adjacent)
    int upm;         // 1: rows are grouped by output parity class and the x1 part of K runs as 4 merged taps on the low-resolution source
    int ksplit;      // > 1: the K loop of a tile is cut into ksplit workgroups (launches of a handful of tiles: PoseNet's 2x5 .. 6x20 maps);
    float* kslab;    //      each writes its raw partial tile to kslab[split] (y-shaped), splitk_finish_kernel sums them and applies the epilogue
};

struct PatchGeo {
    int TH, TW, tiles_y, tiles_x;
    int tmb;      // 32-row blocks per wavefront: 1 = 64-pixel blocks, 2 = 128-pixel blocks
    int refl;     // 0 zero padding; 1 reflection padding, forward (the patch's ring is the mirrored row / column); 2 the ADJOINT of reflection
                  // padding (the zero-padded data gradient plus the ring's contributions folded onto rows / columns 1 and H - 2 / W - 2)
};

struct WgradParams {
    GatherSrc g;
    int kh, kw, Kp, taps, Ktot;   // Ktot = taps * Kp (GEMM rows)
    const float* dy;
    int Hd, Wd, Cdy, dy_choff, Cout;
    int CoutLoad;                  // Cout rounded up to 4 when dy physically has those (zero) channels
    int Mpix;                      // B * Hd * Wd
    int splits, pix_per_split;     // pixel ranges per workgroup (multiple of KP)
    int mtiles, ntiles;
    float* slab;                   // [splits][Ktot + 1][slabN]; row Ktot holds the per-split column sums of dy (bias gradient)
    int slabN;                     // row stride of the slab (Cout rounded up to 16)
    int want_bias;
    int tab_cht_log2;              // wgrad_tab_kernel: log2 of the tiles per table chunk (>= 20: the whole split is one chunk)
    int upm;                       // merged-tap upsample (mcav_wgrad_desc.upm): rows = 16 (class, merged tap) x Kp, pixels = LOW-resolution ones
    int Hf, Wf;                    // upm: full-resolution size of dy (Hd, Wd hold the low-resolution one)
    int split_planes;              // conv_bf16.hip: 1 = the fp32 contraction on three bf16 planes per operand (mcav_wgrad_desc.mma = 2)
    // conv_bf16.hip, wgrad3x3_patch_kernel (patch = 1): pixel blocks of TH x TW (<= 64 pixels) of one image, `bps` consecutive blocks per split,
    // workgroup = (split, 64 input x 64 output channels)
    int patch, pTH, pTW, ptiles_y, ptiles_x, prefl, pnblocks, pbps, pct_co, pnarrow;
};

struct WgradPlan {
    WgradParams p;
    int tile;
    bool use_tab;
    bool use_halo;
    bool use_stem;                 // conv_stem.hip: the 7x7 stride-2 image stem's own weight-gradient kernel
    size_t slab_bytes, pre_bytes;
    int ci_t, groups, per_group;
};

// what the planners take from the machine
struct PlanEnv {
    int cus;      // compute units (patch2_plan counts rounds of one workgroup per CU); 256 where no device answers, which is also the MI355X's
};

struct IgemmRoute {
    int family;            // MCAV_IGEMM_*
    int variant;           // MCAV_RV_* bits: what the family's launch switches on
    int tile;              // tile-config id (the fp32 and bf16 tile families; the id fill_params laid the rows out for elsewhere)
    int mtiles, ntiles;    // rows of the statistics slab; column tiles
    int workgroups;        // of the launch (all launches of a halo route; before the K-split's slab is known to exist: as planned)
    int ksplit;            // fp32 family: the K-split the launch takes if its slab can be allocated (1 = none)
    PatchGeo geo;          // the patch families
    const mcav_igemm_desc* d;      // the descriptor as planned: the caller's, or planar_d where the source is planar and x1 is NULL
    mcav_igemm_desc planar_d;      // ... the caller's with a non-null stand-in for x1 (for the checks; never read)
    IgemmParams p;
};

struct WgradRoute {
    int family;            // MCAV_WGRAD_*
    int variant;
    const mcav_wgrad_desc* d;      // as planned: the caller's, or planar_d (as above)
    mcav_wgrad_desc planar_d;
    WgradPlan pl;
    int workgroups;        // of the launch that writes the slab
    size_t workspace_bytes() const { return pl.slab_bytes + pl.pre_bytes; }
};

// ------------------------------------------------------------------------------------------------ forward / data gradient: fp32 rows
inline int pick_tile(const mcav_igemm_desc* d, long M) {
    if (d->tile) return d->tile;
    if (d->n_count <= 16) return (M >= 256 * 64 && d->kh * d->kw <= 16) ? 4 : 6;      // (a 25-tap table for 256 rows is 26 KB of LDS: 64x16 tiles, 0.071 -> 0.051 ms)
    // 32 output channels: 128x32 tiles (31 KB of LDS with the table, five workgroups per CU) beat 256x32 (56-60 KB, two) on every such
    // launch of the step: 96->32 @96x320 merged-tap forward 0.333 -> 0.289 ms, its pooled adjoint 0.089 -> 0.071, 64->32 @48x160 0.081 -> 0.070
    if (d->n_count <= 32) return 7;
    // The reflection-adjoint kind carries three extra register stages for its border loads: on the 128-row tiles that is 122 VGPRs and two
    // workgroups per CU.  Measured (MI355X, bench.py --layer-report, 96x320 / 48x160 maps): 128x64 0.370 / 0.129 / 0.181 ms, 64x64x32
    // 0.331 / 0.113 / 0.159, 64x64x16 0.300 / 0.100 / 0.154 -- the small maps keep the choices below.  (Re-measured with the reflected sources
    // in tables: 64x64x16 0.265 / 0.078 / 0.131, 128x64 0.274 / 0.080 / 0.134, 64x64x32 0.292 / 0.085 / 0.138.)
    if (d->mode == MCAV_G_ADJ_REFLECT && ((M + 127) / 128) * ((d->n_count + 63) / 64) >= 1024) return 2;
    // measured on MI355X (tools/conv_bench.py): small output tiles with 32-deep K-tiles win at every layer shape of the step --
    // more co-resident workgroups hide the load round trips, and a 32-deep tile halves the barriers per FLOP
    if (d->mode != MCAV_G_SMALLC && ((M + 127) / 128) * ((d->n_count + 63) / 64) >= 1024) return 1;   // many rows (layer1, 48x160): 128x64 tiles, 104 vs 96 TF/s
    // few 64x64 workgroups (layer4's 6x20 maps, M = 2880): 32x64 tiles double them -- 84 -> 104 TF/s on 512->512
    // ... when halving the tiles shortens the longest CU's queue: up to 128 tiles (each half on a CU of its own) or 257..511 (two halves
    // balance better than one whole); in between the halves only pair up on the same CUs (6x20 512->256, 180 tiles: 74 TF/s halved, 87 whole)
    const long t64 = ((M + 63) / 64) * ((d->n_count + 63) / 64);
    if (d->mode != MCAV_G_SMALLC && d->Kp % 32 == 0 && (t64 <= 128 || (t64 > 256 && t64 < 512))) return 12;
    if (d->mode != MCAV_G_SMALLC && d->Kp % 32 == 0) return 10;
    const long t128x64 = ((M + 127) / 128) * ((d->n_count + 63) / 64);
    return t128x64 >= 1024 ? 1 : 2;
}

// a * b * c * e < 2^31 - 1 for positive factors, without overflowing on the way
inline bool bytes_fit_31(long a, long b, long c, long e) {
    const long lim = 0x7fffffffL;
    if (a <= 0 || b <= 0 || c <= 0 || e <= 0) return false;
    if (a >= lim / b) return false;
    a *= b;
    if (a >= lim / c) return false;
    a *= c;
    return a < lim / e;
}

// a * b * c * e < lim, exactly, for positive factors below 2^31 (e: below 2^34): the product is formed in 128 bits, where it cannot overflow
inline bool prod_below(long lim, long a, long b, long c = 1, long e = 1) { return (unsigned __int128)a * b * c * e < (unsigned __int128)lim; }

// The descriptor's checks and the GEMM rows laid out for its tile config (every family launches with these parameters, the patch and bf16
// families for a tile id of their own: plan_igemm overrides d->tile for them).
inline bool fill_params(const mcav_igemm_desc* d, IgemmParams& p, int& tile) {
    if (!d || !d->x1 || !d->w || !d->y) return false;
    if (d->B <= 0 || d->Hs <= 0 || d->Ws <= 0 || d->Hd <= 0 || d->Wd <= 0 || d->C1 <= 0 || d->C2 < 0) return false;
    if (d->C2 > 0 && !d->x2) return false;
    if (d->kh <= 0 || d->kw <= 0 || d->Np <= 0 || d->Kp <= 0 || d->kh > 64 || d->kw > 64 || d->kh * d->kw > 64) return false;
    if (d->n_begin < 0 || d->n_count <= 0 || d->n_begin > d->Np - d->n_count) return false;
    // the destination: channels [y_choff, y_choff + n_count) of a pixel of Cd floats (a launch that ran past Cd would spill into the next pixel)
    if (d->Cd <= 0 || d->y_choff < 0 || d->y_choff > d->Cd - d->n_count) return false;
    if (d->mode == MCAV_G_SMALLC) { if (d->Kp != 4 || d->C1 != 4 || d->C2 != 0) return false; }
    else if (d->Kp % CK != 0 || (long)d->Kp < (long)d->C1 + d->C2) return false;
    if (d->C2 > 0 && (d->C1 % 4 != 0)) return false;
    if (d->mode == MCAV_G_ADJ_REFLECT && (d->kh != 3 || d->kw != 3 || d->Hs != d->Hd || d->Ws != d->Wd || d->Hs < 2 || d->Ws < 2)) return false;
    if (d->pad_mode == MCAV_PAD_REFLECT && (d->Hs < 2 || d->Ws < 2)) return false;
    if (d->up1 && ((d->Hs & 1) || (d->Ws & 1))) return false;
    if (d->pool && ((d->Hd & 1) || (d->Wd & 1) || d->mode == MCAV_G_ADJ_STRIDE2)) return false;
    if (d->pool && d->stats) return false;
    if (d->stats_x && (!d->stats || !d->stats_mean || !d->stats_invstd || d->pool || d->y_choff != 0 || d->n_begin != 0 || d->n_count != d->Cd)) return false;
    // 32-bit byte offsets: the sources, the packed filter ...
    if (!prod_below(0x7fffffffL, d->B, d->Hs, d->Ws, (long)(d->C1 > d->C2 ? d->C1 : d->C2) * 4)) return false;
    const long kstride = ((long)d->kh * d->kw * d->Kp + CK - 1) / CK * CK;
    if (!prod_below(0x7fffffffL, d->Np, kstride, 4)) return false;
    // ... and so has the destination (the pooled one where pool is set): the lean epilogue, the halo and the stem kernels address y -- and
    // dact_aux, addend, stats_x, which share its layout -- through 32-bit byte offsets
    if (!bytes_fit_31((long)d->B, d->pool ? d->Hd >> 1 : d->Hd, d->pool ? d->Wd >> 1 : d->Wd, (long)d->Cd * 4)) return false;
    p.g.x1 = d->x1; p.g.x2 = d->x2; p.g.B = d->B; p.g.Hs = d->Hs; p.g.Ws = d->Ws; p.g.C1 = d->C1; p.g.C2 = d->C2; p.g.up1 = d->up1;
    p.g.mode = d->mode; p.g.stride = d->stride; p.g.sign = d->sign; p.g.offset = d->offset; p.g.pad_mode = d->pad_mode;
    p.w = d->w; p.kh = d->kh; p.kw = d->kw; p.Kp = d->Kp; p.taps = d->kh * d->kw; p.Kstride = kstride_of(p.taps, d->Kp);
    p.y = d->y; p.Hd = d->Hd; p.Wd = d->Wd; p.Cd = d->Cd; p.n_begin = d->n_begin; p.n_count = d->n_count; p.y_choff = d->y_choff;
    p.bias = d->bias; p.act = d->act; p.dact_aux = d->dact_aux; p.dact = d->dact; p.addend = d->addend; p.pool = d->pool; p.stats = d->stats;
    p.stats_x = d->stats ? d->stats_x : nullptr; p.stats_mean = d->stats_mean; p.stats_invstd = d->stats_invstd;
    const long Mlin = (long)d->B * d->Hd * d->Wd;
    p.no_tab = (d->tile >> 8) & 1;
    p.ksplit = 1; p.kslab = nullptr;
    p.wm = d->w_upmerge; p.Np_all = d->Np; p.upm = 0; p.bm = 0;
    tile = pick_tile(d, Mlin) & 0xff;
    if (tile == 0) { mcav_igemm_desc dd = *d; dd.tile = 0; tile = pick_tile(&dd, Mlin); }
    if (((tile >= 8 && tile <= 10) || tile == 12) && (d->mode == MCAV_G_SMALLC || d->Kp % 32 != 0)) return false;      // 32-deep K-tiles need Kp % 32 == 0
    if (tile == 11 && (d->mode == MCAV_G_SMALLC || d->Kp % 64 != 0)) return false;
    int BM, BN;
    tile_dims(tile, BM, BN);
    p.groups = d->groups > 1 ? d->groups : 1;
    if (p.groups > 1) {
        if ((d->mode != MCAV_G_DIRECT && d->mode != MCAV_G_SMALLC) || d->pool || d->B % p.groups != 0) return false;
        p.Mc = (int)(Mlin / p.groups);
        p.McP = round_up(p.Mc, BM);
        p.M = p.groups * p.McP;
    } else if (d->mode == MCAV_G_ADJ_STRIDE2) {
        p.Mc = d->B * ((d->Hd + 1) / 2) * ((d->Wd + 1) / 2);
        p.McP = round_up(p.Mc, BM);
        p.M = 4 * p.McP;
    } else {
        p.Mc = 0; p.McP = 1;
        if (Mlin > 0x7fffffffL) return false;
        p.M = (int)Mlin;
        // merged-tap upsample (see mcav_igemm_desc.w_upmerge): everything the table-driven UPM kernel needs must hold, else the plain path
        const int ck = tile_kd(tile);
        if (d->w_upmerge && d->mode == MCAV_G_DIRECT && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->sign == 1 && d->offset == -1 &&
            d->pad_mode == MCAV_PAD_REFLECT && d->up1 == 1 && d->C2 > 0 && !(d->Hd & 1) && !(d->Wd & 1) && d->Hd == d->Hs && d->Wd == d->Ws &&
            !d->pool && !d->stats && d->C1 % ck == 0 && d->C2 % ck == 0 && d->C1 + d->C2 == d->Kp && (d->C1 & 3) == 0 && !p.no_tab &&
            (long)4 * d->Np * 4 * d->C1 * 4 < 0x7fffffffL) {
            p.upm = 1;
            p.bm = BM;
            p.Mc = d->B * (d->Hd / 2) * (d->Wd / 2);
            p.McP = round_up(p.Mc, BM);
            p.M = 4 * p.McP;
        }
    }
    p.mtiles = (p.M + BM - 1) / BM;
    p.ntiles = (d->n_count + BN - 1) / BN;
    return true;
}

// fp32 family: which kernel launch_igemm<T> starts for the rows of fill_params (a function of the parameters and of the tile's K depth
// and A rows per thread) and the K-split it wants; only the slab of the split is left to the launch.
inline void plan_fp32(IgemmRoute& r) {
    const IgemmParams& p = r.p;
    const int KD = tile_kd(r.tile), AROWS = tile_arows(r.tile);
    const bool c4ok = (p.g.C1 & 3) == 0 && (p.g.C2 & 3) == 0 && (p.g.C2 == 0 || (p.g.C1 & 15) == 0);
    const bool fast_mode = p.g.mode == MCAV_G_DIRECT || (p.g.mode == MCAV_G_ADJ_STRIDE2 && p.g.C2 == 0) || p.g.mode == MCAV_G_SMALLC;
    const bool tab = (p.g.mode == MCAV_G_DIRECT || (p.g.mode == MCAV_G_ADJ_STRIDE2 && p.g.C2 == 0)) && c4ok && p.taps <= TAB_TAPS &&
                     p.g.C1 + p.g.C2 == p.Kp && p.Kp % KD == 0 && (p.g.C2 == 0 || p.g.C1 % KD == 0) && !p.no_tab;
    // (tall tiles put rows of many image lines into one wavefront: most wavefronts would take the border path, so they keep the general kernel)
    const bool tab_refl = p.g.mode == MCAV_G_ADJ_REFLECT && c4ok && p.g.C2 == 0 && p.g.C1 == p.Kp && p.Kp % KD == 0 && !p.no_tab && AROWS <= 2;
    r.family = MCAV_IGEMM_FP32;
    r.ksplit = 1;
    if (p.upm) r.variant = MCAV_RV_TABLE | MCAV_RV_UPM;
    else if (tab) r.variant = MCAV_RV_TABLE;
    else if (tab_refl) r.variant = MCAV_RV_TABLE | MCAV_RV_REFLECT | MCAV_RV_ADJ;
    else if (fast_mode && c4ok) r.variant = MCAV_RV_FAST;
    else if (p.g.mode == MCAV_G_ADJ_REFLECT && c4ok && p.g.C2 == 0) r.variant = MCAV_RV_REFLECT | MCAV_RV_ADJ;
    else r.variant = 0;                                  // the generic kernel
    if (tab && !p.upm) {
        // A handful of tiles with a long K loop (PoseNet conv5-7 and their data gradients: 2 .. 90 tiles of 36 .. 72 K-tiles, one workgroup
        // per CU working through them alone): K is cut over up to 8 workgroups per tile, splitk_finish_kernel sums the partials (fixed order)
        // and applies the epilogue.
        const bool plain = !p.pool && !p.stats && p.groups <= 1 && p.y_choff == 0 && p.n_count == p.Cd && p.n_begin == 0;
        const int tiles = p.mtiles * p.ntiles, ktiles = p.Kp / KD * p.taps;
        static const int enabled = MCAV_KNOB_INT("MCAV_KSPLIT", 1);
        static const int max_tiles = MCAV_KNOB_INT("MCAV_KSPLIT_TILES", 256);
        if (enabled && plain && tiles <= max_tiles && ktiles >= 32) {
            int ksp = 1024 / tiles;
            if (ksp > 8) ksp = 8;
            if (ksp > ktiles / 4) ksp = ktiles / 4;
            if (ksp >= 2) r.ksplit = ksp;
        }
    }
    r.mtiles = p.mtiles; r.ntiles = p.ntiles;
    r.workgroups = p.mtiles * p.ntiles * r.ksplit;
}

// ------------------------------------------------------------------------------------------------ the halo kernels (conv_halo.hip)
// narrow high-resolution 3x3 layers, forward and reflect-adjoint
inline bool plan_halo(const mcav_igemm_desc* d, IgemmRoute& r) {
    if (d->kh != 3 || d->kw != 3 || d->stride != 1) return false;
    if (d->C2 != 0 || d->x2 || (d->C1 != 16 && d->C1 != 32) || d->Kp != d->C1) return false;
    if (d->n_count > 32 || d->stats || d->groups > 1 || d->y_choff != 0) return false;      // wider outputs: the table-driven kernel is faster
    if (d->Hd != d->Hs || d->Wd != d->Ws || d->Hs < 2 || d->Ws < 2) return false;
    if ((d->tile >> 9) & 1) return false;                      // desc.tile bit 9: force the general kernels (A/B timing, parity of both)
    const bool adj = d->mode == MCAV_G_ADJ_REFLECT;
    if (adj) {
        if (d->dact & ~0xff) return false;                     // MCAV_DACT_AFTER_ADDEND and any later flag: the table-driven kernel's epilogue honours them, this one applies act' first
        if (d->up1 || d->bias || d->act != MCAV_ACT_NONE) return false;
        if (d->pool && ((d->Hs & 1) || (d->Ws & 1))) return false;
    } else {
        if (d->mode != MCAV_G_DIRECT || d->sign != 1 || d->offset != -1) return false;
        if (d->n_begin != 0 || d->pool || d->dact_aux || d->addend) return false;
    }
    if (d->n_begin + (d->n_count + 15) / 16 * 16 > d->Np) return false;            // every filter row a launch touches exists in the packed copy
    r.family = MCAV_IGEMM_HALO;
    // upsampled source + reflection padding: 4 merged taps on the low-resolution map (desc.tile bit 10 keeps the 9-tap kernel)
    const bool up = !adj && d->up1 && d->pad_mode == MCAV_PAD_REFLECT && !(d->Hs & 1) && !(d->Ws & 1) && !((d->tile >> 10) & 1);
    r.variant = (adj ? MCAV_RV_ADJ | MCAV_RV_REFLECT : 0) | (up ? MCAV_RV_UPM : 0);
    // 32 input channels x 32 output channels would hold 144 filter registers per lane (one wavefront per SIMD): two launches of 16
    const int nf = (d->n_count > 16 && d->C1 == 16) ? 2 : 1;
    r.ntiles = (d->n_count + 16 * nf - 1) / (16 * nf);       // launches
    r.workgroups = d->B * ((d->Ws + HT_W - 1) / HT_W) * ((d->Hs + HT_H - 1) / HT_H) * r.ntiles;
    return true;
}

// ------------------------------------------------------------------------------------------------ the 7x7 stride-2 stems (conv_stem.hip)
// which stem this forward launch is: 1 = the depth net's image stem (SMALLC, 3 -> 64), 2 = PoseNet conv1 (9 of 16 channels -> 16), 0 = neither
inline int stem_kind(const mcav_igemm_desc* d) {
    if (!d || !d->w_stem || d->kh != 7 || d->kw != 7 || d->stride != 2 || d->sign != 1 || d->offset != -3 || d->C2 != 0 || d->n_begin != 0 ||
        d->pool || d->dact_aux || d->addend || d->y_choff != 0 || ((d->tile >> 9) & 1) || d->pad_mode != MCAV_PAD_ZERO ||
        d->Hd != (d->Hs - 1) / 2 + 1 || d->Wd != (d->Ws - 1) / 2 + 1)
        return 0;
    if (d->mode == MCAV_G_SMALLC && d->C1 == 4 && d->n_count == 64 && d->Np == 64) return 1;
    if (d->mode == MCAV_G_DIRECT && d->C1 == 16 && d->Kp == 16 && d->n_count == 16 && d->Np == 16 && !d->stats && !d->up1) return 2;
    return 0;
}

inline int stem_wgrad_kind(const mcav_wgrad_desc* d) {
    if (!d || d->kh != 7 || d->kw != 7 || d->stride != 2 || d->sign != 1 || d->offset != -3 || d->C2 != 0 || d->upm || ((d->tile >> 9) & 1)) return 0;
    if (d->pad_mode != MCAV_PAD_ZERO || d->up1) return 0;
    if (d->Hd != (d->Hs - 1) / 2 + 1 || d->Wd != (d->Ws - 1) / 2 + 1 || (d->Cdy & 3) || (d->dy_choff & 3)) return 0;
    if (d->mode == MCAV_G_SMALLC && d->C1 == 4 && d->Kp == 4 && d->Cout == 64 && d->Cin == 3 && d->Cdy - d->dy_choff >= 64) return 1;
    if (d->mode == MCAV_G_DIRECT && d->C1 == 16 && d->Kp == 16 && d->Cout == 16 && d->Cin == 9 && d->Cdy - d->dy_choff >= 16) return 2;
    return 0;
}

// the x_planar fields of either descriptor for a launch of stem kind `kind`: 0 = not set, 1 = set and launchable, -1 = refused
// (only the stem kernels read NCHW image sources)
template <class D>
inline int stem_planar_state(const D* d, int kind) {
    if (!d) return 0;
    if (!d->x_planar[0] && !d->x_planar[1] && !d->x_planar[2] && !d->planar_B && !d->planar_stack) return 0;
    if (d->planar_B <= 0 || !d->x_planar[0]) return -1;
    if (kind == 1) {                                      // batch-stacked RGB images
        const int ns = d->B / d->planar_B;
        if (d->planar_stack != 1 || d->B % d->planar_B || ns > 3) return -1;
        for (int i = 0; i < ns; ++i)
            if (!d->x_planar[i]) return -1;
        return 1;
    }
    if (kind == 2) return d->planar_stack == 2 && d->planar_B == d->B && d->x_planar[1] && d->x_planar[2] ? 1 : -1;
    return -1;
}

inline bool plan_stem(const mcav_igemm_desc* d, bool planar, IgemmRoute& r) {
    const int kind = stem_kind(d);
    if (!kind) return false;
    const int th = kind == 1 ? ST_TH_DEPTH : ST_TH_POSE;
    r.family = MCAV_IGEMM_STEM;
    r.mtiles = d->B * ((d->Hd + th - 1) / th) * ((d->Wd + ST_TW - 1) / ST_TW);      // the statistics rows of a tile are image-major: groups need nothing else
    r.ntiles = 1;
    // The split form of the depth stem: measured 0.189 ms against the fp32 kernel's 0.179 (both with the lean epilogue; 24 x 192 x 640): the stem is
    // bound by its patch staging and its 189 MB of output stores, which the split kernel's ONE workgroup per CU (125 KB of LDS) has nothing to
    // overlap with, while its MFMAs take 0.06 instead of 0.10 ms.  OFF under the default mode (mma = 2); mma = 3 (the parity tests) runs it.
    static const int split_on = MCAV_KNOB_INT("MCAV_STEM_SPLIT", 0);
    const bool split = kind == 1 && (d->mma == 3 || (d->mma == 2 && split_on));
    const bool lean = ((d->tile >> 16) & 1) || kind == 2;      // (PoseNet's stem has the lean epilogue only; the split kernel has its own)
    r.variant = (kind == 2 ? MCAV_RV_POSE : 0) | (planar ? MCAV_RV_PLANAR : 0) | (split ? MCAV_RV_SPLIT : 0) | (lean ? MCAV_RV_LEAN : 0);
    r.workgroups = r.mtiles < (split ? 256 : 512) ? r.mtiles : (split ? 256 : 512);      // persistent: 1 (split) / 2 per CU
    return true;
}

// ------------------------------------------------------------------------------------------------ the patch-in-LDS kernels (conv_bf16.hip)
// The block shape for an H x W map: TH TW <= rows, (TH + 2)(TW + 2) <= pix, fewest wasted rows, then the smallest halo; 16-wide blocks read
// the patch without bank conflicts (worth some wasted rows).  Returns the cost (rows computed, weighted).
inline double patch_block(int H, int W, int rows, int pix, int& TH, int& TW) {
    double best = 1e30;
    TH = 4; TW = 16;
    for (int th = 1; th <= 16; ++th)
        for (int tw = 4; tw <= 64; ++tw) {
            if (th * tw > rows || (th + 2) * (tw + 2) > pix) continue;
            const double tiles = (double)((H + th - 1) / th) * ((W + tw - 1) / tw);
            // a lane group = 16 consecutive pixels of the block: one pixel row of a 16-wide block (conflict-free); of a wider block with
            // tw % 4 == 0 at most two runs of a row each (two lanes collide); anything else scatters
            const double bank = tw % 16 == 0 ? 1.0 : (tw > 16 && tw % 4 == 0 ? 1.05 : 1.25);
            const double cost = tiles * rows * (1.0 + 0.05 * (double)((th + 2) * (tw + 2)) / (th * tw)) * bank;
            if (cost < best) { best = cost; TH = th; TW = tw; }
        }
    return best;
}

struct PatchPlan {
    PatchGeo geo;          // conv3x3_patch_kernel's
    int th1, tw1;          // the 64-pixel block shape (the second and the twelve-wavefront form use it whatever geo.tmb is)
};

// true = the descriptor runs on conv3x3_patch_kernel (fills pp): a 3x3 stride-1 zero-padded convolution or its data gradient, one source
inline bool patch_plan(const mcav_igemm_desc* d, PatchPlan& pp, bool f32 = false) {
    PatchGeo& geo = pp.geo;
    static const int enabled = MCAV_KNOB_INT("MCAV_PATCH", 1);
    if (!enabled || !d) return false;
    if (f32 ? (d->mma != 0 || !d->w) : (!d->w16 || d->mma < 1 || d->mma > 3)) return false;
    if (d->kh != 3 || d->kw != 3 || d->stride != 1) return false;
    geo.refl = 0;
    if (d->mode == MCAV_G_DIRECT && d->pad_mode == MCAV_PAD_REFLECT && d->sign == 1 && d->offset == -1) geo.refl = 1;
    else if (d->mode == MCAV_G_ADJ_REFLECT && d->sign == -1 && d->offset == 1) geo.refl = 2;
    else if (d->mode != MCAV_G_DIRECT || d->pad_mode != MCAV_PAD_ZERO) return false;
    else if (!((d->sign == 1 && d->offset == -1) || (d->sign == -1 && d->offset == 1))) return false;
    // reflection padding and its adjoint (the decoder's single-source 3x3 layers; round 4): the split form only
    static const int refl_on = MCAV_KNOB_INT("MCAV_PATCH_REFLECT", 1);
    if (geo.refl && (f32 || d->mma < 2 || !refl_on || d->Hs < 2 || d->Ws < 2)) return false;
    // ... and where it was measured ahead of the fp32 kernels (batch 12, profiles/r04_reflect_patch.txt): 64 outputs or more (half of a 64-wide
    // tile idle: 0.086 against 0.075 ms at 48x160, 64 -> 32), and for the adjoint the 24x80 maps and larger (12x40: level; 6x20, where every block
    // is a border block and runs up to three times the MFMAs: 0.097 against 0.076 ms); mma = 3 (the parity tests) takes it on every shape
    static const int refl_minpix = MCAV_KNOB_INT("MCAV_PATCH_REFLECT_MINPIX", 1000);
    if (geo.refl && d->mma != 3 && (d->n_count < 64 || (geo.refl == 2 && d->Hd * d->Wd < refl_minpix))) return false;
    if (d->C2 != 0 || d->up1 || d->pool || d->w_upmerge) return false;
    if (d->C1 % 32 != 0 || d->Kp != d->C1 || d->Hd != d->Hs || d->Wd != d->Ws || d->n_count < 32) return false;
    if (d->groups > 1 && d->B % d->groups != 0) return false;
    // 128-pixel blocks (half the filter traffic per FLOP) where they waste no more rows than 64-pixel ones and still fill the chip
    static const int force_tmb = MCAV_KNOB_INT("MCAV_PATCH_TMB", 0);
    int th2, tw2;
    const double c1 = patch_block(d->Hd, d->Wd, 64, patch_pix(1), pp.th1, pp.tw1);
    const double c2 = patch_block(d->Hd, d->Wd, 128, patch_pix(2), th2, tw2);
    const long wg2 = (long)d->B * ((d->Hd + th2 - 1) / th2) * ((d->Wd + tw2 - 1) / tw2) * ((d->n_count + 63) / 64);
    geo.tmb = (c2 <= c1 * 1.02 && wg2 >= 1024) ? 2 : 1;
    if (force_tmb == 1 || force_tmb == 2) geo.tmb = force_tmb;
    geo.TH = geo.tmb == 2 ? th2 : pp.th1;
    geo.TW = geo.tmb == 2 ? tw2 : pp.tw1;
    geo.tiles_y = (d->Hd + geo.TH - 1) / geo.TH;
    geo.tiles_x = (d->Wd + geo.TW - 1) / geo.TW;
    // plain bf16 on few blocks (the 6x20 maps): the table-driven 32x64 tiles are faster (0.043 against 0.055 ms on 512 -> 512)
    if (d->mma == 1 && (long)d->B * geo.tiles_y * geo.tiles_x * ((d->n_count + 63) / 64) < 1024) return false;
    return true;
}

// the 64-pixel blocks of pp as a kernel's geometry
inline PatchGeo patch_geo64(const mcav_igemm_desc* d, const PatchPlan& pp) {
    PatchGeo geo = pp.geo;
    geo.TH = pp.th1; geo.TW = pp.tw1; geo.tmb = 1;
    geo.tiles_y = (d->Hd + geo.TH - 1) / geo.TH;
    geo.tiles_x = (d->Wd + geo.TW - 1) / geo.TW;
    return geo;
}

// Twelve-wavefront form (conv3x3_patch3_kernel): three 64-pixel blocks per workgroup, one workgroup per CU.  The split form only; the three
// blocks of a workgroup belong to one statistics group.  MCAV_PATCH3 (tune builds) / the low byte 0x33 of mcav_igemm_desc.tile (tests) select it.
// pp: patch_plan's answer for d (patch = it accepted).
inline bool patch3_plan(const mcav_igemm_desc* d, bool patch, const PatchPlan& pp, PatchGeo& geo) {
    static const int enabled = MCAV_KNOB_INT("MCAV_PATCH3", 0);       // OFF: ahead per launch on the 12x40 / 24x80 maps, level in the step (profiles/r04_patch3.txt)
    static const int min_wgs = MCAV_KNOB_INT("MCAV_PATCH3_MIN_WGS", 192);
    static const int min_k = MCAV_KNOB_INT("MCAV_PATCH3_MIN_K", 128);
    if (d->mma < 2) return false;
    const bool forced = (d->tile & 0xff) == 0x33;
    if ((!enabled && !forced) || !patch) return false;
    geo = patch_geo64(d, pp);
    const long nblk = (long)d->B * geo.tiles_y * geo.tiles_x;
    if (d->groups > 1 && (nblk / d->groups) % P3_SUBS != 0) return false;
    const long wgs = ((nblk + P3_SUBS - 1) / P3_SUBS) * ((d->n_count + 63) / 64);
    // Where it was measured ahead of the first kernel (batch 12, profiles/r04_patch3.txt): 128 or more channels per tap (four or more chunks: a
    // workgroup of two chunks lives for six stages and its set-up and epilogue run alone -- the 48x160 maps: 0.083 -> 0.096 ms) and enough
    // workgroups for one per CU (the 6x20 maps give 128: 0.110 -> 0.117); the 12x40 / 24x80 trunk maps: 0.093 -> 0.079 / 0.085 ms.
    if (!forced && (wgs < min_wgs || d->Kp < min_k)) return false;
    return true;
}

// Second form (conv3x3_patch2_kernel): SB = 4 or 2 sub-blocks of 64 pixels per workgroup, one workgroup per CU; 0 = not this form.  The
// choice is a count of rounds: a launch runs ceil(workgroups / CUs) rounds of SB units of work each, and the fewer sub-blocks win a tie only
// when they save a round (the filter stream per FLOP doubles with them).  A workgroup's sub-blocks must belong to one statistics group.
inline int patch2_plan(const mcav_igemm_desc* d, bool patch, const PatchPlan& pp, const PlanEnv& env, PatchGeo& geo, int& bn) {
    // OFF by default: measured level with or behind the first kernel on every trunk shape (profiles/r04_patch2_forms.txt).
    // mcav_igemm_desc.tile bit 14 selects it (bit 15: its 128 x 32 two-workgroups-per-CU configuration): the parity tests; MCAV_PATCH2=1 in a
    // -DMCAV_TUNE_ENV build: experiments.
    static const int enabled = MCAV_KNOB_INT("MCAV_PATCH2", 0);
    static const int force_sb = MCAV_KNOB_INT("MCAV_PATCH2_SB", 0);
    static const int force_bn = MCAV_KNOB_INT("MCAV_PATCH2_BN", 0);
    if (d->mma < 2) return 0;                                         // (the split form; plain bf16 keeps the first kernel)
    if (!enabled && !((d->tile >> 14) & 3)) return 0;
    if (!patch || pp.geo.refl) return 0;                              // (reflection / its adjoint: the first kernel only)
    geo = patch_geo64(d, pp);
    const long per_img = (long)geo.tiles_y * geo.tiles_x, nblk = d->B * per_img, ntiles = (d->n_count + 63) / 64;
    const int groups = (d->stats && d->groups > 1) ? d->groups : 1;
    const int cus = env.cus;
    auto fits = [&](int sb) { return d->B % groups == 0 && ((d->B / groups) * per_img) % sb == 0; };
    auto cost = [&](int sb) { const long wgs = ((nblk + sb - 1) / sb) * ntiles; return ((wgs + cus - 1) / cus) * sb; };
    int sb = 0;
    if (fits(4)) sb = 4;
    if (fits(2) && (sb == 0 || cost(2) < cost(4))) sb = 2;
    if ((force_sb == 2 || force_sb == 4) && fits(force_sb)) sb = force_sb;
    bn = 64;
    if ((force_bn == 32 || ((d->tile >> 15) & 1)) && fits(2)) { sb = 2; bn = 32; }
    return sb;
}

// The bf16 family's own geometry test -- mcav_igemm_uses_bf16: the host package asks it before the descriptor's stats, w_stem, w_upmerge and
// weight pointers are final and puts the bf16 filter into d->w when it says yes, so a descriptor that passes must never reach an fp32 kernel.
// Returns the bf16 tile id * 2 + k64 (0 = not one the bf16 kernels cover: the fp32 families run it) and sets *refl.  patch = patch_plan(d).
inline int bf16_tile_for(const mcav_igemm_desc* d, bool patch, bool* refl) {
    if (!d || !d->w16 || (d->mma < 1 || d->mma > 3)) return 0;
    // The split form pays where the contraction dominates and the operands are converted once: the patch kernel.  On the table-driven
    // kernels (a conversion per tap) it was measured level with or behind the fp32 MFMA kernels (mma = 3 runs those too: tests).
    if (d->mma == 2 && !patch) return 0;
    if (d->pool || d->w_upmerge) return 0;                            // pooled / merged-tap forms stay on the fp32 kernels
    if ((long)d->kh * d->kw > TAB_TAPS || d->Kp % 32 != 0 || (long)d->C1 + d->C2 != d->Kp) return 0;
    if ((d->C1 & 3) || (d->C2 & 3) || (d->C2 > 0 && d->C1 % 32 != 0)) return 0;
    if (d->n_count < 32) return 0;                                    // narrow outputs: the halo / stencil kernels
    // conv_halo.hip's shapes.  A superset of plan_halo's test on purpose, although plan_igemm asks the halo kernels first: it also covers the
    // descriptors they refuse (stats set, a sub-range, an epilogue they lack), which run the fp32 kernels and must go on doing so.
    if (d->C2 == 0 && d->C1 <= 32 && d->n_count <= 32 && d->kh == 3 && d->stride == 1) return 0;
    const bool direct = d->mode == MCAV_G_DIRECT || (d->mode == MCAV_G_ADJ_STRIDE2 && d->C2 == 0);
    const bool radj = d->mode == MCAV_G_ADJ_REFLECT && d->C2 == 0;
    if (!direct && !radj) return 0;
    *refl = radj;
    const bool k64 = d->mma == 1 && d->Kp % 64 == 0 && (d->C2 == 0 || d->C1 % 64 == 0);      // (the split form keeps 32-deep K-tiles: three planes per panel)
    const long M = (long)d->B * d->Hd * d->Wd;
    const long wg64 = ((M + 63) / 64) * ((d->n_count + 63) / 64);
    int shape = 10;                                                   // 64 x 64
    if (wg64 >= 4096 && !radj) shape = 8;                             // many rows: 128 x 64 (half the filter re-reads)
    else if (wg64 < 512) shape = 12;                                  // few rows (6x20 maps): 32 x 64
    if (d->mma >= 2) {
        static const int forced = MCAV_KNOB_INT("MCAV_SPLIT_TILE", 0);      // tuning knob: 10 / 8 / 12
        if ((forced == 10 || forced == 12 || (forced == 8 && !radj))) shape = forced;
    }
    return shape * 2 + (k64 ? 1 : 0);
}

inline bool igemm_uses_bf16(const mcav_igemm_desc* d) {
    PatchPlan pp;
    bool refl = false;
    return bf16_tile_for(d, d && d->mma == 2 && patch_plan(d, pp), &refl) != 0;      // (only mma = 2 asks for the patch kernel)
}

// the rows of a patch family: fill_params for 64 x 64 tiles (tile 2: fp32 patch, tile 10: bf16), then one row tile per patch block
inline bool patch_rows(const mcav_igemm_desc* d, int tile_id, long blocks, int bn, IgemmRoute& r) {
    mcav_igemm_desc dd = *d;
    dd.tile = tile_id;
    if (!fill_params(&dd, r.p, r.tile)) return false;
    r.p.mtiles = r.mtiles = (int)blocks;                              // rows of the statistics slab = blocks / workgroup rows, image-major (groups = runs of images)
    r.p.ntiles = r.ntiles = (r.p.n_count + bn - 1) / bn;
    r.workgroups = r.mtiles * r.ntiles;
    return true;
}

// fp32 MFMA patch kernel (mma = 0): measured level with the table-driven kernels on the 48x160 / 24x80 maps (0.129 against 0.133 ms, 0.115
// against 0.112) and behind them on the 12x40 / 6x20 maps (ragged 16-wide blocks), so it is OFF by default: MCAV_PATCH_F32=1, or bit 13 of
// mcav_igemm_desc.tile (the parity test), selects it.
inline bool plan_patch_f32(const mcav_igemm_desc* d, IgemmRoute& r) {
    static const int enabled = MCAV_KNOB_INT("MCAV_PATCH_F32", 0);
    if (!enabled && !((d->tile >> 13) & 1)) return false;
    PatchPlan pp;
    if (!patch_plan(d, pp, true)) return false;
    r.geo = pp.geo;
    if (!patch_rows(d, 2, (long)d->B * r.geo.tiles_y * r.geo.tiles_x, 64, r)) return false;
    r.family = MCAV_IGEMM_PATCH_F32;
    r.variant = r.geo.tmb == 2 ? MCAV_RV_TMB2 : 0;
    return true;
}

// The bf16 MFMA kernels where the launch qualifies: 1 = not eligible (the fp32 family runs it), else MCAV_OK / MCAV_E_INVALID.  Past
// bf16_tile_for the caller may have put the bf16 copy into d->w as well: never fall through to the fp32 kernels.
inline int plan_bf16(const mcav_igemm_desc* d, const PlanEnv& env, IgemmRoute& r) {
    PatchPlan pp;
    const bool patch = patch_plan(d, pp);
    bool refl = false;
    const int bt = bf16_tile_for(d, patch, &refl);
    if (!bt) return 1;
    const bool split = d->mma >= 2;
    int bn2 = 64;
    bool ok;
    if (patch3_plan(d, patch, pp, r.geo)) {
        const long nblk = (long)d->B * r.geo.tiles_y * r.geo.tiles_x;
        ok = patch_rows(d, 10, (nblk + P3_SUBS - 1) / P3_SUBS, 64, r);      // a workgroup = three blocks of one group
        r.family = MCAV_IGEMM_BF16_PATCH3;
        r.variant = MCAV_RV_SPLIT | (r.geo.refl == 2 ? MCAV_RV_ADJ | MCAV_RV_REFLECT : r.geo.refl == 1 ? MCAV_RV_REFLECT : 0);
    } else if (const int sb = patch2_plan(d, patch, pp, env, r.geo, bn2)) {
        const long nblk = (long)d->B * r.geo.tiles_y * r.geo.tiles_x;
        ok = patch_rows(d, 10, (nblk + sb - 1) / sb, bn2, r);
        r.family = MCAV_IGEMM_BF16_PATCH2;
        r.variant = MCAV_RV_SPLIT | (sb == 4 ? MCAV_RV_SB4 : 0) | (bn2 == 32 ? MCAV_RV_BN32 : 0);
    } else if (patch) {
        r.geo = pp.geo;
        ok = patch_rows(d, 10, (long)d->B * r.geo.tiles_y * r.geo.tiles_x, 64, r);
        r.family = MCAV_IGEMM_BF16_PATCH;
        r.variant = (split ? MCAV_RV_SPLIT : 0) | (r.geo.tmb == 2 ? MCAV_RV_TMB2 : 0) | (r.geo.refl == 2 ? MCAV_RV_ADJ | MCAV_RV_REFLECT : r.geo.refl == 1 ? MCAV_RV_REFLECT : 0);
    } else {
        mcav_igemm_desc dd = *d;
        dd.tile = bt >> 1;                                            // the fp32 planner lays the rows out for these tile dimensions
        ok = fill_params(&dd, r.p, r.tile) && (r.tile == 8 || r.tile == 10 || r.tile == 12);
        r.family = MCAV_IGEMM_BF16_TILE;
        r.variant = (split ? MCAV_RV_SPLIT : 0) | ((bt & 1) ? MCAV_RV_K64 : 0) | (refl ? MCAV_RV_ADJ | MCAV_RV_REFLECT : 0);
        r.mtiles = r.p.mtiles; r.ntiles = r.p.ntiles;
        r.workgroups = r.mtiles * r.ntiles;
    }
    if (!ok) return MCAV_E_INVALID;
    if ((long)d->Np * r.p.Kstride * 2 * (split ? 3 : 1) >= 0x7fffffffL) return MCAV_E_INVALID;      // the bf16 filter (three planes: split form) in 32-bit byte offsets
    return MCAV_OK;
}

// ------------------------------------------------------------------------------------------------ forward / data gradient: the one cascade
// Order matters where two families accept the same descriptor:
//   planar sources   only the stem kernels read them: asked alone;
//   halo             before everything else: its shapes are excluded from the bf16 test by hand, and it beats the fp32 table kernels on them;
//   stem             7x7 stride 2 with w_stem: no other family's shapes, asked before the opt-in kernels so a forced bit cannot take it;
//   fp32 patch       opt-in (tile bit 13 / MCAV_PATCH_F32), mma = 0 only: before the bf16 test, which needs mma != 0;
//   bf16             twelve-wavefront form, second form (both opt-in), the patch kernel, then the table tiles;
//   fp32             everything else.
// `halo` = false plans as if the halo kernels had declined (see below).
inline int plan_igemm(const mcav_igemm_desc* d, const PlanEnv& env, IgemmRoute& r, bool halo = true) {
    r.family = MCAV_IGEMM_FP32; r.variant = r.tile = r.mtiles = r.ntiles = r.workgroups = 0; r.ksplit = 1; r.geo = PatchGeo{};
    const int planar = stem_planar_state(d, stem_kind(d));      // NCHW image sources: only the two stem kernels read them (x1 may then be NULL)
    if (planar < 0) return MCAV_E_INVALID;
    if (planar && !d->x1) { r.planar_d = *d; r.planar_d.x1 = d->x_planar[0]; d = &r.planar_d; }
    r.d = d;
    if (!fill_params(d, r.p, r.tile)) return MCAV_E_INVALID;
    r.mtiles = r.p.mtiles; r.ntiles = r.p.ntiles;
    if (planar) return plan_stem(d, true, r) ? MCAV_OK : MCAV_E_INVALID;
    if (halo && plan_halo(d, r)) {
        // The halo kernels write no statistics slab, and the host package sizes a slab BEFORE it sets `stats` (which they refuse): a halo
        // route reports the rows of the launch that runs once they decline.
        IgemmRoute next;
        r.mtiles = plan_igemm(d, env, next, false) == MCAV_OK ? next.mtiles : r.p.mtiles;
        return MCAV_OK;
    }
    if (plan_stem(d, false, r)) return MCAV_OK;
    if (plan_patch_f32(d, r)) return MCAV_OK;
    if (d->mma != 0) {
        const int rc = plan_bf16(d, env, r);
        if (rc != 1) return rc;
    }
    plan_fp32(r);
    return MCAV_OK;
}

// ------------------------------------------------------------------------------------------------ weight gradient
// narrow high-resolution layers: conv_halo.hip writes the slab partials.  0 = not applicable, else the number of slab partials (= workgroups)
inline int halo_wgrad_splits(const mcav_wgrad_desc* d) {
    if (d->mode != MCAV_G_DIRECT || d->kh != 3 || d->kw != 3 || d->stride != 1 || d->sign != 1 || d->offset != -1) return 0;
    if (d->C2 != 0 || d->x2 || (d->C1 != 16 && d->C1 != 32) || d->Kp != d->C1 || d->Cin != d->C1) return 0;
    if (d->Cout > 32 || (d->C1 == 32 && d->Cout > 16)) return 0;
    if (d->Hd != d->Hs || d->Wd != d->Ws || d->Hs < 2 || d->Ws < 2) return 0;
    if ((d->Cdy & 3) || (d->dy_choff & 3) || ((d->tile >> 9) & 1)) return 0;
    const int cl = (d->Cout + 3) / 4 * 4;
    if (cl > d->Cdy - d->dy_choff) return 0;                 // the 16-byte dy loads need the (zero) padding channels to exist
    const long tiles = (long)d->B * ((d->Hs + HT_H - 1) / HT_H) * ((d->Ws + HT_W - 1) / HT_W);
    return (int)(tiles < 512 ? tiles : 512);
}

// the image stem: conv_stem.hip writes the slab partials.  0 = not applicable, else the number of slab partials (= persistent workgroups)
inline int stem_wgrad_splits(const mcav_wgrad_desc* d) {
    if (!stem_wgrad_kind(d)) return 0;
    const long tiles = (long)d->B * ((d->Hd + SW_TH - 1) / SW_TH) * ((d->Wd + ST_TW - 1) / ST_TW);
    return (int)(tiles < 512 ? tiles : 512);
}

// mcav_wgrad_desc.dy_bn_*: 0 = not set (all zero), 1 = set and launchable (the depth stem, no bias gradient), -1 = set and refused
// (only the depth stem's kernel folds a BatchNorm backward into its dy tile)
inline int stem_wgrad_bn(const mcav_wgrad_desc* d) {
    if (!d) return 0;
    if (!d->dy_bn_x && !d->dy_bn_gamma && !d->dy_bn_mean && !d->dy_bn_invstd && !d->dy_bn_sums && !d->dy_bn_groups && d->dy_bn_inv_count == 0.f) return 0;
    if (stem_wgrad_kind(d) != 1 || d->dbias) return -1;      // (conv1 has no bias)
    if (d->dy_choff != 0 || d->Cdy != 64) return -1;         // the coefficients are indexed by dy's own channel: dy and c1 are exactly the 64 channels
    if (!d->dy_bn_x || !d->dy_bn_gamma || !d->dy_bn_mean || !d->dy_bn_invstd || !d->dy_bn_sums) return -1;
    if (d->dy_bn_groups < 1 || d->B % d->dy_bn_groups || !(d->dy_bn_inv_count > 0.f)) return -1;
    return 1;
}

// Pixel splits that fill whole generations of resident workgroups: 1044 workgroups on 1024 slots (128->128 at 24x80 with "about 1024") run
// a second generation for 2 % of the work (0.142 ms; 0.124 at twice the splits).  The fewest splits, from one generation's worth up to three,
// whose workgroup count fills its last generation to 95 % (else the best fill).  ktile: pixels per K-tile (a split is a whole number of them).
inline int wgrad_fill_splits(int Mpix, int out_tiles, int slots, int max_splits, int ktile) {
    auto wgs_of = [&](int sp) {
        const int pps = round_up((Mpix + sp - 1) / sp, ktile);
        return out_tiles * ((Mpix + pps - 1) / pps);
    };
    int lo = slots / out_tiles, hi = 3 * slots / out_tiles + 1;
    if (lo < 1) lo = 1;
    if (lo > max_splits) lo = max_splits;
    if (hi > max_splits) hi = max_splits;
    int splits = lo;
    double best = -1.0;
    for (int sp = lo; sp <= hi; ++sp) {
        const int w = wgs_of(sp), gens = (w + slots - 1) / slots;
        const double fill = (double)w / ((double)gens * slots);
        if (fill > best + 1e-9) { best = fill; splits = sp; }
        if (fill >= 0.95) { splits = sp; break; }
    }
    return splits;
}

// the slab [splits][Ktot + 1][slabN] and, above 8 splits, the pre-sums of the two-level reduction
inline void wgrad_slab_sizes(WgradPlan& pl) {
    const WgradParams& p = pl.p;
    auto align256 = [](size_t v) { return (v + 255) / 256 * 256; };
    pl.slab_bytes = align256(sizeof(float) * (size_t)p.splits * (p.Ktot + 1) * p.slabN);
    pl.groups = p.splits > 8 ? 8 : 0;
    pl.per_group = pl.groups ? (p.splits + pl.groups - 1) / pl.groups : 0;
    if (pl.groups) pl.groups = (p.splits + pl.per_group - 1) / pl.per_group;
    pl.pre_bytes = align256(sizeof(float) * (size_t)pl.groups * (p.Ktot + 1) * p.slabN);
}

// The descriptor's checks, the slab GEMM of the fp32 kernels (tile, splits, table chunking) and which of them writes the slab: the halo or
// stem kernel where the layer is one of theirs (they replace the GEMM, never its reduction), else wgrad_tab_kernel / wgrad_kernel.
inline bool plan_wgrad(const mcav_wgrad_desc* d, WgradPlan& pl) {
    if (!d || !d->x1 || !d->dy || !d->dw_oihw) return false;
    if (d->B <= 0 || d->Hs <= 0 || d->Ws <= 0 || d->Hd <= 0 || d->Wd <= 0 || d->C1 <= 0 || d->C2 < 0 || d->Cout <= 0 || d->Cin <= 0) return false;
    if (d->C2 > 0 && (!d->x2 || d->C1 % 4 != 0)) return false;
    if (d->mode != MCAV_G_DIRECT && d->mode != MCAV_G_SMALLC) return false;
    if (d->mode == MCAV_G_SMALLC && (d->Kp != 4 || d->C1 != 4 || d->C2 != 0)) return false;
    if (d->mode == MCAV_G_DIRECT && (d->Kp % CK != 0 || (long)d->Kp < (long)d->C1 + d->C2)) return false;
    if (d->Cin > d->Kp) return false;
    if (d->kh <= 0 || d->kw <= 0) return false;
    if (d->Cdy <= 0 || d->dy_choff < 0 || d->dy_choff > d->Cdy - d->Cout) return false;      // channels [dy_choff, dy_choff + Cout) of dy exist
    if (d->ci_offset < 0 || d->ci_offset > (d->Cin_total > 0 ? d->Cin_total : d->Cin) - d->Cin) return false;      // the launch's input-channel window lies inside the OIHW gradient
    // More than 480 taps have no reduce kernel (ci_t below); the GEMM's Ktot rows, rounded up to a tile, in an int.  Both are refused here,
    // before a product can overflow.
    if (!prod_below(481, d->kh, d->kw) || !prod_below(0x7fffffffL - 256, (long)d->kh * d->kw, d->Kp)) return false;
    // B * Hd * Wd rows in an int; the sources and dy in 32-bit byte offsets
    if (!prod_below(0x80000000L, d->B, d->Hd, d->Wd)) return false;
    const long M = (long)d->B * d->Hd * d->Wd;
    if (!prod_below(0x7fffffffL, d->B, d->Hs, d->Ws, (long)(d->C1 > d->C2 ? d->C1 : d->C2) * 4) || !prod_below(0x7fffffffL, M, d->Cdy, 4)) return false;
    WgradParams& p = pl.p;
    p.g.x1 = d->x1; p.g.x2 = d->x2; p.g.B = d->B; p.g.Hs = d->Hs; p.g.Ws = d->Ws; p.g.C1 = d->C1; p.g.C2 = d->C2; p.g.up1 = d->up1;
    p.g.mode = d->mode; p.g.stride = d->stride; p.g.sign = d->sign; p.g.offset = d->offset; p.g.pad_mode = d->pad_mode;
    p.kh = d->kh; p.kw = d->kw; p.Kp = d->Kp; p.taps = d->kh * d->kw; p.Ktot = p.taps * d->Kp;
    p.dy = d->dy; p.Hd = d->Hd; p.Wd = d->Wd; p.Cdy = d->Cdy; p.dy_choff = d->dy_choff; p.Cout = d->Cout;
    p.CoutLoad = round_up(d->Cout, 4) <= d->Cdy - d->dy_choff ? round_up(d->Cout, 4) : d->Cout;
    p.Mpix = (int)M;
    p.slabN = round_up(d->Cout, 16);
    p.upm = 0; p.Hf = d->Hd; p.Wf = d->Wd; p.patch = 0; p.split_planes = 0;
    if (d->upm) {      // merged-tap upsample half: 16 (class, merged tap) x Kp rows, reduction over the low-resolution pixels
        if (d->mode != MCAV_G_DIRECT || d->kh != 3 || d->kw != 3 || d->stride != 1 || d->sign != 1 || d->offset != -1 || d->pad_mode != MCAV_PAD_REFLECT ||
            !d->up1 || d->C2 != 0 || d->Hd != d->Hs || d->Wd != d->Ws || (d->Hd & 1) || (d->Wd & 1) || d->dbias || d->Kp != d->C1 || (d->C1 & 15) ||
            (d->Cdy & 3) || (d->dy_choff & 3) || (p.CoutLoad & 3))
            return false;
        p.upm = 1;
        p.taps = 16; p.Ktot = 16 * d->Kp;
        p.Hd = d->Hd / 2; p.Wd = d->Wd / 2;
        p.Mpix = d->B * p.Hd * p.Wd;
    }
    int tile = d->tile & 0xff;
    if (!tile) {
        if (d->Cout <= 16) tile = round_up(p.Ktot, 64) < round_up(p.Ktot, 256) ? 6 : 4;
        else if (d->Cout <= 32) tile = 7;      // 128x32 (48 KB of LDS, three workgroups per CU; 256x32 needs 80 KB): 16x25 -> 32 0.052 -> 0.044 ms
        else tile = 2;            // 64x64 beats 128x64 on every layer shape of the step (tools/conv_bench.py wgrad)
    }
    if (p.upm) tile = d->Cout <= 16 ? 6 : 2;                     // 64-row tiles: a row tile never straddles a parity class (4 Kp rows each)
    if (tile != 1 && tile != 2 && tile != 3 && tile != 4 && tile != 6 && tile != 7) return false;
    pl.tile = tile;
    int BM, BN;
    tile_dims(tile, BM, BN);
    p.mtiles = (p.Ktot + BM - 1) / BM;
    p.ntiles = (d->Cout + BN - 1) / BN;
    const int out_tiles = p.mtiles * p.ntiles;
    static const int target_wgs = MCAV_KNOB_INT("MCAV_WGRAD_TARGET_WGS", 0);
    int max_splits = (p.Mpix + 8 * KP - 1) / (8 * KP);           // at least 8 K-tiles each
    if (max_splits > 512) max_splits = 512;
    if (max_splits < 1) max_splits = 1;
    int splits;
    if (target_wgs > 0) {                                        // tuning knob: aim at that many workgroups
        splits = (target_wgs + out_tiles - 1) / out_tiles;
    } else {
        const int occ = tile == 2 ? 4 : (tile == 7 ? 3 : (tile == 6 ? 4 : 2));      // resident workgroups per CU
        splits = wgrad_fill_splits(p.Mpix, out_tiles, 256 * occ, max_splits, KP);
    }
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    p.pix_per_split = round_up((p.Mpix + splits - 1) / splits, KP);
    // table-driven kernel: the per-workgroup offset table (pixels of a split x taps touched by a row tile x sources) must fit
    pl.use_tab = false;
    const int wave_ch = BM / 4;
    const bool fast = d->mode == MCAV_G_DIRECT && (d->C1 & 3) == 0 && (d->C2 & 3) == 0 && (d->C2 == 0 || d->C1 % wave_ch == 0) &&
                      (p.CoutLoad & 3) == 0 && (d->Cdy & 3) == 0 && (d->dy_choff & 3) == 0 && !((d->tile >> 8) & 1);
    p.tab_cht_log2 = 20;
    if (fast) {
        int ntmax = 1;
        for (int mt = 0; mt < p.mtiles; ++mt) {
            const int lo = mt * BM / d->Kp, hi = (mt * BM + BM - 1) / d->Kp < p.taps - 1 ? (mt * BM + BM - 1) / d->Kp : p.taps - 1;
            if (hi - lo + 1 > ntmax) ntmax = hi - lo + 1;
        }
        const int epp = p.upm ? ntmax + 1 : ntmax * (d->C2 > 0 ? 2 : 1);  // table entries per pixel (upm: + the dy offset)
        if ((long)p.pix_per_split * epp <= WG_TABCAP) {
            pl.use_tab = true;                                            // one chunk
        } else if (epp <= 16) {
            int lg = 2;                                                   // two half-buffers of 2^lg tiles: 2^lg * KP * epp <= WG_TABCAP / 2
            while ((2 << lg) * KP * epp <= WG_TABCAP / 2) ++lg;
            p.tab_cht_log2 = lg;
            pl.use_tab = true;
        }
    }
    p.splits = (p.Mpix + p.pix_per_split - 1) / p.pix_per_split;
    if (p.upm && !pl.use_tab) return false;                      // the merged form exists in the table-driven kernel only
    const int halo_splits = p.upm ? 0 : halo_wgrad_splits(d);
    pl.use_halo = halo_splits > 0;
    if (pl.use_halo) { p.splits = halo_splits; pl.use_tab = false; }
    const int stem_splits = p.upm ? 0 : stem_wgrad_splits(d);
    pl.use_stem = stem_splits > 0;
    if (pl.use_stem) { p.splits = stem_splits; pl.use_tab = false; }
    p.want_bias = d->dbias != nullptr;
    wgrad_slab_sizes(pl);
    const int out_taps = p.upm ? 9 : p.taps;                     // filter taps written to OIHW
    int ci_t = 32;                                               // 32 x (CI_T * taps + 1) floats of LDS <= 64 KB ...
    while (ci_t > 1 && ci_t * out_taps > 480) ci_t >>= 1;
    if (ci_t * out_taps > 480) return false;
    const int co_tiles = (d->Cout + 31) / 32;                    // ... and enough blocks to fill the chip
    while (ci_t > 1 && co_tiles * ((d->Cin + ci_t - 1) / ci_t) < 256) ci_t >>= 1;
    pl.ci_t = ci_t;
    return true;
}

// Which weight gradients take wgrad3x3_patch_kernel: 3x3 stride 1, zero or reflection padding, one source of 64-channel multiples, >= 64 outputs.
inline bool wgrad_patch_plan(const mcav_wgrad_desc* d, WgradPlan& pl) {
    static const int enabled = MCAV_KNOB_INT("MCAV_WGRAD_PATCH", 1);
    static const int target = MCAV_KNOB_INT("MCAV_WGRAD_PATCH_WGS", 256);
    if (!enabled || !d || d->mma < 1 || d->mma > 3 || d->upm || d->up1 || d->C2 != 0) return false;
    if (d->mode != MCAV_G_DIRECT || d->kh != 3 || d->kw != 3 || d->stride != 1 || d->sign != 1 || d->offset != -1) return false;
    if (d->pad_mode != MCAV_PAD_ZERO && d->pad_mode != MCAV_PAD_REFLECT) return false;
    if (d->pad_mode == MCAV_PAD_REFLECT && (d->Hs < 2 || d->Ws < 2)) return false;
    if (d->C1 != d->Kp || d->Cin != d->Kp || d->Kp % 64 != 0 || d->Cout < 32 || d->Hd != d->Hs || d->Wd != d->Ws) return false;
    if (d->Cout < 64 && d->Cout != 32) return false;                  // (32 outputs: the narrow form; 33 .. 63 would leave half of a 64-wide tile idle)
    if ((d->Cdy & 3) || (d->dy_choff & 3)) return false;
    mcav_wgrad_desc dd = *d;
    dd.tile = 2;
    if (!plan_wgrad(&dd, pl) || pl.use_halo || pl.use_stem) return false;
    WgradParams& p = pl.p;
    if ((p.CoutLoad & 3) != 0) return false;
    int th, tw;
    patch_block(d->Hd, d->Wd, 64, WGP_PIX, th, tw);
    p.patch = 1; p.split_planes = d->mma >= 2;
    p.pTH = th; p.pTW = tw;
    p.ptiles_y = (d->Hd + th - 1) / th; p.ptiles_x = (d->Wd + tw - 1) / tw;
    p.prefl = d->pad_mode == MCAV_PAD_REFLECT;
    p.pnblocks = d->B * p.ptiles_y * p.ptiles_x;
    p.pct_co = (d->Cout + 63) / 64;
    p.pnarrow = d->Cout <= 32;
    const int ctiles = (d->Kp / 64) * p.pct_co;
    int splits = target / ctiles;                                     // one workgroup per CU
    if (splits < 1) splits = 1;
    if (splits > p.pnblocks) splits = p.pnblocks;
    p.pbps = (p.pnblocks + splits - 1) / splits;
    p.splits = (p.pnblocks + p.pbps - 1) / p.pbps * (p.pnarrow ? 2 : 1);      // slab splits
    pl.use_tab = false;
    wgrad_slab_sizes(pl);
    return true;
}

// Plans the bf16 weight-gradient launch into pl (splits over 64-pixel K-tiles, table chunking); false = not eligible.
inline bool bf16_wgrad_plan(const mcav_wgrad_desc* d, WgradPlan& pl) {
    if (!d || (d->mma < 1 || d->mma > 3) || d->upm) return false;
    if (wgrad_patch_plan(d, pl)) return true;
    if (d->mma == 2) return false;                                    // mma = 2: the split form where it is ahead (the patch kernel), else fp32 MFMA
    if (d->mode != MCAV_G_DIRECT || d->Kp % 16 != 0 || (long)d->C1 + d->C2 != d->Kp || d->Cin != d->Kp) return false;
    if ((d->C1 & 15) || (d->C2 & 15) || d->Cout < 32 || (d->Cdy & 3) || (d->dy_choff & 3)) return false;
    mcav_wgrad_desc dd = *d;
    dd.tile = 2;                                                      // 64 x 64 slab tiles
    if (!plan_wgrad(&dd, pl) || pl.use_halo) return false;
    WgradParams& p = pl.p;
    if ((p.CoutLoad & 3) != 0) return false;
    const int out_tiles = p.mtiles * p.ntiles;
    int max_splits = (p.Mpix + 4 * KPB - 1) / (4 * KPB);
    if (max_splits > 512) max_splits = 512;
    if (max_splits < 1) max_splits = 1;
    const int splits = wgrad_fill_splits(p.Mpix, out_tiles, 1024, max_splits, KPB);      // 1024 resident workgroups (four per CU)
    p.pix_per_split = round_up((p.Mpix + splits - 1) / splits, KPB);
    p.splits = (p.Mpix + p.pix_per_split - 1) / p.pix_per_split;
    int ntmax = 1;
    for (int mt = 0; mt < p.mtiles; ++mt) {
        const int lo = mt * 64 / d->Kp, hi = (mt * 64 + 63) / d->Kp < p.taps - 1 ? (mt * 64 + 63) / d->Kp : p.taps - 1;
        if (hi - lo + 1 > ntmax) ntmax = hi - lo + 1;
    }
    const int epp = ntmax * (d->C2 > 0 ? 2 : 1);
    p.tab_cht_log2 = 20;
    const int tabcap = d->mma >= 2 ? WG_TABCAP / 2 : WG_TABCAP;       // (the split form gives half of the table's LDS to its planes)
    if ((long)p.pix_per_split * epp > tabcap) {
        if (2 * 2 * KPB * epp > tabcap) return false;                 // not even two 2-tile chunks fit
        int lg = 1;
        while ((2 << lg) * KPB * epp <= tabcap / 2) ++lg;
        p.tab_cht_log2 = lg;
    }
    p.split_planes = d->mma >= 2;
    pl.use_tab = true;
    wgrad_slab_sizes(pl);
    return true;
}

// The one decision of the weight gradient, in this order:
//   BatchNorm-fold / planar sources   only the stem kernels implement them: bf16 is not asked, and a plan that is not the stem's is refused;
//   bf16                              the patch kernel, then the table tiles (mma != 0);
//   fp32                              plan_wgrad: the halo or stem kernel where the layer is theirs, else the tile kernels.
inline int plan_wgrad_route(const mcav_wgrad_desc* d, const PlanEnv&, WgradRoute& r) {
    r.family = MCAV_WGRAD_FP32; r.variant = r.workgroups = 0;
    const int bn = stem_wgrad_bn(d);
    const int planar = stem_planar_state(d, stem_wgrad_kind(d));
    if (bn < 0 || planar < 0) return MCAV_E_INVALID;
    if (planar && !d->x1) { r.planar_d = *d; r.planar_d.x1 = d->x_planar[0]; d = &r.planar_d; }
    r.d = d;
    const bool special = bn || planar;
    const bool bf16 = d && d->mma != 0 && !special && bf16_wgrad_plan(d, r.pl);
    if (!bf16 && !plan_wgrad(d, r.pl)) return MCAV_E_INVALID;
    if (special && !r.pl.use_stem) return MCAV_E_INVALID;
    const WgradPlan& pl = r.pl;
    r.workgroups = pl.p.patch ? (pl.p.pnarrow ? pl.p.splits / 2 : pl.p.splits) * (pl.p.Kp / 64) * pl.p.pct_co
                   : pl.use_stem || pl.use_halo ? pl.p.splits : pl.p.splits * pl.p.mtiles * pl.p.ntiles;
    if (bf16) {
        r.family = pl.p.patch ? MCAV_WGRAD_BF16_PATCH : MCAV_WGRAD_BF16_TILE;
        r.variant = (pl.p.split_planes ? MCAV_RV_SPLIT : 0) | (pl.p.patch && pl.p.prefl ? MCAV_RV_REFLECT : 0) | (pl.use_tab ? MCAV_RV_TABLE : 0);
    } else if (pl.use_stem) {
        r.family = MCAV_WGRAD_STEM;
        r.variant = (stem_wgrad_kind(d) == 2 ? MCAV_RV_POSE : 0) | (planar ? MCAV_RV_PLANAR : 0) | (bn ? MCAV_RV_BN_FOLD : 0);
    } else if (pl.use_halo) {
        r.family = MCAV_WGRAD_HALO;
        // upsampled source + reflection padding: 4 merged taps on the low-resolution map (desc.tile bit 10 keeps the 9-tap kernel)
        const bool up = d->up1 && d->pad_mode == MCAV_PAD_REFLECT && !(d->Hs & 1) && !(d->Ws & 1) && d->C1 == 16 && d->Cout <= 16 && !((d->tile >> 10) & 1);
        r.variant = up ? MCAV_RV_UPM : 0;
    } else {
        r.family = MCAV_WGRAD_FP32;
        // (wgrad_kernel's fast gather: what the table-driven kernel asks, without the table's capacity, plus whole 16-pixel rows)
        int BM, BN;
        tile_dims(pl.tile, BM, BN);
        const int wave_ch = BM / 4;          // channels one wavefront's A columns span
        const WgradParams& p = pl.p;
        const bool fast = (p.g.C1 & 3) == 0 && (p.g.C2 & 3) == 0 && (p.g.C2 == 0 || p.g.C1 % wave_ch == 0) && (p.CoutLoad & 3) == 0 && (p.Cdy & 3) == 0 &&
                          (p.dy_choff & 3) == 0 && p.Wd >= 16;
        r.variant = (pl.use_tab ? MCAV_RV_TABLE : fast ? MCAV_RV_FAST : 0) | (pl.p.upm ? MCAV_RV_UPM : 0);
    }
    return MCAV_OK;
}

}  // namespace mcav
