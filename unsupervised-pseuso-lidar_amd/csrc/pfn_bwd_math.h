// Per-pillar arithmetic of the pillar feature net's backward (include/mcav_depth.h: mcav_pillar_pseudo_image_bwd), shared by the HIP kernels
// (pfn_bwd.hip) and by the host-compiled check in tests/pfn_bwd_hostcheck (never by the product on the host, apart from the argument
// checks).  The definition is tests/pfn_bwd_ref.py.  The forward's pre / act / maximum are pfn_math.h's, so the slot that won a channel
// is the one whose value the forward wrote, bit for bit; d_voxels is an ordered fmaf chain over the channels in float32; the terms of the
// three sums are float64 (a product of two float32 is exact there).
#pragma once
#include "pfn_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcav {
namespace pfn {

constexpr int BWD_CHUNK = 64;            // consecutive rows a workgroup stages the upstream gradient of at a time
constexpr int BWD_GRID = 1024;           // workgroups at most: the rows of the slab; chunk i belongs to workgroup i % grid

MCAV_PFN_HD long long bwd_chunks(long long capacity) { return (capacity + BWD_CHUNK - 1) / BWD_CHUNK; }
MCAV_PFN_HD int bwd_grid(long long capacity) {
    const long long c = bwd_chunks(capacity);
    return c < 1 ? 1 : (c < BWD_GRID ? (int)c : BWD_GRID);
}
// the sums a channel owns: d_weight[o, 0 .. C - 1], d_bias[o], d_bias_pad[o]
MCAV_PFN_HD int bwd_sums(int C) { return C + 2; }

// whether row r names a cell of the canvas
MCAV_PFN_HD bool cell_inside(const int* coords, long long r, int B, int ny, int nx) {
    const int b = coords[4 * r], iy = coords[4 * r + 2], ix = coords[4 * r + 3];
    return b >= 0 && b < B && iy >= 0 && iy < ny && ix >= 0 && ix < nx;
}

// where (b, o, iy, ix) of the canvas gradient lies
MCAV_PFN_HD size_t canvas_index(bool nhwc, int b, int o, int iy, int ix, int c_out, int ny, int nx) {
    return nhwc ? (((size_t)b * ny + iy) * nx + ix) * c_out + o : (((size_t)b * c_out + o) * ny + iy) * nx + ix;
}

// g[p, o]: the canvas part (+0.0 without one), d_features added in float32 when there are any
MCAV_PFN_HD float upstream(float canvas_part, bool has_features, float feature_part) {
    return has_features ? canvas_part + feature_part : canvas_part;
}

// The forward's maximum with the slot that attains it.  k: the lowest slot whose act equals the maximum, -1 while the padding term (or
// nothing) holds it; a slot that ties the padding takes it.
struct Winner {
    Max s;
    int k;
};

MCAV_PFN_HD Winner win_start(bool has_padding, float bias_pad) { return Winner{max_start(has_padding, bias_pad), -1}; }

MCAV_PFN_HD void win_join(Winner& w, float a, int k) {
    const bool take = a > w.s.m || (w.k < 0 && a == w.s.m);       // false for a NaN
    max_join(w.s, a);
    w.k = take ? k : w.k;
}

// gradient flows iff feat > 0: not for a NaN, not at relu's corner
MCAV_PFN_HD bool win_flows(const Winner& w) { return !w.s.nan && w.s.m > 0.0f; }

constexpr int NO_FLOW = -2, PADDING = -1;  // win_slot's other answers
// the slot the gradient of (p, o) goes to, PADDING when act(bias_pad) won, NO_FLOW when nothing gets it
MCAV_PFN_HD int win_slot(const Winner& w) { return win_flows(w) ? w.k : NO_FLOW; }

// one pillar's rows [N, C] (n used) under channel (w [C], bias, bias_pad)
MCAV_PFN_HD Winner winner(const float* rows, int n, int N, int C, const float* w, float bias, float bias_pad) {
    Winner s = win_start(n < N, bias_pad);
    for (int k = 0; k < n; ++k) win_join(s, act(pre(rows + (size_t)k * C, w, C, bias)), k);
    return s;
}

// d_voxels[p, k, c]: over the channels in ascending order, those whose gradient goes to slot k.  g [c_out], slot [c_out] = win_slot
template <class G, class S, class W>
MCAV_PFN_HD float d_voxel(const G& g, const S& slot, const W& weight, int c_out, int C, int k, int c) {
    float acc = 0.0f;
    for (int o = 0; o < c_out; ++o)
        if (slot[o] == k) acc = fmaf(g[o], weight[o * C + c], acc);
    return acc;
}

}  // namespace pfn
}  // namespace mcav
