// Per-slot and per-pillar arithmetic of the pillar feature net (include/mcav_depth.h: mcav_pillar_pseudo_image), shared by the HIP kernels
// (pfn_image.hip) and by the host-compiled check in tests/pfn_hostcheck (never by the product on the host, apart from the argument
// checks).  The definition is tests/pfn_ref.py.  float32; the only rounding is fmaf's, one per column, in ascending column order: the
// device's v_fma_f32 and the host's fmaf are both correctly rounded, so the two give the same bits.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MCAV_PFN_HD __host__ __device__ __forceinline__
#else
#define MCAV_PFN_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)           // nothing here is a product followed by a sum outside fmaf; keep it so
#endif

namespace mcav {
namespace pfn {

constexpr int MAX_POINTS = 64;           // a pillar's slots (pillar_math.h)
constexpr int MAX_COLUMNS = 9;
constexpr int MIN_OUT = 32, MAX_OUT = 128;

MCAV_PFN_HD bool columns_ok(int c) { return c == 4 || c == 9; }
MCAV_PFN_HD bool c_out_ok(int c) { return c >= MIN_OUT && c <= MAX_OUT && c % 32 == 0; }

// the layer before its ReLU for one slot and one output channel: bias, then one fmaf per column in ascending order
MCAV_PFN_HD float pre(const float* x, const float* w, int C, float bias) {
    float acc = bias;
    for (int c = 0; c < C; ++c) acc = fmaf(x[c], w[c], acc);
    return acc;
}

// ReLU that keeps a NaN: -0.0, negative values and -inf give +0.0
MCAV_PFN_HD float act(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }

// The NaN-propagating maximum (torch.max) of values that act() returned, i.e. of +0.0, positive numbers, +inf and NaNs.  The running
// maximum of the numbers and whether a NaN was seen are kept apart; which NaN comes out is not defined.
struct Max {
    float m;
    bool nan;
};

// what the padding rows contribute: act(bias_pad) when the pillar has unused slots, nothing (+0.0 is below or equal to every act())
// otherwise
MCAV_PFN_HD Max max_start(bool has_padding, float bias_pad) {
    const float p = has_padding ? act(bias_pad) : 0.0f;
    return Max{p != p ? 0.0f : p, p != p};
}

MCAV_PFN_HD void max_join(Max& s, float a) {
    s.nan = s.nan || a != a;
    s.m = a > s.m ? a : s.m;               // false for a NaN
}

MCAV_PFN_HD float max_value(const Max& s) { return s.nan ? NAN : s.m; }

// the slots of a pillar that hold points
MCAV_PFN_HD int used_slots(int num_points, int N) { return num_points < 0 ? 0 : (num_points > N ? N : num_points); }

// the pillars that exist: min(pillar_offsets[B], capacity), never negative
MCAV_PFN_HD long long live_pillars(const int* pillar_offsets, int B, long long capacity) {
    const long long t = pillar_offsets[B] < 0 ? 0 : pillar_offsets[B];
    return t < capacity ? t : capacity;
}

// The rows of image b among the live pillars, [lo, hi), whatever the table holds: 0 <= lo <= hi <= P.
MCAV_PFN_HD void image_rows(const int* pillar_offsets, int b, long long P, long long& lo, long long& hi) {
    const long long a = pillar_offsets[b], e = pillar_offsets[b + 1];
    lo = a < 0 ? 0 : (a > P ? P : a);
    hi = e < lo ? lo : (e > P ? P : e);
}

// ---- the search for a tile's rows: coords [*, 4] = (b, 0, iy, ix), ascending in (iy, ix) within an image.  64 probes per round (a
// wavefront's lanes; a dependent load per round instead of one per halving): probe i looks at row lo + i * step.
constexpr int PROBES = 64;

MCAV_PFN_HD bool row_below(const int* coords, long long r, int y, int x) {
    const int cy = coords[4 * r + 2], cx = coords[4 * r + 3];
    return cy < y || (cy == y && cx < x);
}

MCAV_PFN_HD long long search_step(long long lo, long long hi) { return hi - lo <= PROBES ? 1 : (hi - lo + PROBES - 1) / PROBES; }

// `below` of the round's probes (those inside [lo, hi)) are below the target: the first row that is not lies behind the last of them
// and not behind the next probe.  The range shrinks by at least a factor of 64 or ends (lo == hi: the answer); on unsorted rows it stays
// inside the range it had.
MCAV_PFN_HD void search_narrow(long long& lo, long long& hi, long long step, int below) {
    if (below == 0) { hi = lo; return; }
    const long long next = lo + below * step;
    lo = lo + (below - 1) * step + 1;
    hi = next < hi ? next : hi;
}

// The first row r of [lo, hi) whose (iy, ix) is not below (y, x) in row-major order; hi if there is none: the rounds above with the
// probes one after another (the kernel's lanes take one each and count with a ballot).
MCAV_PFN_HD long long first_at_or_after(const int* coords, long long lo, long long hi, int y, int x) {
    while (lo < hi) {
        const long long step = search_step(lo, hi);
        int below = 0;
        for (int i = 0; i < PROBES; ++i) {
            const long long r = lo + i * step;
            below += r < hi && row_below(coords, r, y, x) ? 1 : 0;
        }
        search_narrow(lo, hi, step, below);
    }
    return lo;
}

// whether row r belongs to the tile of row iy of image b that starts at column x0 and is w columns wide
MCAV_PFN_HD bool in_tile(const int* coords, long long r, int b, int iy, int x0, int w) {
    const int ix = coords[4 * r + 3];
    return coords[4 * r] == b && coords[4 * r + 2] == iy && ix >= x0 && ix < x0 + w;
}

}  // namespace pfn
}  // namespace mcav
