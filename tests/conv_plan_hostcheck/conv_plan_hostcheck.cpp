// csrc/conv_plan.h on the host, under plain g++ (no HIP header): the planner the library launches from, callable without the library.
//   shared object (tests/test_conv_plan_cpu.py): conv_plan_hostcheck_igemm / _wgrad plan an array of descriptors and return what the C ABI's
//     route queries return, for comparison with the library over the whole sweep.
//   -DCONV_PLAN_HOSTCHECK_MAIN: a program of its own (built with -fsanitize=address,undefined): reads the sweep and the library's answers
//     from a file, checks them, then plans degenerate descriptors -- zeros, negative sizes, INT_MAX sizes, filters up to 64 taps -- which must
//     all be refused or planned without an out-of-range read, a signed overflow or a division by zero.  Prints "conv_plan_hostcheck: ok".
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "conv_plan.h"

using namespace mcav;

static const PlanEnv ENV = {256};

// out[i] = {rc, family, variant, tile, mtiles, ntiles, workgroups, splits, uses_bf16}; workspace[i] = 0.  sane = false: a degenerate descriptor;
// mcav_igemm_uses_bf16 is the geometry test of a launchable shape (its caller has the tensors), so it is asked only where the planner accepted.
static void plan_one(const mcav_igemm_desc* d, int* out, long long* workspace, bool sane = true) {
    IgemmRoute r;
    const int rc = plan_igemm(d, ENV, r);
    memset(out, 0, 9 * sizeof(int));
    out[0] = rc;
    if (rc == MCAV_OK) {
        const int vals[7] = {r.family, r.variant, r.tile, r.mtiles, r.ntiles, r.workgroups, r.ksplit > 1 ? r.ksplit : 1};
        memcpy(out + 1, vals, sizeof(vals));
    }
    out[8] = (sane || rc == MCAV_OK) && igemm_uses_bf16(d) ? 1 : 0;
    *workspace = 0;
}

static void plan_one(const mcav_wgrad_desc* d, int* out, long long* workspace, bool = true) {
    WgradRoute r;
    const int rc = plan_wgrad_route(d, ENV, r);
    memset(out, 0, 9 * sizeof(int));
    out[0] = rc;
    *workspace = 0;
    if (rc != MCAV_OK) return;
    const int vals[8] = {r.family, r.variant, r.pl.tile, r.pl.p.mtiles, r.pl.p.ntiles, r.workgroups, r.pl.p.splits,
                         r.family == MCAV_WGRAD_BF16_PATCH || r.family == MCAV_WGRAD_BF16_TILE ? 1 : 0};
    memcpy(out + 1, vals, sizeof(vals));
    *workspace = (long long)r.workspace_bytes();
}

extern "C" void conv_plan_hostcheck_igemm(const mcav_igemm_desc* d, int n, int* out9, long long* workspace) {
    for (int i = 0; i < n; ++i) plan_one(d + i, out9 + 9 * i, workspace + i);
}

extern "C" void conv_plan_hostcheck_wgrad(const mcav_wgrad_desc* d, int n, int* out9, long long* workspace) {
    for (int i = 0; i < n; ++i) plan_one(d + i, out9 + 9 * i, workspace + i);
}

extern "C" int conv_plan_hostcheck_sizes(int which) { return which == 0 ? (int)sizeof(mcav_igemm_desc) : (int)sizeof(mcav_wgrad_desc); }

#ifdef CONV_PLAN_HOSTCHECK_MAIN
// file: for each of the two descriptor kinds  int n;  n descriptors;  n x 9 ints;  n long longs  (what the library answered)
template <class D>
static bool check_section(FILE* f, const char* what) {
    int n = 0;
    if (fread(&n, sizeof(n), 1, f) != 1 || n <= 0) return false;
    std::vector<D> d(n);
    std::vector<int> want(9 * (size_t)n), got(9 * (size_t)n);
    std::vector<long long> want_ws(n), got_ws(n);
    if (fread(d.data(), sizeof(D), n, f) != (size_t)n || fread(want.data(), sizeof(int), want.size(), f) != want.size() ||
        fread(want_ws.data(), sizeof(long long), n, f) != (size_t)n)
        return false;
    for (int i = 0; i < n; ++i) plan_one(&d[i], &got[9 * (size_t)i], &got_ws[i]);
    for (int i = 0; i < n; ++i)
        if (memcmp(&got[9 * (size_t)i], &want[9 * (size_t)i], 9 * sizeof(int)) != 0 || got_ws[i] != want_ws[i]) {
            printf("conv_plan_hostcheck: %s case %d differs from the library\n", what, i);
            return false;
        }
    printf("conv_plan_hostcheck: %d %s cases\n", n, what);
    return true;
}

static const int SIZES[] = {0, -1, 1, 2, 3, 64, INT_MAX, INT_MIN, INT_MAX - 15};

// every int field of a launchable descriptor replaced by each of SIZES in turn, then all of them at once
template <class D, size_t NF>
static int degenerate(const D& base, int D::*const (&fields)[NF]) {
    int planned = 0, out[9];
    long long ws;
    for (int v : SIZES) {
        D all = base;
        for (int D::*f : fields) {
            D one = base;
            one.*f = v;
            all.*f = v;
            plan_one(&one, out, &ws, false);
            planned += out[0] == MCAV_OK;
        }
        plan_one(&all, out, &ws, false);
        planned += out[0] == MCAV_OK;
    }
    return planned;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const bool ok = check_section<mcav_igemm_desc>(f, "igemm") && check_section<mcav_wgrad_desc>(f, "wgrad");
    fclose(f);
    if (!ok) return 1;

    float dummy[4] = {0.f, 0.f, 0.f, 0.f};      // non-null addresses; nothing reads through them
    int planned = 0, out[9];
    long long ws;
    mcav_igemm_desc zi;
    memset(&zi, 0, sizeof(zi));
    plan_one(&zi, out, &ws, false);              // all zeros
    planned += out[0] == MCAV_OK;
    plan_one((const mcav_igemm_desc*)nullptr, out, &ws, false);
    planned += out[0] == MCAV_OK;
    mcav_wgrad_desc zw;
    memset(&zw, 0, sizeof(zw));
    plan_one(&zw, out, &ws);
    planned += out[0] == MCAV_OK;
    plan_one((const mcav_wgrad_desc*)nullptr, out, &ws);
    planned += out[0] == MCAV_OK;
    if (planned != 0) { printf("conv_plan_hostcheck: an empty descriptor was planned\n"); return 1; }

    // a 64 -> 64 convolution at 2 x 8 x 8 with kh x kw = 1x1 .. 8x8 (64 taps), every mma, every int field degenerate in turn
    typedef int mcav_igemm_desc::*IF;
    const IF ifields[] = {&mcav_igemm_desc::B, &mcav_igemm_desc::Hs, &mcav_igemm_desc::Ws, &mcav_igemm_desc::C1, &mcav_igemm_desc::C2, &mcav_igemm_desc::up1,
                          &mcav_igemm_desc::kh, &mcav_igemm_desc::kw, &mcav_igemm_desc::Np, &mcav_igemm_desc::Kp, &mcav_igemm_desc::mode, &mcav_igemm_desc::stride,
                          &mcav_igemm_desc::sign, &mcav_igemm_desc::offset, &mcav_igemm_desc::pad_mode, &mcav_igemm_desc::Hd, &mcav_igemm_desc::Wd, &mcav_igemm_desc::Cd,
                          &mcav_igemm_desc::n_begin, &mcav_igemm_desc::n_count, &mcav_igemm_desc::y_choff, &mcav_igemm_desc::pool, &mcav_igemm_desc::tile,
                          &mcav_igemm_desc::groups, &mcav_igemm_desc::mma, &mcav_igemm_desc::planar_B, &mcav_igemm_desc::planar_stack};
    typedef int mcav_wgrad_desc::*WF;
    const WF wfields[] = {&mcav_wgrad_desc::B, &mcav_wgrad_desc::Hs, &mcav_wgrad_desc::Ws, &mcav_wgrad_desc::C1, &mcav_wgrad_desc::C2, &mcav_wgrad_desc::up1,
                          &mcav_wgrad_desc::kh, &mcav_wgrad_desc::kw, &mcav_wgrad_desc::Kp, &mcav_wgrad_desc::mode, &mcav_wgrad_desc::stride, &mcav_wgrad_desc::sign,
                          &mcav_wgrad_desc::offset, &mcav_wgrad_desc::pad_mode, &mcav_wgrad_desc::Hd, &mcav_wgrad_desc::Wd, &mcav_wgrad_desc::Cdy,
                          &mcav_wgrad_desc::dy_choff, &mcav_wgrad_desc::Cout, &mcav_wgrad_desc::Cin, &mcav_wgrad_desc::tile, &mcav_wgrad_desc::upm,
                          &mcav_wgrad_desc::Cin_total, &mcav_wgrad_desc::ci_offset, &mcav_wgrad_desc::mma, &mcav_wgrad_desc::dy_bn_groups,
                          &mcav_wgrad_desc::planar_B, &mcav_wgrad_desc::planar_stack};
    int launchable = 0;
    for (int k = 1; k <= 8; ++k)
        for (int mma = 0; mma <= 3; ++mma) {
            mcav_igemm_desc d = zi;
            d.x1 = d.x2 = d.w = dummy; d.y = dummy; d.w16 = dummy;
            d.B = 2; d.Hs = d.Ws = d.Hd = d.Wd = 8; d.C1 = 64; d.kh = d.kw = k; d.Np = d.Kp = 64;
            d.mode = MCAV_G_DIRECT; d.stride = 1; d.sign = 1; d.offset = -(k / 2); d.pad_mode = MCAV_PAD_ZERO;
            d.Cd = d.n_count = 64; d.groups = 1; d.mma = mma;
            plan_one(&d, out, &ws);
            launchable += out[0] == MCAV_OK;
            planned += degenerate(d, ifields);
            mcav_wgrad_desc w = zw;
            w.x1 = w.x2 = w.dy = dummy; w.dw_oihw = dummy; w.dbias = dummy;
            w.B = 2; w.Hs = w.Ws = w.Hd = w.Wd = 8; w.C1 = 64; w.kh = w.kw = k; w.Kp = 64;
            w.mode = MCAV_G_DIRECT; w.stride = 1; w.sign = 1; w.offset = -(k / 2); w.pad_mode = MCAV_PAD_ZERO;
            w.Cdy = w.Cout = w.Cin = 64; w.mma = mma;
            plan_one(&w, out, &ws);
            launchable += out[0] == MCAV_OK;
            planned += degenerate(w, wfields);
        }
    if (launchable != 2 * 8 * 4) { printf("conv_plan_hostcheck: %d of the %d base descriptors planned\n", launchable, 2 * 8 * 4); return 1; }
    printf("conv_plan_hostcheck: degenerate descriptors: %d planned, the rest refused\n", planned);
    printf("conv_plan_hostcheck: ok\n");
    return 0;
}
#endif
