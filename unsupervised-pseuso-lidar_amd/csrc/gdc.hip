// Graph-based depth correction from sparse LiDAR (Pseudo-LiDAR++ GDC; include/mcav_depth.h: mcav_gdc_graph, mcav_gdc_solve; the definition
// is tests/gdc_ref.py, the per-pixel arithmetic csrc/gdc_math.h).
//   graph   : a workgroup owns a 16 x 16 tile; the tile's points plus a `radius` halo go into LDS, back-projected once; one thread per
//             pixel walks its window in raster order (ascending pixel index: the tie rule costs nothing) and keeps the best in registers
//             (compile-time slots), then forms the closed-form weights and stores k neighbour indices and k weights.
//   solve   : count     graph / known pixels per image (integer atomics) and every pixel's in-degree: pixel j scans its window in raster
//                       order for the sources that list it -- the in-degree is bounded by the window, so no atomics and no sort
//             scan/fill the in-degrees become CSR row starts (one block scans the per-block sums); the window is walked again and the
//                       (source, weight) pairs are stored in ascending source order
//             init      out = the start vector (sparse on known graph pixels, depth elsewhere), r = p = 0; pass-through images are marked done
//             fwd<INIT> q = M v with v = out (INIT) or p (the workgroup's rows of the graph pass through LDS); |q|^2 as float64
//                       per-workgroup sums to a slab; the image's last workgroup (mcav_common.h's ticket, drawn in two levels) adds them
//                       in a fixed order and forms alpha, or marks the image done
//             tr<INIT>  r = -(M^T q) and p = r (INIT), or x += alpha p and r -= alpha M^T q, over the unknown pixels; |r|^2 the same way;
//                       the last workgroup forms beta, counts the iteration and tests rs <= tol^2 rs0
//             pupd      p = r + beta p
//             info      the [B, 4] rows
//   Three launches per iteration (fwd, tr, pupd); the workgroups of an image that is done exit on its flag.  Nothing returns to the host,
//   no float atomics, no allocation: the call can be captured, and two runs give the same bytes.
#include <type_traits>

#include "block_ops.h"
#include "gdc_math.h"

namespace mcav {
namespace gdc {

constexpr int TILE = 16, THREADS = 256, WAVES = THREADS / 64;
constexpr int SPAN = TILE + 2 * MAX_RADIUS;              // 30: the tile and its widest halo

// ------------------------------------------------------------------------------------------------------------------- the graph
template <int KC>
__global__ __launch_bounds__(THREADS) void gdc_graph_kernel(const float* depth, const float* sparse, const float* Kmat, int H, int W, Params pr,
                                                            int* nbr, float* weights, unsigned char* flags) {
    __shared__ float sx[SPAN * SPAN], sy[SPAN * SPAN], sz[SPAN * SPAN];       // z = 0 marks "no point here"
    const int b = blockIdx.z, tid = threadIdx.x, r = pr.radius, span = TILE + 2 * r;
    const int y0 = blockIdx.y * TILE - r, x0 = blockIdx.x * TILE - r;
    const size_t image = (size_t)b * H * W;
    const float fx = Kmat[b * 4 + 0], fy = Kmat[b * 4 + 1], cx = Kmat[b * 4 + 2], cy = Kmat[b * 4 + 3];
    for (int e = tid; e < span * span; e += THREADS) {
        const int ly = e / span, lx = e - ly * span, gy = y0 + ly, gx = x0 + lx;
        Point p{0.0f, 0.0f, 0.0f};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float z = depth[image + (size_t)gy * W + gx];
            if (in_range(z, pr.min_depth, pr.max_depth)) p = back_project(gx, gy, z, fx, fy, cx, cy);
        }
        sx[e] = p.x; sy[e] = p.y; sz[e] = p.z;
    }
    __syncthreads();
    const int ty = tid / TILE, tx = tid - ty * TILE, gy = y0 + r + ty, gx = x0 + r + tx;
    if (gy >= H || gx >= W) return;
    const int me = (ty + r) * span + tx + r;
    const Point mine{sx[me], sy[me], sz[me]};
    float bd[KC], w[KC], dz[KC];
    int bi[KC];
    best_init<KC>(bd, bi);
    const bool valid = mine.z > 0.0f;
    if (valid) {
        for (int wy = 0; wy <= 2 * r; ++wy) {
            const int row = (ty + wy) * span + tx, gyy = gy - r + wy;
            for (int wx = 0; wx <= 2 * r; ++wx) {
                const int e = row + wx;
                const float z = sz[e];
                if (e == me || !(z > 0.0f)) continue;
                const Point other{sx[e], sy[e], z};
                best_insert<KC>(bd, bi, dist2(mine, other), gyy * W + (gx - r + wx));
            }
        }
    }
    int m = 0;
#pragma unroll
    for (int s = 0; s < KC; ++s) {
        const bool used = s < pr.k && bi[s] >= 0;
        m += used ? 1 : 0;
        dz[s] = 0.0f;
        if (used) {
            const int jy = bi[s] / W, jx = bi[s] - jy * W;
            dz[s] = sz[(jy - y0) * span + (jx - x0)] - mine.z;
        }
    }
    lle_weights<KC>(dz, m, pr.k, pr.reg, w);
    const size_t pix = image + (size_t)gy * W + gx;
#pragma unroll
    for (int s = 0; s < KC; ++s)
        if (s < pr.k) {
            nbr[pix * pr.k + s] = s < m ? bi[s] : -1;
            weights[pix * pr.k + s] = w[s];
        }
    const bool known = valid && in_range(sparse[pix], pr.min_depth, pr.max_depth);
    flags[pix] = (unsigned char)((m > 0 ? IN_GRAPH : 0) | (known ? KNOWN : 0));
}

// ------------------------------------------------------------------------------------------------------------------- the solver
struct Solve {
    const float* depth; const float* sparse; const int* nbr; const float* weights; const unsigned char* flags;
    float* out; float* info;
    int B, H, W, k, radius, min_known, G;                 // G: workgroups per image; an image's rows are padded to G * THREADS
    double thresh;                                        // tol^2
    int* counts;                                          // [B][2]: graph pixels, known graph pixels
    unsigned* tickets;                                    // [B]
    unsigned* group_tickets;                              // [B][ceil(G / 16)]
    unsigned* done; unsigned* iters_run;                  // [B]
    float* alpha; float* beta;                            // [B]
    double* rs; double* rs0;                              // [B]
    double* slab;                                         // [B][G]
    double* group_slab;                                   // [B][ceil(G / 16)]
    int* row_start;                                       // [B * G * THREADS + 1]: in-degrees, then CSR row starts
    int* block_sum;                                       // [B * G]
    int2* entries;                                        // [<= k B H W]: (source pixel, weight bits), ascending source within a row
    float* r; float* p; float* q;                         // [B H W]
};

// The sources that list pixel j of image b, in raster (ascending index) order: f(source, slot) for each.
template <typename Fn>
__device__ __forceinline__ void for_each_source(const Solve& a, int b, int j, Fn f) {
    const int jy = j / a.W, jx = j - jy * a.W;
    const size_t image = (size_t)b * a.H * a.W;
    const int ya = max(jy - a.radius, 0), yb = min(jy + a.radius, a.H - 1), xa = max(jx - a.radius, 0), xb = min(jx + a.radius, a.W - 1);
    for (int y = ya; y <= yb; ++y)
        for (int x = xa; x <= xb; ++x) {
            const int i = y * a.W + x;
            if (i == j || !(a.flags[image + i] & IN_GRAPH)) continue;
            const int* row = a.nbr + (image + i) * (size_t)a.k;
            for (int s = 0; s < a.k; ++s)
                if (row[s] == j) { f(i, s); break; }
        }
}

__global__ __launch_bounds__(THREADS) void gdc_count_kernel(Solve a) {
    __shared__ int s_red[4];
    const int b = blockIdx.y, tid = threadIdx.x, n = a.H * a.W, i = blockIdx.x * THREADS + tid;
    int fl = 0, degree = 0;
    if (i < n) fl = a.flags[(size_t)b * n + i];
    if (fl & IN_GRAPH) for_each_source(a, b, i, [&](int, int) { ++degree; });
    a.row_start[((size_t)b * a.G + blockIdx.x) * THREADS + tid] = degree;
    const int graph = block_sum<int, WAVES>((fl & IN_GRAPH) ? 1 : 0, s_red);
    const int known = block_sum<int, WAVES>((fl & (IN_GRAPH | KNOWN)) == (IN_GRAPH | KNOWN) ? 1 : 0, s_red);
    const int total = block_sum<int, WAVES>(degree, s_red);
    if (tid == 0) {
        if (graph) atomicAdd(a.counts + 2 * b, graph);
        if (known) atomicAdd(a.counts + 2 * b + 1, known);
        a.block_sum[b * a.G + blockIdx.x] = total;
    }
}

// exclusive scan of the per-block sums in one block, 256 per pass; the total closes the last row
__global__ __launch_bounds__(THREADS) void gdc_scan_kernel(Solve a) {
    __shared__ int s_red[4];
    const int nblocks = a.B * a.G;
    const int total = chunked_scan<int, WAVES>(nblocks, s_red, [&](int i) { return a.block_sum[i]; }, [&](int i, int v) { a.block_sum[i] = v; });
    if (threadIdx.x == 0) a.row_start[(size_t)nblocks * THREADS] = total;
}

__global__ __launch_bounds__(THREADS) void gdc_fill_kernel(Solve a) {
    __shared__ int s_red[4];
    const int b = blockIdx.y, tid = threadIdx.x, n = a.H * a.W, i = blockIdx.x * THREADS + tid;
    const size_t slot = ((size_t)b * a.G + blockIdx.x) * THREADS + tid;
    const int degree = a.row_start[slot];
    int total;
    int at = a.block_sum[b * a.G + blockIdx.x] + block_scan<int, WAVES>(degree, s_red, total);
    a.row_start[slot] = at;
    if (degree == 0 || i >= n) return;
    const size_t image = (size_t)b * n;
    for_each_source(a, b, i, [&](int src, int s) {
        a.entries[at++] = make_int2(src, __float_as_int(a.weights[(image + src) * (size_t)a.k + s]));
    });
}

__global__ __launch_bounds__(THREADS) void gdc_init_kernel(Solve a) {
    const int b = blockIdx.y, n = a.H * a.W, i = blockIdx.x * THREADS + threadIdx.x;
    const bool pass = a.counts[2 * b + 1] < a.min_known;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.done[b] = pass ? 1u : 0u;
        a.iters_run[b] = 0u;
        a.alpha[b] = 0.0f; a.beta[b] = 0.0f;
        a.rs[b] = 0.0; a.rs0[b] = 0.0;
    }
    if (i >= n) return;
    const size_t pix = (size_t)b * n + i;
    const unsigned fl = a.flags[pix];
    const bool take = !pass && (fl & (IN_GRAPH | KNOWN)) == (IN_GRAPH | KNOWN);
    a.out[pix] = take ? a.sparse[pix] : a.depth[pix];
    a.r[pix] = 0.0f; a.p[pix] = 0.0f; a.q[pix] = 0.0f;
}

// One workgroup's share of an inner product goes to the slab; the image's last workgroup returns true with the total in `sum`.  Tickets
// drawn on one address are served one after another, so they are drawn in two levels: the GROUP workgroups of a group share a ticket, the
// group's last workgroup adds the group's entries in a fixed order and draws the image's ticket, of which there are G / GROUP; with one
// ticket per image its 480 draws (192 x 640) took 50 us of each launch.
constexpr int GROUP = 16;

__device__ __forceinline__ bool image_total(const Solve& a, int b, double mine, double* s_red, int* s_flag, double& sum) {
    const int tid = threadIdx.x;
    const double part = block_sum<double, WAVES>(mine, s_red);
    if (tid == 0) handoff_store(a.slab + (size_t)b * a.G + blockIdx.x, part);
    handoff_release();                                    // handoff_last's steps, with the group's arithmetic behind the wait as before
    __syncthreads();
    const int groups = (a.G + GROUP - 1) / GROUP, g = blockIdx.x / GROUP, first = g * GROUP, members = min(GROUP, a.G - first);
    if (tid == 0) *s_flag = handoff_ticket(&a.group_tickets[b * groups + g]) == (unsigned)(members - 1);
    __syncthreads();
    if (!*s_flag) return false;
    double t = tid < members ? handoff_load(a.slab + (size_t)b * a.G + first + tid) : 0.0;
    const double group_sum = block_sum<double, WAVES>(t, s_red);  // a fixed order
    if (tid == 0) {
        handoff_store(a.group_slab + (size_t)b * groups + g, group_sum);
        handoff_store(&a.group_tickets[b * groups + g], 0u);
    }
    if (!handoff_last([&] { return &a.tickets[b]; }, groups, s_flag)) return false;
    t = 0.0;                                              // a fixed order: thread t takes entries t, t + 256, ...
    for (int e = tid; e < groups; e += THREADS) t += handoff_load(a.group_slab + (size_t)b * groups + e);
    sum = block_sum<double, WAVES>(t, s_red);
    return true;
}

// q = M v over the graph pixels: v_i - sum over the slots, in neighbour order, of w v_j.  The workgroup's 256 rows of nbr and weights are
// one contiguous stretch: it is loaded with full-width accesses into LDS (rows at an odd stride: no bank conflicts) and each thread then
// reads its own row; the KC gathers of a thread are issued together and added in order.
template <bool INIT, int KC>
__global__ __launch_bounds__(THREADS) void gdc_fwd_kernel(Solve a) {
    constexpr int STRIDE = KC | 1;
    __shared__ int s_idx[THREADS * STRIDE];
    __shared__ float s_w[THREADS * STRIDE];
    __shared__ double s_red[4];
    __shared__ int s_flag;
    const int b = blockIdx.y, tid = threadIdx.x, n = a.H * a.W, first = blockIdx.x * THREADS, i = first + tid, k = a.k;
    if (a.done[b]) return;
    const size_t image = (size_t)b * n;
    const float* v = (INIT ? a.out : a.p) + image;
    const int rows = min(THREADS, n - first);
    const int* gn = a.nbr + (image + first) * (size_t)k;
    const float* gw = a.weights + (image + first) * (size_t)k;
    for (int e = tid; e < rows * k; e += THREADS) {
        const int row = e / k, s = e - row * k;
        s_idx[row * STRIDE + s] = gn[e];
        s_w[row * STRIDE + s] = gw[e];
    }
    __syncthreads();
    float qi = 0.0f;
    if (i < n && (a.flags[image + i] & IN_GRAPH)) {
        float vj[KC];
        bool used[KC];
#pragma unroll
        for (int s = 0; s < KC; ++s) {
            const int j = s < k ? s_idx[tid * STRIDE + s] : -1;
            used[s] = (unsigned)j < (unsigned)n;
            vj[s] = used[s] ? v[j] : 0.0f;
        }
        float acc = 0.0f;
#pragma unroll
        for (int s = 0; s < KC; ++s)
            if (used[s]) acc = acc + s_w[tid * STRIDE + s] * vj[s];
        qi = v[i] - acc;
        a.q[image + i] = qi;
    }
    if (INIT) return;
    double den;
    if (!image_total(a, b, (double)qi * (double)qi, s_red, &s_flag, den)) return;
    if (tid == 0) {
        if (den > 0.0) handoff_store(a.alpha + b, (float)(a.rs[b] / den));
        else handoff_store(a.done + b, 1u);
        handoff_store(&a.tickets[b], 0u);
    }
}

constexpr int CHUNK = 4096;                               // entries of the transposed rows staged per pass: 32 KB of LDS

// over the unknown pixels: t = (M^T q)_j = q_j - sum over the sources, ascending, of w q_source.  The rows of a workgroup are one
// contiguous stretch of the CSR: it passes through LDS CHUNK entries at a time, loaded with full-width accesses; a thread takes its own
// entries of the stretch in order, four gathers in flight.
template <bool INIT>
__global__ __launch_bounds__(THREADS) void gdc_tr_kernel(Solve a) {
    __shared__ int2 s_ent[CHUNK];
    __shared__ double s_red[4];
    __shared__ int s_flag;
    const int b = blockIdx.y, tid = threadIdx.x, n = a.H * a.W, i = blockIdx.x * THREADS + tid;
    if (a.done[b]) return;
    const size_t image = (size_t)b * n;
    const float* q = a.q + image;
    const size_t slot0 = ((size_t)b * a.G + blockIdx.x) * THREADS;
    const int E0 = a.row_start[slot0], E1 = a.row_start[slot0 + THREADS];
    const bool mine = i < n && (a.flags[image + i] & (IN_GRAPH | KNOWN)) == IN_GRAPH;
    const int e0 = mine ? a.row_start[slot0 + tid] : 0, e1 = mine ? a.row_start[slot0 + tid + 1] : 0;
    float acc = 0.0f;
    for (int c0 = E0; c0 < E1; c0 += CHUNK) {
        const int c1 = min(c0 + CHUNK, E1);
        __syncthreads();                                  // the previous pass has been consumed
        for (int e = c0 + tid; e < c1; e += THREADS) s_ent[e - c0] = a.entries[e];
        __syncthreads();
        int e = max(e0, c0);
        const int hi = min(e1, c1);
        for (; e + 4 <= hi; e += 4) {
            const int2 en0 = s_ent[e - c0], en1 = s_ent[e - c0 + 1], en2 = s_ent[e - c0 + 2], en3 = s_ent[e - c0 + 3];
            const float q0 = q[en0.x], q1 = q[en1.x], q2 = q[en2.x], q3 = q[en3.x];
            acc = acc + __int_as_float(en0.y) * q0;
            acc = acc + __int_as_float(en1.y) * q1;
            acc = acc + __int_as_float(en2.y) * q2;
            acc = acc + __int_as_float(en3.y) * q3;
        }
        for (; e < hi; ++e) {
            const int2 en = s_ent[e - c0];
            acc = acc + __int_as_float(en.y) * q[en.x];
        }
    }
    float ri = 0.0f;
    if (mine) {
        const float t = q[i] - acc;
        if (INIT) {
            ri = -t;
            a.p[image + i] = ri;
        } else {
            const float alpha = a.alpha[b];
            a.out[image + i] = a.out[image + i] + alpha * a.p[image + i];
            ri = a.r[image + i] - alpha * t;
        }
        a.r[image + i] = ri;
    }
    double rs;
    if (!image_total(a, b, (double)ri * (double)ri, s_red, &s_flag, rs)) return;
    if (tid == 0) {
        if (INIT) {
            handoff_store(a.rs0 + b, rs);
            if (!(rs > 0.0) || rs <= a.thresh * rs) handoff_store(a.done + b, 1u);
        } else {
            handoff_store(a.beta + b, (float)(rs / a.rs[b]));
            handoff_store(a.iters_run + b, a.iters_run[b] + 1u);
            if (!(rs > 0.0) || rs <= a.thresh * a.rs0[b]) handoff_store(a.done + b, 1u);
        }
        handoff_store(a.rs + b, rs);
        handoff_store(&a.tickets[b], 0u);
    }
}

__global__ __launch_bounds__(THREADS) void gdc_pupd_kernel(Solve a) {
    const int b = blockIdx.y, n = a.H * a.W, i = blockIdx.x * THREADS + threadIdx.x;
    if (a.done[b] || i >= n) return;
    const size_t pix = (size_t)b * n + i;
    if ((a.flags[pix] & (IN_GRAPH | KNOWN)) == IN_GRAPH) a.p[pix] = a.r[pix] + a.beta[b] * a.p[pix];
}

__global__ __launch_bounds__(64) void gdc_info_kernel(Solve a) {
    for (int b = threadIdx.x; b < a.B; b += 64) {
        const int graph = a.counts[2 * b], known = a.counts[2 * b + 1];
        const double rs0 = a.rs0[b];
        float* row = a.info + 4 * b;
        row[0] = (float)graph;
        row[1] = (float)known;
        row[2] = (float)a.iters_run[b];
        row[3] = known < a.min_known ? 1.0f : (rs0 > 0.0 ? (float)(a.rs[b] / rs0) : 0.0f);
    }
}

struct Layout {
    size_t counts, tickets, group_tickets, group_slab, done, iters_run, alpha, beta, rs, rs0, slab, row_start, block_sum, entries, r, p, q, total, zeroed;
    int G;
};

inline bool layout(int B, int H, int W, int k, int radius, Layout& l) {
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || k < 1 || k > MAX_K || radius < 1 || radius > MAX_RADIUS) return false;
    const unsigned long long n = (unsigned long long)H * (unsigned long long)W;
    if (n > (1ull << 24)) return false;                   // the info row holds pixel counts as float32
    const unsigned long long G = (n + THREADS - 1) / THREADS, padded = (unsigned long long)B * G * THREADS;
    if (padded * (unsigned long long)k > 0x7fffffffull || (unsigned long long)B * G > 0x7fffffffull) return false;      // int32 entry indices
    l.G = (int)G;
    const size_t N = (size_t)B * (size_t)n;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += align_up(bytes, 256); return here; };
    l.counts = take(sizeof(int) * 2 * B);
    l.tickets = take(sizeof(unsigned) * B);
    const size_t groups = (size_t)((G + 15) / 16);
    l.group_tickets = take(sizeof(unsigned) * (size_t)B * groups);
    l.zeroed = at;                                        // counts and tickets: cleared by every call
    l.done = take(sizeof(unsigned) * B);
    l.iters_run = take(sizeof(unsigned) * B);
    l.alpha = take(sizeof(float) * B);
    l.beta = take(sizeof(float) * B);
    l.rs = take(sizeof(double) * B);
    l.rs0 = take(sizeof(double) * B);
    l.slab = take(sizeof(double) * (size_t)B * G);
    l.group_slab = take(sizeof(double) * (size_t)B * groups);
    l.row_start = take(sizeof(int) * ((size_t)padded + 1));
    l.block_sum = take(sizeof(int) * (size_t)B * G);
    l.entries = take(sizeof(int2) * N * (size_t)k);
    l.r = take(sizeof(float) * N);
    l.p = take(sizeof(float) * N);
    l.q = take(sizeof(float) * N);
    l.total = at;
    return true;
}

}  // namespace gdc
}  // namespace mcav

using namespace mcav;

MCAV_EXPORT size_t mcav_gdc_workspace_bytes(int B, int H, int W, int k, int radius) {
    gdc::Layout l;
    return gdc::layout(B, H, W, k, radius, l) ? l.total : 0;
}

MCAV_EXPORT int mcav_gdc_graph(const float* depth, const float* sparse, const float* K, int B, int H, int W, int k, int radius, float reg,
                               float min_depth, float max_depth, int* nbr, float* weights, unsigned char* flags, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!depth || !sparse || !K || !nbr || !weights || !flags || !workspace) return MCAV_E_INVALID;
    const gdc::Params pr{reg, min_depth, max_depth, k, radius};
    gdc::Layout l;
    if (!gdc::layout(B, H, W, k, radius, l) || !gdc::params_ok(pr)) return MCAV_E_INVALID;
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    const dim3 grid((unsigned)((W + gdc::TILE - 1) / gdc::TILE), (unsigned)((H + gdc::TILE - 1) / gdc::TILE), (unsigned)B);
    if (grid.y > 65535u) return MCAV_E_INVALID;
    hipStream_t s = as_stream(stream);
    if (k <= 4) gdc::gdc_graph_kernel<4><<<grid, gdc::THREADS, 0, s>>>(depth, sparse, K, H, W, pr, nbr, weights, flags);
    else if (k <= 8) gdc::gdc_graph_kernel<8><<<grid, gdc::THREADS, 0, s>>>(depth, sparse, K, H, W, pr, nbr, weights, flags);
    else if (k <= 12) gdc::gdc_graph_kernel<12><<<grid, gdc::THREADS, 0, s>>>(depth, sparse, K, H, W, pr, nbr, weights, flags);
    else gdc::gdc_graph_kernel<16><<<grid, gdc::THREADS, 0, s>>>(depth, sparse, K, H, W, pr, nbr, weights, flags);
    return launch_status();
}

MCAV_EXPORT int mcav_gdc_solve(const float* depth, const float* sparse, const int* nbr, const float* weights, const unsigned char* flags, int B,
                               int H, int W, int k, int radius, int min_known, int iters, float tol, float* out, float* info, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!depth || !sparse || !nbr || !weights || !flags || !out || !info || !workspace) return MCAV_E_INVALID;
    gdc::Layout l;
    if (!gdc::layout(B, H, W, k, radius, l) || iters < 0 || !(tol >= 0.0f) || out == depth || out == sparse) return MCAV_E_INVALID;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return MCAV_E_INVALID;
    if (workspace_bytes < l.total) return MCAV_E_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    gdc::Solve a;
    a.depth = depth; a.sparse = sparse; a.nbr = nbr; a.weights = weights; a.flags = flags; a.out = out; a.info = info;
    a.B = B; a.H = H; a.W = W; a.k = k; a.radius = radius; a.min_known = min_known; a.G = l.G;
    a.thresh = (double)tol * (double)tol;
    a.counts = reinterpret_cast<int*>(ws + l.counts);
    a.tickets = reinterpret_cast<unsigned*>(ws + l.tickets);
    a.group_tickets = reinterpret_cast<unsigned*>(ws + l.group_tickets);
    a.group_slab = reinterpret_cast<double*>(ws + l.group_slab);
    a.done = reinterpret_cast<unsigned*>(ws + l.done);
    a.iters_run = reinterpret_cast<unsigned*>(ws + l.iters_run);
    a.alpha = reinterpret_cast<float*>(ws + l.alpha);
    a.beta = reinterpret_cast<float*>(ws + l.beta);
    a.rs = reinterpret_cast<double*>(ws + l.rs);
    a.rs0 = reinterpret_cast<double*>(ws + l.rs0);
    a.slab = reinterpret_cast<double*>(ws + l.slab);
    a.row_start = reinterpret_cast<int*>(ws + l.row_start);
    a.block_sum = reinterpret_cast<int*>(ws + l.block_sum);
    a.entries = reinterpret_cast<int2*>(ws + l.entries);
    a.r = reinterpret_cast<float*>(ws + l.r);
    a.p = reinterpret_cast<float*>(ws + l.p);
    a.q = reinterpret_cast<float*>(ws + l.q);
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)l.G, (unsigned)B);
    if (hipMemsetAsync(ws, 0, l.zeroed, s) != hipSuccess) return MCAV_E_LAUNCH;
    gdc::gdc_count_kernel<<<grid, gdc::THREADS, 0, s>>>(a);
    gdc::gdc_scan_kernel<<<1, gdc::THREADS, 0, s>>>(a);
    gdc::gdc_fill_kernel<<<grid, gdc::THREADS, 0, s>>>(a);
    gdc::gdc_init_kernel<<<grid, gdc::THREADS, 0, s>>>(a);
    const int kc = k <= 4 ? 4 : k <= 8 ? 8 : k <= 12 ? 12 : 16;
    auto forward = [&](auto init) {
        constexpr bool INIT = decltype(init)::value;
        if (kc == 4) gdc::gdc_fwd_kernel<INIT, 4><<<grid, gdc::THREADS, 0, s>>>(a);
        else if (kc == 8) gdc::gdc_fwd_kernel<INIT, 8><<<grid, gdc::THREADS, 0, s>>>(a);
        else if (kc == 12) gdc::gdc_fwd_kernel<INIT, 12><<<grid, gdc::THREADS, 0, s>>>(a);
        else gdc::gdc_fwd_kernel<INIT, 16><<<grid, gdc::THREADS, 0, s>>>(a);
    };
    forward(std::true_type{});
    gdc::gdc_tr_kernel<true><<<grid, gdc::THREADS, 0, s>>>(a);
    for (int it = 0; it < iters; ++it) {
        forward(std::false_type{});
        gdc::gdc_tr_kernel<false><<<grid, gdc::THREADS, 0, s>>>(a);
        gdc::gdc_pupd_kernel<<<grid, gdc::THREADS, 0, s>>>(a);
    }
    gdc::gdc_info_kernel<<<1, 64, 0, s>>>(a);
    return launch_status();
}
