"""TEST INFRASTRUCTURE: the definition of the graph-based depth correction (Pseudo-LiDAR++ GDC; include/mcav_depth.h: mcav_gdc_graph,
mcav_gdc_solve; pseudo_lidar.gdc) in numpy.  Every function takes the working dtype: float32 is the restatement the kernels and
csrc/gdc_math.h are held against (one operation per rounding, in the order written here), float64 is the arbiter.

    inputs   depth, sparse [B, H, W] float32 on one grid, K [B, 4] = (fx, fy, cx, cy) of that grid
    valid    min_depth < depth <= max_depth, compared as floats (NaN and +-inf drop out)
    known    valid and min_depth < sparse <= max_depth
    point    X = ((u - cx) / fx * z, (v - cy) / fy * z, z)
    graph    candidates of pixel i: the valid j != i of the (2 radius + 1)^2 window around it (clipped) whose squared distance
             ((dx dx + dy dy) + dz dz) is below +inf; neighbours: the min(k, #candidates) smallest, ties to the lower pixel index, stored
             in ascending (distance, index) order; nbr = v * W + u of the neighbour, -1 in the unused slots, whose weight is +0.0.
             A valid pixel with a candidate is a graph pixel (flags bit 0); bit 1 marks a known pixel, in the graph or not.
    weights  d_j = z_j - z_i; s = sum d_j, q = sum d_j d_j in neighbour order; lam = reg q if q > 0 else reg; t = s / (lam + q);
             w'_j = 1 - d_j t; w_j = w'_j / sum w'_j (sklearn.manifold.barycenter_weights on the scalar depths, through Sherman-Morrison)
    solve    M = I - W over the graph pixels; z' = sparse on the known graph pixels L, minimise |M z'|^2 over the others U by conjugate
             gradient on the normal equations from z'_U = depth_U: r = -(M^T M z')_U, p = r, rs = |r|^2;
               q = M p; den = |q|^2; alpha = rs / den; x += alpha p; r -= alpha (M^T q)_U; rs' = |r|^2; beta = rs' / rs; p = r + beta p
             inner products in float64, alpha and beta rounded to the working dtype; (M v)_i = v_i - sum_slots w v_j in neighbour order
             from +0; (M^T q)_j = q_j - sum over the sources that list j, in ascending source order from +0, of w q_source.
             An image is done once rs <= tol^2 rs0 or rs is not positive (after an iteration, or at the start), or when den is not
             positive (that iteration is not run or counted); at most `iters` iterations.
    output   out = z' on graph pixels, the input's bits elsewhere; an image with fewer than min_known known graph pixels is passed
             through unchanged; info [B, 4] = (graph pixels, known graph pixels, iterations run, rs / rs0): (.., .., 0, 1) for a
             passed-through image, rs / rs0 = 0 where rs0 is not positive.
"""
import numpy as np

F = np.float32
D = np.float64


def valid_mask(z, min_depth, max_depth):
    z = np.asarray(z, F)
    with np.errstate(invalid="ignore"):
        return (z > F(min_depth)) & (z <= F(max_depth))


def points(depth, K, dtype=F):
    """[H, W] depth, (fx, fy, cx, cy) -> x, y, z [H, W] in dtype, every quotient and product rounded on its own"""
    H, W = depth.shape
    fx, fy, cx, cy = (dtype(F(v)) for v in K)
    z = np.asarray(depth, F).astype(dtype)
    u = np.arange(W, dtype=dtype)[None, :]
    v = np.arange(H, dtype=dtype)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = ((u - cx) / fx) * z
        y = ((v - cy) / fy) * z
    return x.astype(dtype), y.astype(dtype), z


def window_offsets(radius):
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def graph_image(depth, sparse, K, k=10, radius=3, reg=1e-3, min_depth=1e-3, max_depth=80.0, dtype=F):
    """one image -> nbr int32 [H, W, k], weights dtype [H, W, k], flags uint8 [H, W]"""
    depth, sparse = np.asarray(depth, F), np.asarray(sparse, F)
    H, W = depth.shape
    ok = valid_mask(depth, min_depth, max_depth)
    known = ok & valid_mask(sparse, min_depth, max_depth)
    x, y, z = points(depth, K, dtype)
    offs = window_offsets(radius)
    d2 = np.full((H, W, len(offs)), np.inf, dtype)
    idx = np.full((H, W, len(offs)), -1, np.int64)
    vv, uu = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore", over="ignore"):
        for c, (dy, dx) in enumerate(offs):                   # raster order = ascending pixel index
            v2, u2 = vv + dy, uu + dx
            inside = (v2 >= 0) & (v2 < H) & (u2 >= 0) & (u2 < W)
            v2c, u2c = np.clip(v2, 0, H - 1), np.clip(u2, 0, W - 1)
            ex, ey, ez = x[v2c, u2c] - x, y[v2c, u2c] - y, z[v2c, u2c] - z
            dist = (ex * ex + ey * ey) + ez * ez
            cand = inside & ok & ok[v2c, u2c] & (dist < np.inf)
            d2[:, :, c] = np.where(cand, dist, np.inf)
            idx[:, :, c] = np.where(cand, v2c * W + u2c, -1)
    order = np.argsort(d2, axis=2, kind="stable")[:, :, :k]    # stable: ties to the lower index
    nb = np.take_along_axis(idx, order, axis=2)
    if nb.shape[2] < k:
        nb = np.concatenate([nb, np.full((H, W, k - nb.shape[2]), -1, np.int64)], axis=2)
    used = nb >= 0
    in_graph = used[:, :, 0]
    zf = z.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(used, zf[np.where(used, nb, 0)] - z[:, :, None], dtype(0)).astype(dtype)
    w = closed_form_weights(d, used, reg, dtype)
    flags = in_graph.astype(np.uint8) | (known.astype(np.uint8) << 1)
    return nb.astype(np.int32), w, flags


def closed_form_weights(d, used, reg, dtype=F):
    """d [..., k] = z_j - z_i (0 in unused slots), used [..., k] -> the weights, 0 in unused slots; sums in slot order from +0"""
    k = d.shape[-1]
    s = np.zeros(d.shape[:-1], dtype)
    q = np.zeros(d.shape[:-1], dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(k):
            s = np.where(used[..., j], s + d[..., j], s)
            q = np.where(used[..., j], q + d[..., j] * d[..., j], q)
        lam = np.where(q > 0, dtype(F(reg)) * q, dtype(F(reg))).astype(dtype)
        t = s / (lam + q)
        wp = np.where(used, dtype(1) - d * t[..., None], dtype(0)).astype(dtype)
        tot = np.zeros(d.shape[:-1], dtype)
        for j in range(k):
            tot = np.where(used[..., j], tot + wp[..., j], tot)
        w = np.where(used, wp / np.where(used[..., :1], tot[..., None], dtype(1)), dtype(0))
    return w.astype(dtype)


def general_weights(d_row, reg):
    """sklearn.manifold.barycenter_weights for one row of m scalar differences, float64: C = d d^T + lam I, w = C^-1 1 / sum"""
    d_row = np.asarray(d_row, D)
    m = len(d_row)
    C = np.outer(d_row, d_row)
    trace = np.trace(C)
    C[np.diag_indices(m)] += D(F(reg)) * trace if trace > 0 else D(F(reg))
    w = np.linalg.solve(C, np.ones(m))
    return w / w.sum()


def check_closed_form(d, used, reg, rows=None, bound=1e-8):
    """the closed form in float64 against the general solve on the given rows (all by default); -> the largest relative difference"""
    w = closed_form_weights(np.asarray(d, D), used, reg, D).reshape(-1, d.shape[-1])
    dd, uu = np.asarray(d, D).reshape(-1, d.shape[-1]), used.reshape(-1, d.shape[-1])
    worst = 0.0
    for i in (range(len(dd)) if rows is None else rows):
        m = int(uu[i].sum())
        if m == 0:
            continue
        g = general_weights(dd[i, :m], reg)
        worst = max(worst, float(np.abs(g - w[i, :m]).max() / np.abs(g).max()))
    assert worst <= bound, worst
    return worst


def graph(depth, sparse, K, dtype=F, **kw):
    """batch form -> nbr [B, H, W, k], weights, flags"""
    out = [graph_image(depth[b], sparse[b], K[b], dtype=dtype, **kw) for b in range(len(depth))]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def brute_force_knn(depth, K, k, min_depth=1e-3, max_depth=80.0, dtype=F):
    """exact KNN over the whole image, ties to the lower index -> nbr int32 [H, W, k]"""
    H, W = depth.shape
    ok = valid_mask(depth, min_depth, max_depth).reshape(-1)
    x, y, z = (a.reshape(-1) for a in points(np.asarray(depth, F), K, dtype))
    nb = np.full((H * W, k), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in np.flatnonzero(ok):
            ex, ey, ez = x - x[i], y - y[i], z - z[i]
            dist = (ex * ex + ey * ey) + ez * ez
            dist = np.where(ok & (dist < np.inf), dist, np.inf)
            dist[i] = np.inf
            order = np.argsort(dist, kind="stable")[:k]
            order = order[dist[order] < np.inf]
            nb[i, :len(order)] = order
    return nb.reshape(H, W, k)


class Operator:
    """M = I - W of one image over its graph pixels, with the two products in the definition's summation orders"""

    def __init__(self, nbr, weights, flags, dtype=F):
        self.dtype = dtype
        self.k = nbr.shape[-1]
        self.nbr = nbr.reshape(-1, self.k).astype(np.int64)
        self.w = np.asarray(weights).reshape(-1, self.k).astype(dtype)
        fl = flags.reshape(-1)
        self.graph = (fl & 1) != 0
        self.known = self.graph & ((fl & 2) != 0)
        self.unknown = self.graph & ~self.known
        self.used = self.nbr >= 0
        src, slot = np.nonzero(self.used & self.graph[:, None])
        tgt = self.nbr[src, slot]
        order = np.lexsort((src, tgt))                       # by target, then ascending source
        self.t_src, self.t_slot, self.t_tgt = src[order], slot[order], tgt[order]
        start = np.searchsorted(self.t_tgt, self.t_tgt, side="left")
        self.t_rank = np.arange(len(order)) - start
        self.max_in = int(self.t_rank.max()) + 1 if len(order) else 0

    def forward(self, v):
        acc = np.zeros(len(v), self.dtype)
        for s in range(self.k):
            u = self.used[:, s] & self.graph
            acc = np.where(u, acc + self.w[:, s] * v[np.where(u, self.nbr[:, s], 0)], acc).astype(self.dtype)
        return np.where(self.graph, v - acc, self.dtype(0)).astype(self.dtype)

    def transposed(self, q):
        acc = np.zeros(len(q), self.dtype)
        for r in range(self.max_in):
            m = self.t_rank == r
            t = self.t_tgt[m]
            acc[t] = acc[t] + self.w[self.t_src[m], self.t_slot[m]] * q[self.t_src[m]]
        return np.where(self.graph, q - acc, self.dtype(0)).astype(self.dtype)

    def dense(self):
        n = len(self.graph)
        M = np.zeros((n, n), D)
        g = np.flatnonzero(self.graph)
        M[g, g] = 1.0
        src, slot = np.nonzero(self.used & self.graph[:, None])
        M[src, self.nbr[src, slot]] -= self.w[src, slot].astype(D)
        return M


def dot64(a):
    return float(np.sum(np.asarray(a, D) ** 2))


def solve_image(depth, sparse, nbr, weights, flags, min_known=1, iters=400, tol=1e-4, dtype=F):
    """one image -> out [H, W] (dtype; the bits of `depth` off the graph), info (graph, known, iterations, rs / rs0)"""
    op = Operator(nbr, weights, flags, dtype)
    n_graph, n_known = int(op.graph.sum()), int(op.known.sum())
    out = np.asarray(depth, F).astype(dtype).reshape(-1).copy()
    if n_known < int(min_known):
        return out.reshape(depth.shape), (n_graph, n_known, 0, 1.0)
    x = out.copy()
    x[op.known] = np.asarray(sparse, F).reshape(-1)[op.known].astype(dtype)
    U = op.unknown
    zero = np.zeros(len(x), dtype)
    vec = np.where(op.graph, x, dtype(0)).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(U, -op.transposed(op.forward(vec)), zero).astype(dtype)
        p = r.copy()
        rs0 = rs = dot64(r)
        thresh = D(F(tol)) * D(F(tol)) * rs0
        it = 0
        done = not (rs0 > 0) or rs <= thresh
        while not done and it < int(iters):
            q = op.forward(p)
            den = dot64(q)
            if not den > 0:
                break
            alpha = dtype(rs / den)
            vec = np.where(U, vec + alpha * p, vec).astype(dtype)
            r = np.where(U, r - alpha * op.transposed(q), zero).astype(dtype)
            rs_new = dot64(r)
            beta = dtype(rs_new / rs)
            rs = rs_new
            it += 1
            if rs <= thresh or not (rs > 0):
                break
            p = np.where(U, r + beta * p, zero).astype(dtype)
    out = np.where(op.graph, vec, out).astype(dtype)
    return out.reshape(depth.shape), (n_graph, n_known, it, rs / rs0 if rs0 > 0 else 0.0)


def gdc(depth, sparse, K, k=10, radius=3, reg=1e-3, min_depth=1e-3, max_depth=80.0, min_known=1, iters=400, tol=1e-4, dtype=F, graph_of=None):
    """batch form -> out [B, H, W] dtype, info float64 [B, 4]; graph_of: a (nbr, weights, flags) to solve on instead of building one"""
    nbr, w, fl = graph(depth, sparse, K, dtype=dtype, k=k, radius=radius, reg=reg, min_depth=min_depth, max_depth=max_depth) \
        if graph_of is None else graph_of
    res = [solve_image(depth[b], sparse[b], nbr[b], w[b], fl[b], min_known, iters, tol, dtype) for b in range(len(depth))]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], D)


def dense_solution(depth, sparse, nbr, weights, flags):
    """the float64 least-squares solution of one image through numpy's lstsq on the dense operator -> out [H, W] float64"""
    op = Operator(nbr, weights, flags, D)
    M = op.dense()
    z = np.asarray(depth, F).astype(D).reshape(-1).copy()
    z[op.known] = np.asarray(sparse, F).reshape(-1)[op.known].astype(D)
    U, Lk, G = np.flatnonzero(op.unknown), np.flatnonzero(op.known), np.flatnonzero(op.graph)
    if len(U) and len(Lk):
        A = M[np.ix_(G, U)]
        b = -M[np.ix_(G, Lk)] @ z[Lk]
        z[U] = np.linalg.lstsq(A, b, rcond=None)[0]
    return z.reshape(depth.shape)
