"""TEST INFRASTRUCTURE: the cases of the graph-based depth correction (tests/gdc_ref.py), shared by the CPU tests (float32 restatement vs
float64, vs csrc/gdc_math.h on the host) and the GPU tests (restatement vs the kernels).  Seeded numpy; a case's inputs and references
are computed once and are read-only.

The scene: a wall at 12 m, the ground plane y = 1.65 m and a box face at 6 m, whichever is nearest along the ray; the prediction is the
truth times a smooth 5-15 % error and 0.3 % noise; known depths sit on every second pixel of four rows (a 4-beam scanner).  Every case
exists because the kernels can go wrong there:
    scene      24 x 40, B = 2, a different K per image
    odd        23 x 37: the 16 x 16 tile divides neither side
    full       8 x 8, radius 7: the window covers the image -- exact KNN
    wide       9 x 70: tile boundaries inside a short image
    k1, k16, r1  the ends of the parameter ranges (radius 1 leaves 8 candidates for k = 10)
    wall       fronto-parallel, noise-free: many exact distance ties
    holes      NaN / +inf / 0 / beyond max_depth in blocks wider than the window: pixels with fewer than k candidates, isolated valid
               pixels that leave the graph, a known pixel on an invalid prediction, sparse values outside the range
    mixed      B = 3: the scene, an image without any known pixel, an image below min_known (= 3, with two known pixels)
SCAN_CASES, a list of its own (the GPU tests take it; the CPU suites' transcriptions and dense solves do not):
    chunks     128 x 516, B = 1: 258 workgroups of 256 pixels, more than the 256 block sums that the one-block scan takes per pass, so
               the CSR row starts of the last two workgroups carry the first pass's total
"""
import functools

import numpy as np

import gdc_ref as R

F = np.float32
CASES = ["scene", "odd", "full", "wide", "k1", "k16", "r1", "wall", "holes", "mixed"]
SCAN_CASES = ["chunks"]
HARDEST = "holes"


def intrinsics(H, W, shift=0.0):
    return np.array([0.58 * W + shift, 0.58 * W - shift, W / 2 - 0.5 + shift, 0.45 * H - shift], F)


def scene(H, W, K, seed):
    """-> truth, prediction, sparse: float32 [H, W]"""
    fx, fy, cx, cy = (float(v) for v in K)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rx, ry = (u - cx) / fx, (v - cy) / fy
    with np.errstate(divide="ignore", invalid="ignore"):
        ground = np.where(ry > 0, 1.65 / ry, np.inf)
    box = np.where((np.abs(6 * rx) < 1) & (6 * ry > 0.2) & (6 * ry < 1.65), 6.0, np.inf)
    truth = np.minimum(np.minimum(12.0, ground), box)
    rng = np.random.RandomState(seed)
    pred = truth * (1.12 + 0.04 * np.sin(u / 7) + 0.03 * np.cos(v / 5)) * (1 + 0.003 * rng.randn(H, W))
    sparse = np.zeros((H, W))
    for frac in (0.4, 0.52, 0.64, 0.8):
        row = int(np.floor(frac * H))
        sparse[row, ::2] = truth[row, ::2]
    return truth.astype(F), pred.astype(F), sparse.astype(F)


def batch(shapes_seeds, H, W):
    Ks = np.stack([intrinsics(H, W, s) for s, _ in shapes_seeds])
    parts = [scene(H, W, Ks[b], seed) for b, (_, seed) in enumerate(shapes_seeds)]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]), Ks)


@functools.lru_cache(maxsize=None)
def build(case):
    """-> dict(depth, sparse, K, truth, params) with params the keywords of gdc_ref.graph / gdc_ref.gdc"""
    params = dict(k=10, radius=3, reg=1e-3, min_depth=1e-3, max_depth=80.0)
    min_known = 1
    if case in ("scene", "k1", "k16", "r1"):
        truth, depth, sparse, K = batch([(0.0, 11), (1.25, 12)], 24, 40)
        params.update({"k1": dict(k=1), "k16": dict(k=16), "r1": dict(radius=1)}.get(case, {}))
    elif case == "odd":
        truth, depth, sparse, K = batch([(0.5, 21)], 23, 37)
    elif case == "full":
        truth, depth, sparse, K = batch([(0.0, 31), (0.75, 32)], 8, 8)
        params.update(radius=7, k=5)
    elif case == "wide":
        truth, depth, sparse, K = batch([(0.25, 41)], 9, 70)
    elif case == "wall":
        H, W = 20, 33
        K = np.stack([np.array([16.0, 16.0, 16.0, 8.0], F)])           # binary fractions: x and y are exact, so distances tie exactly
        truth = np.full((1, H, W), 8.0, F)
        depth = np.full((1, H, W), 8.5, F)
        depth[0, :, 20:] = 9.0
        sparse = np.zeros((1, H, W), F)
        sparse[0, 10, ::3] = 8.0
    elif case == "holes":
        truth, depth, sparse, K = batch([(0.0, 51), (2.0, 52)], 24, 40)
        depth = depth.copy(); sparse = sparse.copy()
        depth[0, 2:12, 3:14] = np.nan                                   # 10 x 11 hole ...
        depth[0, 7, 8] = truth[0, 7, 8]                                 # ... with an isolated valid pixel in it: leaves the graph
        sparse[0, 7, 8] = truth[0, 7, 8]                                # known, but off the graph
        depth[0, 12:22, 25:36] = np.inf
        depth[0, 16:18, 30:32] = truth[0, 16:18, 30:32]                 # a 2 x 2 island: three candidates each
        depth[1, 0:9, 0:9] = 0.0
        depth[1, 14:24, 28:40] = 90.0                                   # beyond max_depth
        depth[1, 9, 20] = -3.0
        sparse[0, 9, 4] = 7.0                                           # a known depth on an invalid prediction: not known
        assert np.isnan(depth[0, 9, 4])
        sparse[1, 9, 2:30:4] = [np.nan, np.inf, 500.0, -1.0, 1e-4, 80.0, 80.00001]       # outside the range, but for the 80.0
        sparse[1, 3, 3] = 5.0                                           # on a 0 prediction
    elif case == "chunks":
        truth, depth, sparse, K = batch([(0.0, 71)], 128, 516)
    elif case == "mixed":
        min_known = 3
        truth, depth, sparse, K = batch([(0.0, 61), (0.5, 62), (1.0, 63)], 24, 40)
        sparse = sparse.copy()
        sparse[1] = 0.0
        sparse[2] = 0.0
        sparse[2, 5, 5], sparse[2, 15, 30] = truth[2, 5, 5], truth[2, 15, 30]
    else:
        raise KeyError(case)
    out = dict(depth=np.ascontiguousarray(depth, F), sparse=np.ascontiguousarray(sparse, F), K=np.ascontiguousarray(K, F),
               truth=np.ascontiguousarray(truth, F), params=params, min_known=min_known)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def graph32(case):
    a = build(case)
    return frozen(R.graph(a["depth"], a["sparse"], a["K"], dtype=F, **a["params"]))


@functools.lru_cache(maxsize=None)
def graph64(case):
    a = build(case)
    return frozen(R.graph(a["depth"], a["sparse"], a["K"], dtype=np.float64, **a["params"]))


@functools.lru_cache(maxsize=None)
def solved32(case, iters, tol=1e-4):
    """the float32 restatement on the float32 graph -> out [B, H, W], info [B, 4]"""
    a = build(case)
    return frozen(R.gdc(a["depth"], a["sparse"], a["K"], min_known=a["min_known"], iters=iters, tol=tol, dtype=F, graph_of=graph32(case),
                        **a["params"]))


@functools.lru_cache(maxsize=None)
def solved64(case, iters, tol=1e-4):
    """float64 arithmetic on the SAME (float32) graph and weights: what separates it from solved32 is the solver's rounding alone"""
    a = build(case)
    return frozen(R.gdc(a["depth"], a["sparse"], a["K"], min_known=a["min_known"], iters=iters, tol=tol, dtype=np.float64,
                        graph_of=graph32(case), **a["params"]))


@functools.lru_cache(maxsize=None)
def dense64(case):
    """the dense float64 least-squares solution on the float32 graph, per image (passed-through images keep the prediction)"""
    a = build(case)
    nbr, w, fl = graph32(case)
    out = []
    for b in range(len(a["depth"])):
        known = int(((fl[b] & 3) == 3).sum())
        out.append(R.dense_solution(a["depth"][b], a["sparse"][b], nbr[b], w[b], fl[b]) if known >= a["min_known"]
                   else a["depth"][b].astype(np.float64))
    return frozen((np.stack(out),))[0]


def frozen(arrays):
    for v in arrays:
        v.setflags(write=False)
    return arrays


def check_non_trivial(case):
    """the case holds what its line above promises"""
    a = build(case)
    nbr, w, fl = graph32(case)
    k = a["params"]["k"]
    used = (nbr >= 0).sum(-1)
    in_graph, known = (fl & 1) != 0, (fl & 2) != 0
    assert in_graph.any() and (used[in_graph] >= 1).all() and (used[~in_graph] == 0).all()
    if case == "holes":
        assert not in_graph[0, 7, 8] and known[0, 7, 8]                 # isolated: off the graph, still flagged known
        assert (used[0, 16:18, 30:32] == 3).all()
        assert not known[0, 9, 4] and not known[1, 3, 3]
        assert known[1, 9, 2:30:4].tolist() == [False] * 5 + [True, False]
    if case == "r1":
        assert used.max() == 8 < k
    if case == "full":
        assert (used[in_graph] == k).all()
    if case == "mixed":
        assert [int((in_graph[b] & known[b]).sum()) for b in range(3)][1:] == [0, 2]
    if case == "chunks":
        B, H, W = fl.shape
        assert B * ((H * W + 255) // 256) > 256                        # B * G workgroups: a second pass of the block-sum scan
        assert in_graph[0].reshape(-1)[256 * 256:].any() and (in_graph & known).sum() > 1000
