"""TEST INFRASTRUCTURE: the cases of the box tests (tests/test_box_cpu.py, tests/test_box_gpu.py), built from seeds, with their reference
results computed once per process (tests/box_ref.py) and shared.

PAIRS: a few thousand box pairs by family (pair_family(name) -> (a, b) float32 [n, 7]).
CASES: the suppression cases, the smallest shapes at which the kernels can go wrong; build(name) -> the arguments of box_ref.nms /
mcav_box_nms as a dict.  Candidates come in CLUSTERS around well separated objects: a cluster's members overlap each other far above
every threshold used (jitter of a few centimetres and hundredths of a radian: iou above 0.6), different objects do not overlap at all
(iou exactly 0 in both arithmetics: the circle test), so no pair comes near a threshold and the float64 rule keeps the restatement's
rows: check_non_trivial(name) asserts exactly that, with no pair excluded."""
import functools

import numpy as np

import box_ref as R

F = np.float32
PI = np.pi


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    assert np.array_equal(ua, ub), "%d of %d words differ, first at %s" % ((ua != ub).sum(), ua.size, np.argwhere(ua != ub)[:1].tolist())


# ---------------------------------------------------------------------------------------------- pairs
def random_boxes(rng, n, x=(0.0, 70.0), size=(1.0, 6.0, 0.5, 2.5)):
    b = np.empty((n, 7), F)
    b[:, 0], b[:, 1], b[:, 2] = rng.uniform(x[0], x[1], n), rng.uniform(-40, 40, n), rng.uniform(-2.5, 0.5, n)
    b[:, 3], b[:, 4], b[:, 5] = rng.uniform(size[0], size[1], n), rng.uniform(size[2], size[3], n), rng.uniform(1.0, 3.0, n)
    b[:, 6] = rng.uniform(-PI, PI, n)
    return b


def near(rng, a, reach=0.8):
    """a second box for every row of a: its own sizes and heading, the centre within `reach` of the sum of the half-diagonals"""
    b = random_boxes(rng, len(a))
    b[:, 3:5] = a[:, 3:5] * rng.uniform(0.5, 1.5, (len(a), 2)).astype(F)
    R_ = (np.hypot(a[:, 3], a[:, 4]) + np.hypot(b[:, 3], b[:, 4])) / 2
    phi, rad = rng.uniform(0, 2 * PI, len(a)), R_ * reach * np.sqrt(rng.uniform(0, 1, len(a)))
    b[:, 0], b[:, 1] = a[:, 0] + rad * np.cos(phi), a[:, 1] + rad * np.sin(phi)
    b[:, 2] = a[:, 2] + rng.uniform(-1, 1, len(a))
    return b


def rotated(v, h):
    c, s = np.cos(h.astype(np.float64)), np.sin(h.astype(np.float64))
    return v[0] * c - v[1] * s, v[0] * s + v[1] * c


INVALID = [(0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.nan), (5, np.nan), (6, np.nan), (6, np.inf), (3, 0.0), (4, -1.0),
           (5, 0.0), (3, 5e-4), (4, 1e-30), (5, 2000.0), (3, 1025.0), (3, np.inf), (6, 32.000004), (6, -33.0), (6, 1e30), (1, -np.inf)]
PAIR_FAMILIES = ("random", "wide-heading", "identical", "quarter-turns", "shared-edge", "touching-corner", "inside", "axis-aligned",
                 "cm-against-50m", "heading-limit", "far-small", "invalid")


@functools.lru_cache(maxsize=None)
def pair_family(name):
    rng = np.random.RandomState(1000 + PAIR_FAMILIES.index(name))
    if name == "random":
        a = random_boxes(rng, 1500)
        return a, near(rng, a, 1.1)
    if name == "wide-heading":
        a = random_boxes(rng, 300)
        b = near(rng, a)
        a[:, 6], b[:, 6] = rng.uniform(-8 * PI, 8 * PI, 300), rng.uniform(-32, 32, 300)
        return a, b
    if name == "identical":
        a = random_boxes(rng, 150)
        return a, a.copy()
    if name == "quarter-turns":
        a = random_boxes(rng, 200)
        b = a.copy()
        b[:, 6] = (a[:, 6].astype(np.float64) + rng.randint(-7, 8, 200) * (PI / 2)).astype(F)
        return a, b
    if name in ("shared-edge", "touching-corner"):
        a = random_boxes(rng, 150)
        b = a.copy()
        off = (a[:, 3].astype(np.float64), 0.0 * a[:, 4] if name == "shared-edge" else a[:, 4].astype(np.float64))
        ox, oy = rotated(off, a[:, 6])
        b[:, 0], b[:, 1] = a[:, 0] + ox, a[:, 1] + oy
        return a, b
    if name == "inside":
        a = random_boxes(rng, 150)
        b = random_boxes(rng, 150)
        b[:, :3] = a[:, :3] + rng.uniform(-0.05, 0.05, (150, 3)).astype(F)
        b[:, 3:6] = a[:, 3:6] * F(0.3)
        return a, b
    if name == "axis-aligned":
        a = random_boxes(rng, 300)
        b = near(rng, a)
        a[:, 6] = b[:, 6] = 0.0
        return a, b
    if name == "cm-against-50m":
        a, b = random_boxes(rng, 100), random_boxes(rng, 100)
        a[:, 3:5], b[:, 3:5] = 0.01, 50.0
        b[:, :2] = a[:, :2] + rng.uniform(-30, 30, (100, 2)).astype(F)
        half = slice(0, 50)
        a[half], b[half] = b[half].copy(), a[half].copy()
        return a, b
    if name == "heading-limit":
        a = random_boxes(rng, 60)
        b = near(rng, a, 0.5)
        a[:, 6] = np.where(np.arange(60) % 2, F(32.0), F(-32.0))
        b[:30, 6] = np.nextafter(F(32.0), F(0.0))
        return a, b
    if name == "far-small":                                   # where a clip that does not translate to A's centre loses its digits
        a = random_boxes(rng, 300, x=(60.0, 70.0), size=(0.05, 0.3, 0.05, 0.3))
        return a, near(rng, a, 0.6)
    if name == "invalid":
        a = random_boxes(rng, 2 * len(INVALID))
        b = near(rng, a, 0.2)
        for k, (col, value) in enumerate(INVALID):
            a[2 * k, col] = value                            # against a valid box, and against itself
            b[2 * k + 1] = a[2 * k + 1] = a[2 * k]
        return a, b
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def pair_reference(name, mode):
    """-> (inter, iou) of the restatement and the float64 formulation's dict, computed once"""
    a, b = pair_family(name)
    return R.pairs_iou(a, b, mode), R.iou_f64(a, b, mode)


@functools.lru_cache(maxsize=None)
def iou_matrix_operands():
    """a [130, 7], b [77, 7]: no multiples of the kernel's 64 x 64 tile; crowded enough that hundreds of pairs overlap, b holds rows of a,
    both hold invalid rows"""
    rng = np.random.RandomState(77)
    a, b = random_boxes(rng, 130, x=(0.0, 25.0)), random_boxes(rng, 77, x=(0.0, 25.0))
    a[:, 1], b[:, 1] = a[:, 1] / 4, b[:, 1] / 4
    b[:40] = near(rng, a[:40], 0.5)
    b[40:50] = a[100:110]
    for k, (col, value) in enumerate(INVALID[:8]):
        a[16 * k + 3, col] = value
        b[9 * k + 1, col] = value
    return a, b


@functools.lru_cache(maxsize=None)
def iou_matrix_reference(mode):
    return R.iou_matrix(*iou_matrix_operands(), mode)


# ---------------------------------------------------------------------------------------------- suppression cases
def cluster(rng, centre, members, stacked=False):
    """`members` boxes around one object at centre (x, y): jitter of centimetres, so every pair overlaps far above 0.5"""
    base = np.array([centre[0], centre[1], rng.uniform(-1.2, -0.8), rng.uniform(3.6, 4.4), rng.uniform(1.6, 2.0), rng.uniform(1.4, 1.7),
                     rng.uniform(-PI, PI)])
    out = np.tile(base, (members, 1))
    out[:, :2] += rng.uniform(-0.04, 0.04, (members, 2))
    out[:, 2] += rng.uniform(-0.02, 0.02, members)
    out[:, 3:6] *= rng.uniform(0.98, 1.02, (members, 3))
    out[:, 6] += rng.uniform(-0.015, 0.015, members)
    if stacked:
        out[1::2, 2] += 4.0                                   # the same footprint one floor up: overlaps in the bird's-eye view only
    return out.astype(F)


def grid_centres(rng, n, spacing=9.0):
    side = int(np.ceil(np.sqrt(n)))
    cells = rng.permutation(side * side)[:n]
    return np.stack([(cells % side) * spacing, (cells // side) * spacing - side * spacing / 2], 1)


SPEC = {
    # name: sizes of the candidate clusters in the order walked (an int n: n clusters of 3), and the call's arguments
    "count-0": dict(groups=[], A=70, iou_thresh=0.1),
    "count-1": dict(groups=[1], A=70, iou_thresh=0.5),
    "count-63": dict(groups=[3] * 21, A=200, iou_thresh=0.01),
    "count-64": dict(groups=[3] * 21 + [1], A=200, iou_thresh=0.1),
    "count-65-3d": dict(groups=[3] * 21 + [2], A=333, iou_thresh=0.1, mode="3d"),
    "count-129-post-30": dict(groups=[3] * 43, A=300, iou_thresh=0.5, post_max=30),
    "cut-4096-ties": dict(groups=[3] * 1700, A=6001, iou_thresh=0.1, quantised=50, pre_max=4096, post_max=4096),
    "batch-3-empty-middle": dict(groups=[3] * 30, A=257, iou_thresh=0.01, B=3, empty=(1,)),
    "chain-over-chunk": dict(groups=[3] * 20 + [1, 1, "i", 1, "j", 1, "k"] + [3] * 10, A=160, iou_thresh=0.1, chain=True),
    "zeros-and-nans": dict(groups=[3] * 8, A=90, iou_thresh=0.1, score_thresh=0.0, zeros=True),
    "invalid-on-top": dict(groups=[3] * 12, A=120, iou_thresh=0.5, invalid=True),
    "classes": dict(groups=[3] * 25, A=150, iou_thresh=0.1, classes=True, B=2),
    "stacked-3d": dict(groups=[3] * 20, A=130, iou_thresh=0.1, mode="3d", stacked=True),
    "stacked-bev": dict(groups=[3] * 20, A=130, iou_thresh=0.1, stacked=True),
    "radix-20000": dict(groups=[3] * 2000, A=20000, iou_thresh=0.5, pre_max=3000, post_max=500),
}
CASES = tuple(SPEC)
HARDEST = "cut-4096-ties"
CHAIN_X = (0.0, 2.0, 4.0)                                     # i, j, k along x, 3.9 m long: i-j and j-k overlap (iou 0.32), i-k do not


@functools.lru_cache(maxsize=None)
def build(name):
    spec = SPEC[name]
    rng = np.random.RandomState(2000 + CASES.index(name))
    B, A = spec.get("B", 1), spec["A"]
    score_thresh = spec.get("score_thresh", 0.1)
    boxes, scores = np.empty((B, A, 7), F), np.empty((B, A), F)
    classes = np.zeros((B, A), np.int32) if spec.get("classes") else None
    chain = {}
    for b in range(B):
        groups = [] if b in spec.get("empty", ()) else spec["groups"]
        centres = grid_centres(rng, len(groups) + 1)
        rows, cls = [], []
        for g, size in enumerate(groups):
            if isinstance(size, str):
                row = np.array([[500.0 + CHAIN_X["ijk".index(size)], -200.0, -1.0, 3.9, 1.8, 1.5, 0.0]], F)
                chain[size] = len(np.concatenate(rows)) if rows else 0
                rows.append(row)
            else:
                rows.append(cluster(rng, centres[g], size, spec.get("stacked", False)))
            cls += [0, 0, 1, 1][:len(rows[-1])]
        cand = np.concatenate(rows) if rows else np.zeros((0, 7), F)
        n = len(cand)
        assert n <= A - 8
        if spec.get("quantised"):
            s = 0.3 + rng.randint(0, spec["quantised"], n) / 100.0
        elif spec.get("chain"):
            s = 0.95 - 0.004 * np.arange(n)                   # the order walked is the order built
        elif spec.get("zeros"):
            s = np.where(np.arange(n) % 3 == 0, 0.5, np.where(np.arange(n) % 3 == 1, -0.0, 0.0))
        else:
            s = rng.uniform(0.15, 0.95, n)
        # the rest: boxes on top of the candidates whose scores do not pass, NaN scores, and (where asked) invalid boxes with high scores
        rest = A - n
        filler = random_boxes(rng, rest, x=(0.0, 60.0))
        if n:
            filler[:rest // 2] = cand[rng.randint(0, n, rest // 2)]
        fs = rng.uniform(-1.0, score_thresh - 0.05, rest) if score_thresh > 0 else rng.uniform(-1.0, -0.01, rest)
        fs[::5] = np.nan
        if spec.get("invalid"):
            for k, (col, value) in enumerate(INVALID[:rest - 2]):
                filler[k, col], fs[k] = value, 0.99
        perm = rng.permutation(A)
        boxes[b, perm], scores[b, perm] = np.concatenate([cand, filler]), np.concatenate([s, fs]).astype(F)
        if classes is not None:
            classes[b, perm] = np.concatenate([np.array(cls, np.int32), rng.randint(0, 2, rest).astype(np.int32)])
        if chain and "at" not in chain:
            chain["at"] = {key: int(perm[v]) for key, v in chain.items()}
    return dict(boxes=boxes, scores=scores, classes=classes, score_thresh=score_thresh, iou_thresh=spec["iou_thresh"],
                pre_max=spec.get("pre_max", 4096), post_max=spec.get("post_max", 500), mode=spec.get("mode", "bev"), chain=chain.get("at"))


def call_args(case):
    a = dict(build(case))
    a.pop("chain")
    return a


@functools.lru_cache(maxsize=None)
def reference(case):
    return R.nms(**call_args(case))


@functools.lru_cache(maxsize=None)
def reference_f64(case):
    return R.nms(f64=True, **call_args(case))


@functools.lru_cache(maxsize=None)
def check_non_trivial(case):
    """conditions, not tolerances: no candidate pair's float64 iou within 4 x the bound of the threshold (no pair excluded), a third of the
    candidates kept and a third suppressed where there are six or more, the chain where the case has one, the cut where it has one"""
    a, spec = build(case), SPEC[case]
    want = reference(case)
    thresh = float(F(a["iou_thresh"]))
    for b in range(a["scores"].shape[0]):
        order = R.order_of(a["boxes"][b], a["scores"][b], a["score_thresh"], a["pre_max"])
        i, j, value, bound = R.overlaps(a["boxes"][b], order, a["mode"], f64=True)
        assert not (np.abs(value - thresh) <= 4 * bound).any(), (case, b)
        n, kept = len(order), int(want["num"][b])
        groups = [] if b in spec.get("empty", ()) else spec["groups"]
        assert n == min(sum(g if isinstance(g, int) else 1 for g in groups), a["pre_max"]), (case, n)
        if "post_max" in spec and a["post_max"] < 4096:
            last = order.tolist().index(int(want["keep"][b, kept - 1]))
            assert kept == a["post_max"] and last % 64 < 63 and last + 1 < n, (case, kept, last)  # reached in the middle of a chunk
        elif n >= 6:
            assert 3 * kept >= n and 3 * (n - kept) >= n, (case, n, kept)
        if spec.get("quantised") or case == "radix-20000":
            with np.errstate(invalid="ignore"):
                cands = int((R.valid(a["boxes"][b]) & (a["scores"][b] >= F(a["score_thresh"]))).sum())
            assert cands > a["pre_max"] == n
        if spec.get("quantised"):
            s = a["scores"][b]
            inside, level = set(order.tolist()), s[order[-1]]
            same = np.nonzero(s == level)[0]
            assert 0 < sum(int(k) in inside for k in same) < len(same)                          # equal scores straddle the cut
            assert max(k for k in same if int(k) in inside) < min(k for k in same if int(k) not in inside)
    if a["chain"]:
        at, keep = a["chain"], want["keep"][0, :want["num"][0]].tolist()
        order = R.order_of(a["boxes"][0], a["scores"][0], a["score_thresh"], a["pre_max"]).tolist()
        pi, pj, pk = (order.index(at[key]) for key in "ijk")
        assert pi < 64 <= pj < pk and at["i"] in keep and at["j"] not in keep and at["k"] in keep
        trio = a["boxes"][0][[at["i"], at["j"], at["k"]]]
        v = R.iou_f64(trio[[0, 1, 0]], trio[[1, 2, 2]], a["mode"])["iou"]
        assert v[0] > thresh and v[1] > thresh and v[2] == 0.0
    return True
