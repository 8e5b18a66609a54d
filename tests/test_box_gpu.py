"""GPU: oriented-box overlap and batched suppression (include/mcav_depth.h: mcav_box_iou, mcav_box_nms; pseudo_lidar.boxes_iou_bev,
boxes_iou3d, nms, DetectionBatch) against the restatement (tests/box_ref.py), bit for bit, on the pairs and cases of tests/box_cases.py:
the IoU matrix in both modes at sizes that are no multiple of the tile; keep, num and the gathered rows of every suppression case between
sentinel bands and starting as sentinels, equal to the float64 rule's kept sets, a second run, the variants without classes and without
gathered outputs; graph capture with out= and a replay on new contents; split(); per-class scores; the suppression behind a pseudo-image
and a stub head; the C ABI's and the Python side's refusals."""
import numpy as np
import pytest
import torch

import box_cases as C
import box_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -7.0
INT_SENTINEL = -12345
GUARD = 64                                                   # elements in front of and behind a guarded buffer: 256 bytes


def dev(v, dtype=None):
    return torch.from_numpy(np.array(v, dtype or v.dtype)).to(DEV)


def guarded(shape, dtype, fill):
    """-> (a contiguous view of `shape` inside a buffer with GUARD elements of `fill` on either side, the whole buffer)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n].view(shape), whole


def guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def holder(B, post_max, fill=SENTINEL):
    """a DetectionBatch whose four outputs sit between guards, full of sentinels -> (batch, [(whole buffer, its fill)])"""
    from pseudo_lidar import DetectionBatch
    db = DetectionBatch(B, post_max, DEV)
    db.keep, wk = guarded((B, post_max), torch.int32, INT_SENTINEL)
    db.num, wn = guarded((B,), torch.int32, INT_SENTINEL)
    db.boxes, wb = guarded((B, post_max, 7), torch.float32, fill)
    db.scores, wsc = guarded((B, post_max), torch.float32, fill)
    return db, [(wk, INT_SENTINEL), (wn, INT_SENTINEL), (wb, fill), (wsc, fill)]


def on_device(a):
    return dict(boxes=dev(a["boxes"]), scores=dev(a["scores"]), classes=None if a["classes"] is None else dev(a["classes"]),
                score_thresh=a["score_thresh"], iou_thresh=a["iou_thresh"], pre_max=a["pre_max"], post_max=a["post_max"], iou=a["mode"])


def check(db, want):
    assert np.array_equal(db.keep.cpu().numpy(), want["keep"]) and np.array_equal(db.num.cpu().numpy(), want["num"])
    C.same_bits(db.boxes.cpu().numpy(), want["boxes"])       # every element written: no sentinel is left, +0.0 behind the count
    C.same_bits(db.scores.cpu().numpy(), want["scores"])


# ---------------------------------------------------------------------------------------------- the IoU matrix
@pytest.mark.parametrize("mode", ["bev", "3d"])
def test_iou_matrix_matches_restatement(mode):
    from pseudo_lidar import boxes_iou3d, boxes_iou_bev
    fn = boxes_iou_bev if mode == "bev" else boxes_iou3d
    a, b = C.iou_matrix_operands()                           # 130 x 77: three row tiles, two column tiles, ragged ends
    got = fn(dev(a), dev(b))
    C.same_bits(got.cpu().numpy(), C.iou_matrix_reference(mode))
    C.same_bits(fn(dev(a[:1]), dev(b[:64])).cpu().numpy(), C.iou_matrix_reference(mode)[:1, :64])
    assert tuple(fn(dev(a[:0]), dev(b)).shape) == (0, 77)
    for family in ("identical", "quarter-turns", "cm-against-50m", "heading-limit", "invalid"):
        pa, pb = C.pair_family(family)
        (_, iou), _ = C.pair_reference(family, mode)
        C.same_bits(torch.diagonal(fn(dev(pa), dev(pb))).cpu().numpy().copy(), iou)


def test_iou_matrix_stays_inside_its_buffer():
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401
    a, b = C.iou_matrix_operands()
    out, whole = guarded((len(a), len(b)), torch.float32, SENTINEL)
    da, db_ = dev(a), dev(b)
    assert L.lib().mcav_box_iou(L.ptr(da), len(a), L.ptr(db_), len(b), 0, L.ptr(out), L.stream()) == 0
    C.same_bits(out.cpu().numpy(), C.iou_matrix_reference("bev"))
    assert guards_intact(whole, SENTINEL)
    for bad in (dict(a=None), dict(out=None), dict(na=-1), dict(mode=2), dict(b=L.c_p(db_.data_ptr() + 2))):
        arg = dict(a=L.ptr(da), na=len(a), b=L.ptr(db_), nb=len(b), mode=0, out=L.ptr(out))
        arg.update(bad)
        out.fill_(SENTINEL)
        assert L.lib().mcav_box_iou(arg["a"], arg["na"], arg["b"], arg["nb"], arg["mode"], arg["out"], L.stream()) == -1, bad
        assert bool((whole == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- every suppression case
@pytest.mark.parametrize("case", C.CASES)
def test_nms_matches_restatement_and_float64_rule(case):
    from pseudo_lidar import nms
    C.check_non_trivial(case)
    a, want = C.call_args(case), C.reference(case)
    B = a["scores"].shape[0]
    kw = on_device(a)
    db, wholes = holder(B, a["post_max"])
    assert nms(out=db, **kw) is db
    check(db, want)
    assert all(guards_intact(w, fill) for w, fill in wholes)
    assert np.array_equal(db.keep.cpu().numpy(), C.reference_f64(case)["keep"])                # the float64 rule keeps the same rows
    assert db.counts().tolist() == want["num"].tolist() and db.labels is None

    second, wholes2 = holder(B, a["post_max"], fill=float("nan"))                              # other buffers, another workspace
    nms(out=second, **kw)
    for name in ("keep", "num", "boxes", "scores"):
        x, y = getattr(second, name), getattr(db, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert all(guards_intact(w, fill) or fill != fill for w, fill in wholes2)
    nms(out=db, **kw)                                                                          # the same buffers and workspace again
    check(db, want)

    for b, part in enumerate(db.split()):
        n = int(want["num"][b])
        assert part["keep"].cpu().numpy().tolist() == want["keep"][b, :n].tolist() and part["labels"] is None
        C.same_bits(part["boxes"].cpu().numpy(), want["boxes"][b, :n])
        C.same_bits(part["scores"].cpu().numpy(), want["scores"][b, :n])


@pytest.mark.parametrize("case", ["classes", "count-65-3d"])
def test_null_variants_of_the_c_call(case):
    """the C entry without classes, without out_boxes, without out_scores: the outputs that are there hold the restatement's bytes, and
    the workspace between its own guards is enough"""
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401
    a = C.call_args(case)
    B, A = a["scores"].shape
    boxes, scores = dev(a["boxes"]), dev(a["scores"])
    classes = None if a["classes"] is None else dev(a["classes"])
    nbytes = L.lib().mcav_box_nms_workspace_bytes(B, A, a["pre_max"])
    for drop in ((), ("classes",), ("out_boxes",), ("out_scores",), ("classes", "out_boxes", "out_scores")):
        want = R.nms(**dict(a, classes=None)) if "classes" in drop else C.reference(case)
        db, wholes = holder(B, a["post_max"])
        ws, whole_ws = guarded((nbytes,), torch.uint8, 0xA5)
        rc = L.lib().mcav_box_nms(L.ptr(boxes), L.ptr(scores), L.ptr(None if "classes" in drop else classes), B, A, a["score_thresh"],
                                  a["iou_thresh"], R.MODES[a["mode"]], a["pre_max"], a["post_max"], L.ptr(db.keep), L.ptr(db.num),
                                  L.ptr(None if "out_boxes" in drop else db.boxes), L.ptr(None if "out_scores" in drop else db.scores),
                                  L.ptr(ws), nbytes, L.stream())
        assert rc == 0, drop
        assert np.array_equal(db.keep.cpu().numpy(), want["keep"]) and np.array_equal(db.num.cpu().numpy(), want["num"]), drop
        if "out_boxes" in drop:
            assert bool((wholes[2][0] == SENTINEL).all())
        else:
            C.same_bits(db.boxes.cpu().numpy(), want["boxes"])
        if "out_scores" in drop:
            assert bool((wholes[3][0] == SENTINEL).all())
        else:
            C.same_bits(db.scores.cpu().numpy(), want["scores"])
        assert all(guards_intact(w, fill) for w, fill in wholes) and guards_intact(whole_ws, 0xA5)


def test_per_class_scores_become_labels():
    from pseudo_lidar import nms
    a = C.call_args("classes")
    rng = np.random.RandomState(4)
    B, A = a["scores"].shape
    other = (a["scores"] - rng.uniform(0.05, 0.5, (B, A)).astype(F)).astype(F)
    first = a["classes"] == 0
    per_class = np.stack([np.where(first, a["scores"], other), np.where(first, other, a["scores"])], 2).astype(F)
    kw = on_device(a)
    kw.update(scores=dev(per_class), classes=None)
    got = nms(**kw)
    want = R.nms(**dict(a, classes=None))                    # the argmax does not separate the classes unless it is passed as classes
    check(got, want)
    labels = got.labels.cpu().numpy()
    for b in range(B):
        n = int(want["num"][b])
        assert labels[b, :n].tolist() == a["classes"][b][want["keep"][b, :n]].tolist() and (labels[b, n:] == -1).all()
    assert got.split()[0]["labels"].shape[0] == int(want["num"][0])
    kw.update(classes=dev(a["classes"]))
    check(nms(**kw), C.reference("classes"))


# ---------------------------------------------------------------------------------------------- capture and replay
def test_capture_with_out_and_replay_on_new_contents():
    from pseudo_lidar import nms
    a, b = C.call_args("classes"), C.call_args("classes")
    rng = np.random.RandomState(9)
    perm = rng.permutation(a["scores"].shape[1])
    b = dict(b, boxes=a["boxes"][:, perm].copy(), scores=a["scores"][:, perm[::-1]].copy(), classes=a["classes"][:, perm].copy())
    kw = on_device(a)
    db, wholes = holder(a["scores"].shape[0], a["post_max"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nms(out=db, **kw)                                    # warm-up: the workspace exists
    torch.cuda.current_stream().wait_stream(s)
    check(db, C.reference("classes"))
    ws = db._ws
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nms(out=db, **kw)
    assert db._ws is ws
    kw["boxes"].copy_(dev(b["boxes"])); kw["scores"].copy_(dev(b["scores"])); kw["classes"].copy_(dev(b["classes"]))
    db.keep.fill_(INT_SENTINEL); db.num.fill_(INT_SENTINEL); db.boxes.fill_(SENTINEL); db.scores.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    want = R.nms(**b)
    assert not np.array_equal(want["keep"], C.reference("classes")["keep"])
    check(db, want)
    assert all(guards_intact(w, fill) for w, fill in wholes)


# ---------------------------------------------------------------------------------------------- behind the pseudo-image
def test_nms_behind_a_pseudo_image_and_a_stub_head():
    """pillars -> PillarFeatureNet.pseudo_image -> a head made of torch operations (one anchor per cell: the centre from the cell, the
    sizes fixed, the heading and the score from two channels) -> nms: what Inference.detections chains, on a case of tests/pfn_cases.py"""
    import pfn_cases
    from pseudo_lidar import PillarBatch, PillarFeatureNet, PillarGrid, nms
    a = pfn_cases.build(pfn_cases.CASES[0])
    P, N, Cc = a["voxels"].shape
    pb = PillarBatch(len(a["offsets"]) - 1, P, N, Cc, DEV)
    pb.voxels, pb.coords, pb.num_points = (dev(a[n]) for n in ("voxels", "coords", "num_points"))
    pb.offsets.copy_(dev(a["offsets"]))
    pb.grid = PillarGrid(x=(0.0, float(a["nx"])), y=(0.0, float(a["ny"])), z=(-1.0, 1.0), size=(1.0, 1.0))
    net = PillarFeatureNet(dev(a["weight"]), dev(a["bias"]))

    def head(canvas):
        B, _, ny, nx = canvas.shape
        ys, xs = torch.meshgrid(torch.arange(ny, device=DEV, dtype=torch.float32), torch.arange(nx, device=DEV, dtype=torch.float32), indexing="ij")
        boxes = torch.empty((B, ny * nx, 7), device=DEV)
        boxes[:, :, 0], boxes[:, :, 1], boxes[:, :, 2] = xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5, -1.0
        boxes[:, :, 3], boxes[:, :, 4], boxes[:, :, 5] = 2.6, 1.2, 1.5
        boxes[:, :, 6] = torch.tanh(canvas[:, 0]).reshape(B, -1) * 3.0
        return boxes, torch.sigmoid(canvas[:, 1] - canvas[:, 2]).reshape(B, -1)

    boxes, scores = head(net.pseudo_image(pb))
    got = nms(boxes, scores, score_thresh=0.3, iou_thresh=0.1, pre_max=256, post_max=40)
    want = R.nms(boxes.cpu().numpy(), scores.cpu().numpy(), score_thresh=0.3, iou_thresh=0.1, pre_max=256, post_max=40)
    assert want["num"].min() >= 2
    check(got, want)


# ---------------------------------------------------------------------------------------------- refusals
def test_c_abi_refuses_bad_arguments_untouched():
    from mcav import lib as L
    import pseudo_lidar  # noqa: F401
    a = C.call_args("classes")
    B, A = a["scores"].shape
    boxes, scores, classes = dev(a["boxes"]), dev(a["scores"]), dev(a["classes"])
    db, wholes = holder(B, a["post_max"])
    nbytes = L.lib().mcav_box_nms_workspace_bytes(B, A, a["pre_max"])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    good = dict(boxes=L.ptr(boxes), scores=L.ptr(scores), classes=L.ptr(classes), B=B, A=A, score_thresh=a["score_thresh"],
                iou_thresh=a["iou_thresh"], mode=0, pre_max=a["pre_max"], post_max=a["post_max"], keep=L.ptr(db.keep), num=L.ptr(db.num),
                out_boxes=L.ptr(db.boxes), out_scores=L.ptr(db.scores), ws=L.ptr(ws), nbytes=nbytes)
    call = lambda **kw: L.lib().mcav_box_nms(*[dict(good, **kw)[k] for k in good], L.stream())
    off = lambda t, n: L.c_p(t.data_ptr() + n)
    nan = float("nan")
    for bad in (dict(boxes=None), dict(scores=None), dict(keep=None), dict(num=None), dict(ws=None), dict(B=0), dict(B=65536), dict(A=0),
                dict(B=4, A=1 << 29), dict(pre_max=0), dict(pre_max=4097), dict(post_max=0), dict(post_max=a["pre_max"] + 1),
                dict(score_thresh=nan), dict(iou_thresh=nan), dict(mode=2), dict(boxes=off(boxes, 2)), dict(classes=off(classes, 1)),
                dict(keep=off(db.keep, 2)), dict(out_boxes=off(db.boxes, 2)), dict(ws=off(ws, 8))):
        assert call(**bad) == -1, bad
    assert call(nbytes=nbytes - 1) == -2
    torch.cuda.synchronize()
    assert all(bool((w == fill).all()) for w, fill in wholes)
    assert call() == 0
    check(db, C.reference("classes"))


def test_python_side_refusals_on_the_gpu():
    from mcav import lib as L
    from pseudo_lidar import DetectionBatch, boxes_iou_bev, nms
    boxes, scores = torch.zeros(2, 8, 7, device=DEV), torch.zeros(2, 8, device=DEV)
    empty = nms(boxes, scores)                                # nothing valid: written, all empty
    assert empty.counts().tolist() == [0, 0] and bool((empty.keep == -1).all()) and not bool(empty.boxes.view(torch.int32).any())
    for call in (lambda: nms(boxes, scores.double()), lambda: nms(boxes, scores, classes=torch.zeros(2, 8, device=DEV)),
                 lambda: nms(boxes, scores, classes=torch.zeros(2, 8, dtype=torch.int32)),
                 lambda: nms(boxes, scores, out=DetectionBatch(3, 500, DEV)), lambda: nms(boxes, scores, out=DetectionBatch(2, 100, DEV)),
                 lambda: nms(boxes, scores, out=empty.keep), lambda: nms(boxes.transpose(0, 1)[:, :, :], scores),
                 lambda: nms(boxes, scores.cpu()), lambda: boxes_iou_bev(boxes[0], boxes[1].double()),
                 lambda: boxes_iou_bev(boxes[0], boxes[1].cpu())):
        with pytest.raises(L.MCAVError):
            call()
