"""GPU: the graph-based depth correction (include/mcav_depth.h: mcav_gdc_graph, mcav_gdc_solve; pseudo_lidar.gdc; Inference.clouds(gdc=...))
against its restatement (tests/gdc_ref.py) on the cases of tests/gdc_cases.py.  The graph, its weights and flags are held bit for bit.
The solver differs from the restatement only in the order in which the float64 inner products are added, which can move alpha and beta
by one float32 rounding; its tolerance is the project's convention for differing summation orders: four times what separates the float32
restatement from float64 arithmetic on the same graph, measured per case and iteration count on the CPU when the test runs, plus
1e-6 m.  Measured (largest over the cases): iters = 1: 6.8e-6 m, iters = 2: 1.2e-5 m, iters = 5: 3.4e-4 m (`holes`; 5.9e-5 m on the
scene); the float32 restatement after 400 iterations against the dense float64 least-squares solution on the scene: 2.0e-3 m (this
scene converges slower than float32 resolves: float64 CG needs 3652 and 4760 iterations to reach the dense solution to 2e-13 m).
On one MI355X the kernels differed from the restatement by 0 m on every case at 1, 2 and 5 iterations, and by 1.96e-3 m from the dense
solution after 400 (the restatement's own figure)."""
import numpy as np
import pytest
import torch

import gdc_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
PAD = 64                                                     # sentinel elements behind every output


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Buffers:
    """outputs with PAD sentinel elements behind each; the workspace between two sentinel blocks"""

    def __init__(self, B, H, W, k, radius):
        from mcav import lib as L
        import pseudo_lidar  # noqa: F401  (registers the signatures)
        self.h = L.lib()
        self.shape, self.k, self.radius = (B, H, W), k, radius
        n = B * H * W
        self.n = n
        self.nbr = torch.full((n * k + PAD,), -77, dtype=torch.int32, device=DEV)
        self.w = torch.full((n * k + PAD,), -77.0, device=DEV)
        self.fl = torch.full((n + PAD,), 77, dtype=torch.uint8, device=DEV)
        self.out = torch.full((n + PAD,), -77.0, device=DEV)
        self.info = torch.full((4 * B + PAD,), -77.0, device=DEV)
        self.need = self.h.mcav_gdc_workspace_bytes(B, H, W, k, radius)
        assert self.need > 0 and self.need % 256 == 0
        self.ws = torch.full((self.need + 512,), 0x5A, dtype=torch.uint8, device=DEV)

    def graph(self, a):
        from mcav import lib as L
        B, H, W = self.shape
        p = a["params"]
        self.depth, self.sparse, self.K = dev(a["depth"]), dev(a["sparse"]), dev(a["K"])
        L.check(self.h.mcav_gdc_graph(L.ptr(self.depth), L.ptr(self.sparse), L.ptr(self.K), B, H, W, p["k"], p["radius"], p["reg"],
                                      p["min_depth"], p["max_depth"], L.ptr(self.nbr), L.ptr(self.w), L.ptr(self.fl),
                                      L.c_p(self.ws.data_ptr() + 256), self.need, L.stream()), "mcav_gdc_graph")

    def solve(self, a, iters, tol=1e-4):
        from mcav import lib as L
        B, H, W = self.shape
        L.check(self.h.mcav_gdc_solve(L.ptr(self.depth), L.ptr(self.sparse), L.ptr(self.nbr), L.ptr(self.w), L.ptr(self.fl), B, H, W, self.k,
                                      self.radius, a["min_known"], iters, tol, L.ptr(self.out), L.ptr(self.info),
                                      L.c_p(self.ws.data_ptr() + 256), self.need, L.stream()), "mcav_gdc_solve")

    def results(self):
        B, H, W = self.shape
        n, k = self.n, self.k
        torch.cuda.synchronize()
        return (self.nbr[:n * k].cpu().numpy().reshape(B, H, W, k), self.w[:n * k].cpu().numpy().reshape(B, H, W, k),
                self.fl[:n].cpu().numpy().reshape(B, H, W), self.out[:n].cpu().numpy().reshape(B, H, W),
                self.info[:4 * B].cpu().numpy().reshape(B, 4))

    def sentinels_intact(self):
        n, k, B = self.n, self.k, self.shape[0]
        assert bool((self.nbr[n * k:] == -77).all()) and bool((self.w[n * k:] == -77.0).all()) and bool((self.fl[n:] == 77).all())
        assert bool((self.out[n:] == -77.0).all()) and bool((self.info[4 * B:] == -77.0).all())
        assert bool((self.ws[:256] == 0x5A).all()) and bool((self.ws[256 + self.need:] == 0x5A).all())


def buffers_for(case):
    a = C.build(case)
    return a, Buffers(*a["depth"].shape, a["params"]["k"], a["params"]["radius"])


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def check_graph(case):
    C.check_non_trivial(case)
    a, buf = buffers_for(case)
    buf.graph(a)
    nbr, w, fl, _, _ = buf.results()
    want = C.graph32(case)
    assert np.array_equal(fl, want[2])
    assert np.array_equal(nbr, want[0])
    assert np.array_equal(bits(w), bits(want[1]))
    buf.sentinels_intact()
    assert bool((buf.out == -77.0).all())                    # the graph call writes no other output


@pytest.mark.parametrize("case", C.CASES)
def test_graph_matches_restatement_bit_for_bit(case):
    check_graph(case)


def solver_bound(case, iters):
    """4 x (float32 restatement against float64 arithmetic on the same graph) + 1e-6 m, over the finite pixels"""
    x, y = C.solved32(case, iters)[0], C.solved64(case, iters)[0]
    ok = np.isfinite(y)
    measured = float(np.abs(x.astype(np.float64) - y)[ok].max())
    return measured, 4 * measured + 1e-6


def check_solver(case, counts):
    """iters = 0: the start vector's bits.  iters > 0: the restatement within the bound; known pixels, pixels off the graph and
    passed-through images bit for bit at every count; info exact; sentinels and the workspace's neighbours untouched."""
    a, buf = buffers_for(case)
    buf.graph(a)
    fl = C.graph32(case)[2]
    off, known = (fl & 1) == 0, (fl & 3) == 3
    for iters in counts:
        buf.solve(a, iters)
        _, _, _, out, info = buf.results()
        want, winfo = C.solved32(case, iters)
        assert np.array_equal(bits(out[off]), bits(a["depth"][off]))
        passed = winfo[:, 1] < a["min_known"]
        for b in range(len(out)):
            if passed[b]:
                assert np.array_equal(bits(out[b]), bits(a["depth"][b]))
            else:
                assert np.array_equal(bits(out[b][known[b]]), bits(a["sparse"][b][known[b]]))
        assert np.array_equal(info[:, :3], winfo[:, :3].astype(F)), (info, winfo)
        if iters == 0:
            assert np.array_equal(bits(out), bits(want))
            assert np.array_equal(info[:, 3], winfo[:, 3].astype(F))
        else:
            measured, bound = solver_bound(case, iters)
            ok = np.isfinite(want)
            assert np.array_equal(np.isfinite(out), ok)
            err = float(np.abs(out.astype(np.float64) - want.astype(np.float64))[ok].max())
            print("%s iters %d: kernels against the restatement %.3g m (float32 against float64 %.3g m, bound %.3g m)"
                  % (case, iters, err, measured, bound))
            assert err <= bound
            assert np.allclose(info[:, 3], winfo[:, 3], rtol=1e-3, atol=0)
        buf.sentinels_intact()


@pytest.mark.parametrize("case", C.CASES)
def test_solver_matches_restatement(case):
    check_solver(case, (0, 1, 2, 5))


@pytest.mark.parametrize("case", C.SCAN_CASES)
def test_more_block_sums_than_one_scan_pass(case):
    """258 workgroups: the scan of the per-workgroup in-degree sums takes a second pass and carries the first one's total into the CSR
    row starts, which the transposed product reads.  The graph bit for bit, the solver at 0 and 2 iterations under its bound."""
    check_graph(case)
    check_solver(case, (0, 2))


def test_400_iterations_against_the_dense_float64_solution():
    a, buf = buffers_for("scene")
    buf.graph(a)
    buf.solve(a, 400, tol=0.0)
    _, _, _, out, info = buf.results()
    dense = C.dense64("scene")
    measured = float(np.abs(C.solved32("scene", 400, 0.0)[0].astype(np.float64) - dense).max())
    err = float(np.abs(out.astype(np.float64) - dense).max())
    print("scene, 400 iterations against the dense solution: kernels %.3g m, restatement %.3g m" % (err, measured))
    assert err <= 4 * measured + 1e-6
    assert info[:, 2].tolist() == [400.0, 400.0]
    t = a["truth"].astype(np.float64)
    assert (np.mean(np.abs(out - t) / t, axis=(1, 2)) <= np.mean(np.abs(a["depth"] - t) / t, axis=(1, 2)) / 5).all()


def test_tolerance_stops_an_image_and_leaves_it():
    """with a loose tolerance the images stop early, each at the restatement's count, and the later launches leave them untouched"""
    a, buf = buffers_for("scene")
    buf.graph(a)
    buf.solve(a, 60, tol=3e-2)
    _, _, _, out, info = buf.results()
    want, winfo = C.solved32("scene", 60, 3e-2)
    assert (winfo[:, 2] < 60).all() and (winfo[:, 2] > 0).all()
    assert info[:, 2].tolist() == winfo[:, 2].tolist()
    x, y = want, C.solved64("scene", 60, 3e-2)
    assert C.solved64("scene", 60, 3e-2)[1][:, 2].tolist() == winfo[:, 2].tolist()
    assert np.abs(out.astype(np.float64) - want).max() <= 4 * np.abs(x - y[0]).max() + 1e-6


def test_pass_through_and_info():
    a, buf = buffers_for("mixed")
    buf.graph(a)
    buf.solve(a, 5)
    _, _, fl, out, info = buf.results()
    assert np.array_equal(bits(out[1:]), bits(a["depth"][1:]))
    assert info[1].tolist() == [960.0, 0.0, 0.0, 1.0] and info[2].tolist() == [960.0, 2.0, 0.0, 1.0]
    assert info[0, :3].tolist() == [960.0, 80.0, 5.0] and 0 < info[0, 3] < 1
    assert not np.array_equal(out[0], a["depth"][0])


def test_two_runs_give_the_same_bytes():
    a, buf = buffers_for("holes")
    buf.graph(a)
    buf.solve(a, 5)
    first = [x.copy() for x in buf.results()]
    buf.out.fill_(-77.0)
    buf.ws[256:256 + buf.need].fill_(0xC3)                   # whatever an earlier call left in the workspace
    buf.graph(a)
    buf.solve(a, 5)
    for x, y in zip(first, buf.results()):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def test_capture_and_replay_on_new_contents():
    from pseudo_lidar import GDCResult, gdc
    a, b = C.build("scene"), C.build("holes")
    depth, sparse, K = dev(a["depth"]), dev(a["sparse"]), dev(a["K"])
    out = GDCResult(2, 24, 40, 10, DEV)
    gdc(depth, sparse, K, iters=5, out=out)                  # warm-up: allocates the workspace
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gdc(depth, sparse, K, iters=5, out=out)
    for case, src in (("holes", b), ("scene", a)):
        depth.copy_(dev(src["depth"])); sparse.copy_(dev(src["sparse"])); K.copy_(dev(src["K"]))
        out.depth.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        got, want = out.depth.cpu().numpy(), C.solved32(case, 5)[0]
        ok = np.isfinite(want)
        assert np.array_equal(out.nbr.cpu().numpy(), C.graph32(case)[0])
        assert np.abs(got.astype(np.float64) - want)[ok].max() <= solver_bound(case, 5)[1]
        assert out.info[:, 2].tolist() == [5.0, 5.0]


def test_python_entry_and_the_cloud_of_the_corrected_map():
    """gdc with keep_graph against the restatement; K given as P with sizes; gdc -> project_batch(input="depth") is the cloud of the
    corrected map"""
    from pseudo_lidar import PseudoLiDAR, gdc
    a = C.build("scene")
    res = gdc(dev(a["depth"])[:, None], dev(a["sparse"])[:, None], a["K"], iters=5, keep_graph=True)
    want = C.solved32("scene", 5)[0]
    assert res.graph is not None and res.graph[0] is res.nbr and res.graph[2] is res.flags
    assert np.array_equal(res.graph[0].cpu().numpy(), C.graph32("scene")[0]) and np.array_equal(res.flags.cpu().numpy(), C.graph32("scene")[2])
    assert np.array_equal(bits(res.graph[1].cpu().numpy()), bits(C.graph32("scene")[1]))
    assert np.abs(res.depth.cpu().numpy().astype(np.float64) - want).max() <= solver_bound("scene", 5)[1]
    P = np.zeros((2, 3, 4))
    P[:, 0, 0], P[:, 1, 1], P[:, 0, 2], P[:, 1, 2], P[:, 2, 2] = a["K"][:, 0] * 2, a["K"][:, 1] * 4, a["K"][:, 2] * 2, a["K"][:, 3] * 4, 1
    res2 = gdc(dev(a["depth"]), dev(a["sparse"]), P=P, sizes=[(96, 80)] * 2, iters=5)
    assert res2.graph is None
    assert np.array_equal(bits(res2.depth.cpu().numpy()), bits(res.depth.cpu().numpy()))
    pl = PseudoLiDAR.from_matrices(np.eye(4), P[0], 0)
    T = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1.0]])           # velodyne -> camera axes
    kw = dict(sizes=[(96, 80)] * 2, P=P, T=T, input="depth", max_height=10.0)
    cloud = pl.project_batch(res.depth, **kw)
    again = pl.project_batch(dev(res.depth.cpu().numpy()), **kw)
    raw = pl.project_batch(dev(a["depth"]), **kw)
    assert cloud.counts()[-1] > 1000 and np.array_equal(cloud.counts(), again.counts())
    n = int(cloud.counts()[-1])
    assert np.array_equal(bits(cloud.points[:n].cpu().numpy()), bits(again.points[:n].cpu().numpy()))
    m = min(n, int(raw.counts()[-1]))
    assert not np.array_equal(cloud.points[:m].cpu().numpy(), raw.points[:m].cpu().numpy())


def test_cli_on_the_synthetic_tree(tmp_path, monkeypatch):
    """python inference.py --gdc writes clouds that differ from the run without it and equal the Python composition; without the
    scans in the configuration it is refused"""
    import yaml
    import inference
    from kitti_velo_tree import make_velo_tree, velo_config
    from trainer import Trainer
    monkeypatch.chdir(tmp_path)
    split, rows, _ = make_velo_tree(str(tmp_path), frames=2, sweep=2000, extra=300)
    cfg = velo_config(split, str(tmp_path), 64, 128, batch=2)
    cfg["action"].update(from_scratch=True)
    torch.manual_seed(4)
    t = Trainer(cfg)
    t.save_chkpnt()
    cfg["datasets"]["calibration"] = True
    with open("cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    base = ["--config", "cfg.yaml", "--checkpoint", t.save_path, "--scale", "30", "--max-depth", "80"]
    beams = [str(i) for i in range(64)]
    inference.main(base + ["--out", "plain"])
    inference.main(base + ["--out", "gdc", "--gdc", "--gdc-beams"] + beams + ["--gdc-iters", "20", "--gdc-k", "6", "--gdc-radius", "2"])
    inf = inference.Inference(cfg, checkpoint=t.save_path)
    seen = 0
    for samples in inf.loader():
        opts = dict(beams=tuple(range(64)), iters=20, k=6, radius=2)
        res = inf.corrected_depth(samples, opts, scale=30.0)
        assert (res.info[:, 1] >= 3).all(), res.info
        want = inf.projector.project_batch(res.depth, sizes=samples["native_size"], P=samples["P_rect"], T=samples["T_velo_cam"],
                                           input="depth", max_depth=80.0)
        parts = [p.cpu().numpy() for p in want.split()]
        for b, path in enumerate(samples["path"]):
            got = np.fromfile(inf.cloud_path("gdc", path), F).reshape(-1, 4)
            plain = np.fromfile(inf.cloud_path("plain", path), F).reshape(-1, 4)
            assert len(got) > 100 and np.array_equal(bits(got), bits(parts[b]))
            assert got.shape != plain.shape or not np.array_equal(got, plain)
            seen += 1
    assert seen == len(rows)
    cfg["datasets"]["groundtruth"] = "resized"
    with open("bad.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(ValueError):
        inference.main(["--config", "bad.yaml", "--checkpoint", t.save_path, "--out", "x", "--gdc"])
    t.set_train()
