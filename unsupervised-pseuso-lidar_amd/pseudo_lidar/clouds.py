"""Network maps -> pseudo-LiDAR cloud batches -> a detector's pillars on the GPU, and what makes the maps metric before that.

`project_batch` (PseudoLiDAR.project_batch hands it the instance's calibration): a batch of disparities (or of depths) at the network's
resolution -> one `CloudBatch` of float32 x, y, z, i rows (KITTI .bin / sensor_msgs/PointCloud2 layout) with the resize to the
calibration's resolution inside, per-image calibration, and either the dense cloud or one return per (beam, azimuth) cell of a LiDAR-like
grid (`beam_tables`).  mcav_pl_batch_project: nothing comes back to the host until `counts()`, `split()` or `save_bin()` ask for it.
`ground_scale(m)` gives a monocular prediction its metric scale without ground truth (DNet's dense geometrical constraint): per image,
camera_height / median height of the pixels whose surface normal points down (mcav_ground_scale; the definition is
tests/ground_scale_ref.py).  `project_batch(..., scale="ground")` runs it and hands the scales on, on the device.
`gdc(depth, sparse, K)` is Pseudo-LiDAR++'s graph-based depth correction: a few exact LiDAR depths (a 4-beam scanner's, as a sparse map
on the prediction's grid: geometry.velodyne.sparse_maps) are propagated over the predicted depth map along a windowed KNN graph of its
back-projected pixels, keeping the predicted local shape (mcav_gdc_graph, mcav_gdc_solve; the definition is tests/gdc_ref.py).  The
corrected map goes into project_batch(input="depth").
`pillarize(points, offsets)` / `CloudBatch.pillars()` turn a cloud batch into what a LiDAR 3-D detector reads (PointPillars / SECOND /
OpenPCDet): a `PillarBatch` of voxels [P, N, C], coords [P, 4] and num_points [P] on a `PillarGrid`, the first N points of every non-empty
cell in cloud order (mcav_pillarize; the definition is tests/pillar_ref.py); `PillarBatch.pseudo_image(net)`: PillarFeatureNet.py.
`occupancy(points, offsets)` / `CloudBatch.occupancy()` is the other change of representation End-to-End Pseudo-LiDAR defines, the soft
quantisation for detectors that read a dense voxel grid (PIXOR): a [B, nz, ny, nx] canvas on a `VoxelGrid` in which every cell holds
the mean Gaussian weight of its own points plus 1/26 of its 26 neighbours' (mcav_cloud_occupancy; the definition is tests/quant_ref.py),
differentiable back to the cloud rows (mcav_cloud_occupancy_bwd) and from there, through project_batch, to the disparity.
"""
import ctypes

import numpy as np
import torch

from mcav import lib as L

from ._host import OffsetBatch, _matrices, _plane, _sizes, grown, pack_table, recorded, table_box, table_calib, table_sizes, upload

L.register({
    "mcav_pl_batch_workspace_bytes": (L.c_sz, [L.c_i] * 5),
    "mcav_pl_beam_tables_check": (L.c_i, [L.c_p, L.c_i, L.c_p, L.c_i]),
    "mcav_pl_batch_project": (L.c_i, [L.c_p] + [L.c_i] * 5 + [L.c_p] * 5 + [L.c_i, L.c_i, L.c_f, ctypes.c_double, ctypes.c_double, L.c_i, L.c_i,
                                      L.c_p, L.c_sz, L.c_p, L.c_p, L.c_sz, L.c_p]),
    "mcav_pl_batch_project_scaled": (L.c_i, [L.c_p] + [L.c_i] * 5 + [L.c_p] * 5 + [L.c_i, L.c_i, L.c_f, L.c_p, ctypes.c_double, ctypes.c_double,
                                             L.c_i, L.c_i, L.c_p, L.c_sz, L.c_p, L.c_p, L.c_sz, L.c_p]),
    "mcav_pl_batch_project_indexed": (L.c_i, [L.c_p] + [L.c_i] * 5 + [L.c_p] * 5 + [L.c_i, L.c_i, L.c_f, L.c_p, ctypes.c_double, ctypes.c_double,
                                              L.c_i, L.c_i, L.c_p, L.c_sz, L.c_p, L.c_p, L.c_p, L.c_sz, L.c_p]),
    "mcav_pl_batch_project_bwd_workspace_bytes": (L.c_sz, [L.c_i] * 3),
    "mcav_pl_batch_project_bwd": (L.c_i, [L.c_p, L.c_sz, L.c_p, L.c_p, L.c_p] + [L.c_i] * 5 + [L.c_p, L.c_p, L.c_f, L.c_p, L.c_i, L.c_p, L.c_p,
                                          L.c_sz, L.c_p]),
    "mcav_ground_scale_workspace_bytes": (L.c_sz, [L.c_i] * 3),
    "mcav_ground_scale": (L.c_i, [L.c_p, L.c_i, L.c_i, L.c_i, L.c_p, L.c_p, L.c_p, L.c_f, L.c_f, L.c_i, L.c_f, L.c_i, L.c_p, L.c_p, L.c_p,
                                  L.c_sz, L.c_p]),
    "mcav_gdc_workspace_bytes": (L.c_sz, [L.c_i] * 5),
    "mcav_gdc_graph": (L.c_i, [L.c_p] * 3 + [L.c_i] * 5 + [L.c_f] * 3 + [L.c_p] * 4 + [L.c_sz, L.c_p]),
    "mcav_gdc_solve": (L.c_i, [L.c_p] * 5 + [L.c_i] * 7 + [L.c_f] + [L.c_p] * 3 + [L.c_sz, L.c_p]),
    "mcav_pillarize_workspace_bytes": (L.c_sz, [L.c_i, ctypes.c_longlong, L.c_i, L.c_i]),
    "mcav_pillarize": (L.c_i, [L.c_p, L.c_p, L.c_i, ctypes.c_longlong] + [L.c_f] * 6 + [L.c_i] * 4 + [L.c_p] * 3 + [ctypes.c_longlong, L.c_p,
                               L.c_p, L.c_sz, L.c_p]),
    "mcav_pillarize_indexed": (L.c_i, [L.c_p, L.c_p, L.c_i, ctypes.c_longlong] + [L.c_f] * 6 + [L.c_i] * 4 + [L.c_p] * 3 +
                               [ctypes.c_longlong, L.c_p, L.c_p, L.c_p, L.c_sz, L.c_p]),
    "mcav_pillarize_bwd": (L.c_i, [L.c_p] * 4 + [L.c_i, ctypes.c_longlong, L.c_i, L.c_i, L.c_p, ctypes.c_longlong, L.c_p]),
    "mcav_cloud_occupancy_workspace_bytes": (L.c_sz, [L.c_i, ctypes.c_longlong, L.c_i, L.c_i, L.c_i]),
    "mcav_cloud_occupancy": (L.c_i, [L.c_p, L.c_p, L.c_i, ctypes.c_longlong] + [L.c_f] * 6 + [L.c_i] * 3 + [L.c_f, L.c_p, L.c_p, L.c_p, L.c_sz,
                                     L.c_p]),
    "mcav_cloud_occupancy_bwd": (L.c_i, [L.c_p] * 4 + [L.c_i, ctypes.c_longlong] + [L.c_f] * 6 + [L.c_i] * 3 + [L.c_f, L.c_p, L.c_p]),
})

PLB_INPUT_DEPTH = GS_INPUT_DEPTH = PILLAR_DECORATE = 1         # include/mcav_depth.h MCAV_PLB_INPUT_DEPTH, MCAV_GS_INPUT_DEPTH, MCAV_PILLAR_DECORATE


class BeamTables:
    """The (beam, azimuth) grid of project_batch(beams=...): elev [n_beams + 1] = tan(e) |tan(e)| at the beam edges, azim [n_azimuth + 1] =
    tan(phi) at the azimuth edges, float64, finite and strictly increasing (anything else is refused: MCAV_E_INVALID).  The host arrays
    are what a reference reads; the device copies (made once per device) hold the same bytes."""

    def __init__(self, elev, azim):
        self.elev = np.ascontiguousarray(elev, dtype=np.float64).reshape(-1)
        self.azim = np.ascontiguousarray(azim, dtype=np.float64).reshape(-1)
        self.n_beams, self.n_azimuth = self.elev.size - 1, self.azim.size - 1
        L.check(L.lib().mcav_pl_beam_tables_check(self.elev.ctypes.data_as(ctypes.c_void_p), self.n_beams,
                                                  self.azim.ctypes.data_as(ctypes.c_void_p), self.n_azimuth), "beam tables")
        self._dev = {}

    def __iter__(self):                        # (elev, azim) = tables
        return iter((self.elev, self.azim))

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.elev).to(device), torch.from_numpy(self.azim).to(device))
        return self._dev[key]


def beam_tables(n_beams=64, n_azimuth=512, elevation=(-23.6, 2.0), azimuth=(-45.0, 45.0)):
    """Uniform-angle tables, built once on the host: n_beams beams between the elevations and n_azimuth bins between the azimuths, in
    degrees.  The defaults are Pseudo-LiDAR++'s sparsifier: 64 beams of 0.4 degrees, 90 degrees in 512 bins.  Edges that do not increase
    (swapped limits, a span reaching +-90 degrees) are refused."""
    if int(n_beams) < 1 or int(n_azimuth) < 1:
        raise L.MCAVError("beam_tables: n_beams and n_azimuth must be positive")
    e = np.tan(np.deg2rad(np.linspace(float(elevation[0]), float(elevation[1]), int(n_beams) + 1)))
    a = np.tan(np.deg2rad(np.linspace(float(azimuth[0]), float(azimuth[1]), int(n_azimuth) + 1)))
    return BeamTables(e * np.abs(e), a)


class GroundScale:
    """The estimator's result, on the device: `rows` [B, 4] float32 = (scale, median height, ground pixels, status) per image, `scales` =
    rows[:, 0] (a view; the fallback where status is 0), `mask` uint8 [B, h, w] with keep_mask.  Nothing is read back."""

    def __init__(self, batch, device, mask_shape=None):
        self.rows = torch.empty((int(batch), 4), dtype=torch.float32, device=device)
        self.mask = None if mask_shape is None else torch.empty(mask_shape, dtype=torch.uint8, device=device)
        self._uploaded_bytes, self._uploaded, self._ws = None, None, None

    @property
    def scales(self):
        return self.rows[:, 0]


def ground_scale(m, sizes=None, P=None, camera_height=1.65, max_angle_deg=5.0, box=None, min_ground=100, fallback=float("nan"),
                 input="disparity", keep_mask=False, out=None):
    """The metric scale of every image of a batch from its ground plane (mcav_ground_scale).
    m: [B, h, w] or [B, 1, h, w] float32 on the GPU -- the network's sigmoid disparity, or depths with input="depth"; sizes: B pairs
    (Hb, Wb), the resolution P describes (default (h, w)); P: [3, 4] or [B, 3, 4] (P_rect_02).  camera_height: the camera above the road in
    metres (1.65 on KITTI); max_angle_deg: the cone around the camera's y axis a ground normal lies in; box: (y0, y1, x0, x1) in network
    pixels (or B of them) to look in, None = everywhere; an image with fewer than min_ground ground pixels gets `fallback` and status 0.
    out: a GroundScale to reuse (needed under graph capture).  -> GroundScale; no host synchronisation."""
    m = _plane(m, "ground_scale")
    B, h, w = m.shape
    if P is None:
        raise L.MCAVError("ground_scale: P (the camera's 3x4 projection) is required")
    if input not in ("disparity", "depth"):
        raise L.MCAVError("ground_scale: input must be 'disparity' or 'depth', got %r" % (input,))
    sz = _sizes(sizes, B, h, w, "ground_scale")
    Pm = _matrices(P, B, (3, 4), "ground_scale: P must be [3, 4] or [B, 3, 4]")
    bx = None if box is None else np.asarray(box, dtype=np.int32)
    try:
        bx = None if box is None else np.broadcast_to(bx, (B, 4))
    except ValueError:
        raise L.MCAVError("ground_scale: box must be (y0, y1, x0, x1) or %d of them, got %r" % (B, box))
    meta = pack_table(Pm, None, sz, bx)
    dev = m.device
    if out is None:
        out = GroundScale(B, dev, (B, h, w) if keep_mask else None)
    elif not isinstance(out, GroundScale) or out.rows.shape[0] != B or out.rows.device != dev:
        raise L.MCAVError("ground_scale: out must be a GroundScale of %d images on %s" % (B, dev))
    if keep_mask and (out.mask is None or tuple(out.mask.shape) != (B, h, w)):
        raise L.MCAVError("ground_scale: out holds no [%d, %d, %d] mask" % (B, h, w))
    hl = L.lib()
    nbytes = hl.mcav_ground_scale_workspace_bytes(B, h, w)
    if nbytes == 0:
        raise L.MCAVError("ground_scale: a batch of %d x %d x %d pixels is refused (h, w >= 3, fewer than 2^31 pixels)" % (B, h, w))
    table, out._ws = upload(out, meta, dev), grown(out._ws, nbytes, dev)
    cos_max = float(np.float32(np.cos(np.deg2rad(np.float64(max_angle_deg)))))
    with torch.cuda.device(dev):
        L.check(hl.mcav_ground_scale(L.ptr(m), B, h, w, table_sizes(table, B), table_calib(table), table_box(table, B) if box is not None else None,
                                     float(camera_height), cos_max, int(min_ground), float(fallback),
                                     GS_INPUT_DEPTH if input == "depth" else 0, L.ptr(out.rows), L.ptr(out.mask if keep_mask else None),
                                     L.ptr(out._ws), out._ws.numel(), L.stream()), "mcav_ground_scale")
    return out


class GDCResult:
    """gdc's result, on the device: `depth` [B, h, w] float32, the corrected map; `info` [B, 4] float32 = (graph pixels, known graph
    pixels, iterations run, rs / rs0) per image; `graph`: with keep_graph the graph it was solved on, (nbr, weights, flags), else None.
    The object owns the graph's buffers either way (a later call with out= reuses them): `nbr` int32 [B, h, w, k] (pixel index or -1),
    `weights` float32 [B, h, w, k], `flags` uint8 [B, h, w] (bit 0: in the graph, bit 1: known).  Nothing is read back."""

    def __init__(self, batch, h, w, k, device):
        self.depth = torch.empty((int(batch), int(h), int(w)), dtype=torch.float32, device=device)
        self.info = torch.empty((int(batch), 4), dtype=torch.float32, device=device)
        self.nbr = torch.empty((int(batch), int(h), int(w), int(k)), dtype=torch.int32, device=device)
        self.weights = torch.empty((int(batch), int(h), int(w), int(k)), dtype=torch.float32, device=device)
        self.flags = torch.empty((int(batch), int(h), int(w)), dtype=torch.uint8, device=device)
        self.graph, self._inputs, self._ws = None, None, None
        self._uploaded_bytes, self._uploaded = None, None               # K as given on the host (its bytes) and on the device


def grid_intrinsics(P, sizes, h, w):
    """P [B, 3, 4] (or [3, 4]) at the resolutions `sizes` (B pairs (Hb, Wb)) -> float32 [B, 4] = (fx, fy, cx, cy) on an h x w grid: row 0
    times w / Wb, row 1 times h / Hb, as project_batch rescales its calibration."""
    sz = np.asarray(sizes.cpu() if torch.is_tensor(sizes) else sizes, dtype=np.float64).reshape(-1, 2)
    Pm = _matrices(P, sz.shape[0], (3, 4), "gdc: P must be [3, 4] or [B, 3, 4]")
    sx, sy = float(w) / sz[:, 1], float(h) / sz[:, 0]
    return np.stack([Pm[:, 0, 0] * sx, Pm[:, 1, 1] * sy, Pm[:, 0, 2] * sx, Pm[:, 1, 2] * sy], axis=1).astype(np.float32)


def gdc(depth, sparse, K=None, k=10, radius=3, reg=1e-3, min_depth=1e-3, max_depth=80.0, min_known=1, iters=400, tol=1e-4, out=None,
        keep_graph=False, P=None, sizes=None):
    """Graph-based depth correction from sparse LiDAR (Pseudo-LiDAR++; mcav_gdc_graph + mcav_gdc_solve).
    depth: [B, h, w] or [B, 1, h, w] float32 on the GPU, the predicted metric depth; sparse: the same shape, exact depths, 0 where there
    is none; K: [B, 4] or [4] = (fx, fy, cx, cy) of that grid (host values or a float32 tensor on the GPU), or P [B, 3, 4] / [3, 4] with
    sizes (B pairs (Hb, Wb), default (h, w)): the rows are rescaled to the grid.  k: neighbours (1..16) within a (2 radius + 1)^2 window
    (radius 1..7); reg: the ridge of the weights; a pixel counts iff min_depth < depth <= max_depth; an image with fewer than min_known
    known pixels passes through unchanged; at most iters conjugate-gradient iterations, an image stops once |r|^2 <= tol^2 |r0|^2.
    out: a GDCResult to reuse with its workspace (needed under graph capture); keep_graph: the result's `.graph` holds (nbr, weights,
    flags).  -> GDCResult; no host synchronisation."""
    depth, sparse = _plane(depth, "gdc"), _plane(sparse, "gdc")
    if depth.shape != sparse.shape or depth.device != sparse.device:
        raise L.MCAVError("gdc: depth and sparse must have one shape and device, got %s and %s" % (tuple(depth.shape), tuple(sparse.shape)))
    B, h, w = depth.shape
    k, radius = int(k), int(radius)
    if not 1 <= k <= 16 or not 1 <= radius <= 7:
        raise L.MCAVError("gdc: k must be in 1..16 and radius in 1..7, got %r and %r" % (k, radius))
    if int(iters) < 0 or not float(tol) >= 0.0 or not float(reg) > 0.0:
        raise L.MCAVError("gdc: iters and tol must not be negative and reg must be positive, got %r, %r, %r" % (iters, tol, reg))
    if (K is None) == (P is None):
        raise L.MCAVError("gdc: give K (fx, fy, cx, cy of the grid) or P with sizes, not both")
    dev = depth.device
    if out is None:
        out = GDCResult(B, h, w, k, dev)
    elif not isinstance(out, GDCResult) or tuple(out.nbr.shape) != (B, h, w, k) or out.depth.device != dev:
        raise L.MCAVError("gdc: out must be a GDCResult of [%d, %d, %d] with k = %d on %s" % (B, h, w, k, dev))
    if torch.is_tensor(K) and K.is_cuda:
        if tuple(K.shape) != (B, 4):
            raise L.MCAVError("gdc: a K tensor on the GPU must be [%d, 4], got %s" % (B, tuple(K.shape)))
        Kd = L.dev(K, "K")
    else:
        try:
            Kh = grid_intrinsics(P, _sizes(sizes, B, h, w, "gdc"), h, w) if K is None else \
                np.broadcast_to(np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float32), (B, 4))
        except ValueError:
            raise L.MCAVError("gdc: K must be [4] or [%d, 4]" % B)
        Kd = upload(out, Kh.tobytes(), dev)
    hl = L.lib()
    nbytes = hl.mcav_gdc_workspace_bytes(B, h, w, k, radius)
    if nbytes == 0:
        raise L.MCAVError("gdc: a batch of %d x %d x %d pixels with k = %d is refused (h w <= 2^24, k B h w < 2^31)" % (B, h, w, k))
    out._ws = grown(out._ws, nbytes, dev)
    with torch.cuda.device(dev):
        L.check(hl.mcav_gdc_graph(L.ptr(depth), L.ptr(sparse), L.ptr(Kd), B, h, w, k, radius, float(reg), float(min_depth), float(max_depth),
                                  L.ptr(out.nbr), L.ptr(out.weights), L.ptr(out.flags), L.ptr(out._ws), out._ws.numel(), L.stream()),
                "mcav_gdc_graph")
        L.check(hl.mcav_gdc_solve(L.ptr(depth), L.ptr(sparse), L.ptr(out.nbr), L.ptr(out.weights), L.ptr(out.flags), B, h, w, k, radius,
                                  int(min_known), int(iters), float(tol), L.ptr(out.depth), L.ptr(out.info), L.ptr(out._ws),
                                  out._ws.numel(), L.stream()), "mcav_gdc_solve")
    out._inputs = (depth, sparse, Kd)                 # alive as long as the enqueued work may read them
    out.graph = (out.nbr, out.weights, out.flags) if keep_graph else None
    return out


class CloudBatch(OffsetBatch):
    """The clouds of a batch on the device: `points` [capacity, 4] float32 (x, y, z, i); image b owns points[offsets[b]:offsets[b+1]]."""

    def __init__(self, batch, capacity, device):
        OffsetBatch.__init__(self, batch, device)
        self.points = torch.empty((int(capacity), 4), dtype=torch.float32, device=device)
        self._uploaded_bytes, self._uploaded, self._ws = None, None, None     # project_batch's calibration table and workspace
        self.ground, self._packed, self._scales = None, None, None      # scale="ground": the estimate, its scales packed; the [B] scales in use
        self.pixels = None                                              # int32 [capacity] with provenance: the pixel behind every row
        self._fwd, self._bwd_ws, self._stamp = None, [None], 0          # the backward's record and workspace (boxed: nodes share it); calls so far

    def split(self):
        """-> B views of `points`, one per image (clipped to the capacity)"""
        return [self.points[lo:hi] for lo, hi in self.ranges(self.points.shape[0])]

    def save_bin(self, paths):
        """One device -> host copy of the used prefix, then one KITTI .bin (float32 x y z i) per image."""
        paths = list(paths)
        if len(paths) != len(self):
            raise L.MCAVError("save_bin: %d paths for %d clouds" % (len(paths), len(self)))
        n = int(self.counts()[-1])
        if n > self.points.shape[0]:
            raise L.MCAVError("save_bin: the batch has %d points, the buffer holds %d" % (n, self.points.shape[0]))
        host = self.points[:n].cpu().numpy()
        for (lo, hi), path in zip(self.ranges(n), paths):
            host[lo:hi].tofile(path)

    def pillars(self, **kw):
        """pillarize(self.points, self.offsets, **kw) -> PillarBatch (grid, max_points, capacity, decorate, out, provenance)"""
        return pillarize(self.points, self.offsets, **kw)

    def occupancy(self, **kw):
        """occupancy(self.points, self.offsets, **kw) -> the [B, nz, ny, nx] canvas (grid, sigma2, out, provenance)"""
        return occupancy(self.points, self.offsets, **kw)


def project_batch(m, P, T, sparsity, sizes=None, input="disparity", scale=1.0, intensity=None, max_height=1.0, max_depth=None, beams=None,
                  out=None, padded=None, ground=None, provenance=False):
    """m: [B, h, w] or [B, 1, h, w] float32 on the GPU -- the network's sigmoid disparity, or depths with input="depth".
    sizes: B pairs (Hb, Wb), the resolution P describes (default: (h, w)); padded: (Hg, Wg) bounding them (default: the largest).
    P [3, 4] / [B, 3, 4], T [4, 4] / [B, 4, 4], sparsity: the calibration and the thinning, as a PseudoLiDAR holds them.
    scale multiplies the depth (pred_depth_scale_factor): a number for the whole batch, a float32 tensor [B] on the GPU with one per
    image (an image whose scale is not finite and positive gets an empty cloud), or "ground": ground_scale's estimate with this batch's
    sizes and P and the keywords in the dict `ground`, handed on on the device (the GroundScale is kept as out.ground; `ground` may hold
    camera_height, max_angle_deg, box, min_ground, fallback and keep_mask).  A scale tensor that is not contiguous (a column of a
    GroundScale's rows) is packed into a new tensor on every call: under graph capture hand over a contiguous one.
    intensity: a plane shaped as m for the 4th column (default 0).  max_height: the reference's max_high cut; max_depth: None = off.
    beams: a beam_tables result = one return per cell instead of the dense cloud; sparsity applies to the dense cloud only.
    out: a CloudBatch to reuse (needed under graph capture).  -> CloudBatch; no host synchronisation.
    provenance: also fill out.pixels, int32 [capacity]: the pixel r * Wg + c of its image's padded grid that became each row
    (mcav_pl_batch_project_indexed; the cloud is the same, bit for bit); project_batch_backward then works on the result.
    Differentiable: with grad mode on and an m that requires a gradient the call is a node of the autograd graph -- out.points carries
    the grad_fn, out.pixels is filled -- whose backward is project_batch_backward (mcav_pl_batch_project_bwd) on the current stream.
    Only m gets a gradient: which pixels survive the cuts, the sparsifier and the beam grid is piecewise constant, and scale, a scale
    tensor, scale="ground" (the estimate is a median, taken as a constant), intensity and the calibration are constants.  The
    CloudBatch must not be projected into again, nor the plane changed in place, before backward runs (both are refused)."""
    m = _plane(m, "project_batch")
    B, h, w = m.shape
    if input not in ("disparity", "depth"):
        raise L.MCAVError("project_batch: input must be 'disparity' or 'depth', got %r" % (input,))
    if intensity is not None:
        if intensity.dim() == 4 and intensity.shape[1] == 1:
            intensity = intensity[:, 0]
        if tuple(intensity.shape) != (B, h, w):
            raise L.MCAVError("project_batch: intensity must be shaped as m, got %s" % (tuple(intensity.shape),))
        intensity = L.dev(intensity.contiguous() if intensity.is_cuda else intensity, "intensity")
    sz = _sizes(sizes, B, h, w, "project_batch")
    Hg, Wg = (int(sz[:, 0].max()), int(sz[:, 1].max())) if padded is None else (int(padded[0]), int(padded[1]))
    if (sz[:, 0] > Hg).any() or (sz[:, 1] > Wg).any():
        raise L.MCAVError("project_batch: sizes %r exceed the padded size (%d, %d)" % (sz.tolist(), Hg, Wg))
    if beams is not None:
        if sparsity:
            raise L.MCAVError("project_batch: sparsity has no meaning with beams; build the PseudoLiDAR with sparsity 0")
        if not isinstance(beams, BeamTables):
            beams = BeamTables(*beams)
    refusal = "project_batch: P must be [3, 4] or [B, 3, 4] and T [4, 4] or [B, 4, 4]"
    Pm, Tm = _matrices(P, B, (3, 4), refusal), _matrices(T, B, (4, 4), refusal)
    dev = m.device
    nb, na = (beams.n_beams, beams.n_azimuth) if beams is not None else (0, 0)
    meta = pack_table(Pm, Tm, sz)
    capacity = B * nb * na if beams is not None else B * Hg * Wg
    if out is None:
        out = CloudBatch(B, capacity, dev)
    elif not isinstance(out, CloudBatch) or len(out) != B or out.points.device != dev:
        raise L.MCAVError("project_batch: out must be a CloudBatch of %d images on %s" % (B, dev))
    hl = L.lib()
    nbytes = hl.mcav_pl_batch_workspace_bytes(B, Hg, Wg, nb, na)
    if nbytes == 0:
        raise L.MCAVError("project_batch: a batch of %d x %d x %d pixels (%d x %d cells) is beyond the call's 2^31 limit" % (B, Hg, Wg, nb, na))
    out._host, table = None, upload(out, meta, dev)
    ws = out._ws = grown(out._ws, nbytes, dev)
    elev, azim = beams.on(dev) if beams is not None else (None, None)
    scales = None
    if isinstance(scale, str):
        if scale != "ground":
            raise L.MCAVError("project_batch: scale must be a number, a tensor [B] or 'ground', got %r" % (scale,))
        gkw = dict(ground or {})
        unknown = set(gkw) - {"camera_height", "max_angle_deg", "box", "min_ground", "fallback", "keep_mask"}
        if unknown:
            raise L.MCAVError("project_batch: ground= takes camera_height, max_angle_deg, box, min_ground, fallback and keep_mask, "
                              "not %s (sizes, P and input are the batch's)" % sorted(unknown))
        if out.ground is not None and gkw.get("keep_mask") and out.ground.mask is None:
            out.ground = None                                                      # made without a mask by an earlier call: a new one
        out.ground = ground_scale(m, sizes=sz, P=Pm, input=input, out=out.ground, **gkw)
        if out._packed is None:
            out._packed = torch.empty(B, dtype=torch.float32, device=dev)
        scales, scale = out._packed.copy_(out.ground.scales), 1.0                  # column 0 of the rows, packed: B floats, same stream
    elif torch.is_tensor(scale):
        if tuple(scale.shape) != (B,):
            raise L.MCAVError("project_batch: a scale tensor must be [%d], got %s" % (B, tuple(scale.shape)))
        scales, scale = L.dev(scale.contiguous() if scale.is_cuda else scale, "scale"), 1.0
    elif ground is not None:
        raise L.MCAVError("project_batch: ground= has no meaning without scale='ground'")
    flags = PLB_INPUT_DEPTH if input == "depth" else 0
    if scales is not None:
        out._scales = scales                                                       # alive as long as the cloud is

    def run(pixels):
        with torch.cuda.device(dev):
            head = (L.ptr(m), B, h, w, Hg, Wg, table_sizes(table, B), table_calib(table), L.ptr(intensity), L.ptr(elev), L.ptr(azim), nb, na,
                    float(scale))
            mid = (float(max_height), float("inf") if max_depth is None else float(max_depth), sparsity, flags, L.ptr(out.points),
                   out.points.shape[0], L.ptr(out.offsets))
            tail = (L.ptr(ws), ws.numel(), L.stream())
            if pixels is not None:
                L.check(hl.mcav_pl_batch_project_indexed(*head, L.ptr(scales), *mid, L.ptr(pixels), *tail), "mcav_pl_batch_project_indexed")
            elif scales is None:
                L.check(hl.mcav_pl_batch_project(*head, *mid, *tail), "mcav_pl_batch_project")
            else:
                L.check(hl.mcav_pl_batch_project_scaled(*head, L.ptr(scales), *mid, *tail), "mcav_pl_batch_project_scaled")

    # what the backward reads besides the cloud: the plane, the table this call used, the scale as the kernels took it
    out.points, out.pixels = recorded(
        m, out, out.points, out.pixels, index_shape=(out.points.shape[0],), provenance=provenance, run=run, saved=(m, out.offsets),
        record=lambda pixels: dict(m=m.detach(), table=table, scale=float(scale), scales=scales, flags=flags, padded=(Hg, Wg), pixels=pixels,
                                   offsets=out.offsets, capacity=out.points.shape[0], ws=out._bwd_ws),
        backward=_project_backward, again="backward: the CloudBatch was projected into again after this forward")
    return out


def project_batch_backward(cloud, grad_points, out=None):
    """The backward of project_batch as a plain call (mcav_pl_batch_project_bwd; a memset and two launches, no host synchronisation).
    cloud: a CloudBatch filled by project_batch with provenance=True (or by a differentiable call), its points, offsets, pixels and the
    plane it was made from still holding what they held; grad_points: [capacity, 4] float32, the gradient of cloud.points (column 3 is
    ignored, rows behind the count are never read).  -> d_m [B, h, w] float32, every element written: the float64 sum over the resized
    pixels whose taps touch it, no atomics, the same bytes from run to run.  out: a tensor to fill (else a new one; under graph capture it
    comes from the capture's pool).  The workspace lives on the CloudBatch."""
    if not isinstance(cloud, CloudBatch):
        raise L.MCAVError("project_batch_backward: cloud must be a CloudBatch, got %r" % type(cloud).__name__)
    if cloud._fwd is None or cloud.pixels is None:
        raise L.MCAVError("project_batch_backward: the CloudBatch holds no provenance (project_batch(..., provenance=True) records it)")
    return _project_backward(cloud._fwd, grad_points, out)


def _project_backward(f, grad_points, out):
    m, (Hg, Wg), cap, box = f["m"], f["padded"], f["capacity"], f["ws"]
    B, h, w = m.shape
    if not torch.is_tensor(grad_points) or tuple(grad_points.shape) != (cap, 4):
        raise L.MCAVError("project_batch_backward: grad_points must be [%d, 4]" % cap)
    dev = m.device
    if L.dev(grad_points, "grad_points").device != dev:
        raise L.MCAVError("project_batch_backward: grad_points is on %s, the cloud on %s" % (grad_points.device, dev))
    if out is None:
        out = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or tuple(out.shape) != (B, h, w) or L.dev(out, "out").device != dev:
        raise L.MCAVError("project_batch_backward: out must be float32 %s on %s" % ([B, h, w], dev))
    hl = L.lib()
    nbytes = hl.mcav_pl_batch_project_bwd_workspace_bytes(B, Hg, Wg)
    if nbytes == 0:
        raise L.MCAVError("project_batch_backward: a batch of %d x %d x %d pixels is refused" % (B, Hg, Wg))
    ws = box[0] = grown(box[0], nbytes, dev)
    with torch.cuda.device(dev):
        L.check(hl.mcav_pl_batch_project_bwd(L.ptr(grad_points), cap, L.ptr(f["pixels"]), L.ptr(f["offsets"]), L.ptr(m), B, h, w, Hg, Wg,
                                             table_sizes(f["table"], B), table_calib(f["table"]), f["scale"], L.ptr(f["scales"]), f["flags"],
                                             L.ptr(out), L.ptr(ws), ws.numel(), L.stream()), "mcav_pl_batch_project_bwd")
    return out


class PillarGrid:
    """The cells of pillarize: ranges x, y, z in metres (velodyne frame) and the pillar's size (vx, vy); one cell in z.  nx =
    round((x1 - x0) / vx), ny likewise.  The default is PointPillars' KITTI grid: 432 x 496 pillars of 0.16 m.  Empty, reversed or
    non-finite ranges and sizes are refused.  The kernels take the scalars as float32."""

    def __init__(self, x=(0.0, 69.12), y=(-39.68, 39.68), z=(-3.0, 1.0), size=(0.16, 0.16)):
        try:
            vals = [float(v) for pair in (x, y, z, size) for v in pair]
            if len(vals) != 8 or any(len(pair) != 2 for pair in (x, y, z, size)):
                raise ValueError
        except (TypeError, ValueError):
            raise L.MCAVError("PillarGrid: x, y, z are (low, high) pairs and size is (vx, vy), got %r %r %r %r" % (x, y, z, size))
        with np.errstate(over="ignore"):
            f32 = np.array(vals, np.float64).astype(np.float32)
        if not np.isfinite(f32).all():
            raise L.MCAVError("PillarGrid: every range and size must be finite (in float32), got %r" % (vals,))
        self.x, self.y, self.z, self.size = tuple(vals[0:2]), tuple(vals[2:4]), tuple(vals[4:6]), tuple(vals[6:8])
        if not (f32[6] > 0 and f32[7] > 0):
            raise L.MCAVError("PillarGrid: the pillar size must be positive, got %r" % (self.size,))
        if not (f32[1] > f32[0] and f32[3] > f32[2] and f32[5] > f32[4]):
            raise L.MCAVError("PillarGrid: empty range in x %r, y %r or z %r" % (self.x, self.y, self.z))
        self.nx = int(round((self.x[1] - self.x[0]) / self.size[0]))
        self.ny = int(round((self.y[1] - self.y[0]) / self.size[1]))
        if self.nx < 1 or self.ny < 1 or self.nx * self.ny >= 2 ** 31:
            raise L.MCAVError("PillarGrid: %d x %d cells" % (self.nx, self.ny))

    def scalars(self):
        """x0, y0, z0, z1, vx, vy as the C call takes them"""
        return self.x[0], self.y[0], self.z[0], self.z[1], self.size[0], self.size[1]

    def __repr__(self):
        return "PillarGrid(x=%r, y=%r, z=%r, size=%r) [%d x %d]" % (self.x, self.y, self.z, self.size, self.nx, self.ny)


class PillarBatch(OffsetBatch):
    """The pillars of a batch on the device: `voxels` [capacity, N, C] float32, `coords` [capacity, 4] int32 = (image, 0, iy, ix),
    `num_points` [capacity] int32 and `offsets` int32 [B + 1]; image b owns rows offsets[b]:offsets[b+1]."""

    def __init__(self, batch, capacity, max_points, columns, device):
        OffsetBatch.__init__(self, batch, device)
        self.voxels = torch.empty((int(capacity), int(max_points), int(columns)), dtype=torch.float32, device=device)
        self.coords = torch.empty((int(capacity), 4), dtype=torch.int32, device=device)
        self.num_points = torch.empty(int(capacity), dtype=torch.int32, device=device)
        self.grid, self._ws = None, None
        self.slot_points = None                                         # int32 [capacity, N] with provenance: the cloud row in every slot
        self._fwd, self._stamp = None, 0                                # what pillarize_backward reads; calls so far

    def split(self):
        """-> B tuples (voxels, coords, num_points) of views, one per image (clipped to the capacity)"""
        return [(self.voxels[lo:hi], self.coords[lo:hi], self.num_points[lo:hi]) for lo, hi in self.ranges(self.voxels.shape[0])]

    def pseudo_image(self, net, **kw):
        """net.pseudo_image(self, **kw): the batch through a PillarFeatureNet into its [B, C_out, ny, nx] canvas (layout, out, features)"""
        return net.pseudo_image(self, **kw)

    def save_npz(self, paths, features=None):
        """One device -> host copy of the used prefix (the three arrays packed on the device), then one .npz per image with `voxels`,
        `coords` and `num_points`; coords keep the image's index within this batch in column 0.  features: a [capacity, C_out] float32
        tensor of PillarFeatureNet.features(self); every .npz then also holds its image's rows as `features`."""
        paths = list(paths)
        if len(paths) != len(self):
            raise L.MCAVError("save_npz: %d paths for %d images" % (len(paths), len(self)))
        P = int(self.counts()[-1])
        if P > self.voxels.shape[0]:
            raise L.MCAVError("save_npz: the batch has %d pillars, the buffers hold %d" % (P, self.voxels.shape[0]))
        N, C = self.voxels.shape[1:]
        host = torch.cat([self.voxels[:P].reshape(-1).view(torch.int32), self.coords[:P].reshape(-1), self.num_points[:P]]).cpu().numpy()
        vox = host[:P * N * C].view(np.float32).reshape(P, N, C)
        coords = host[P * N * C:P * N * C + 4 * P].reshape(P, 4)
        num = host[P * N * C + 4 * P:]
        extra = None
        if features is not None:
            if not torch.is_tensor(features) or features.dim() != 2 or features.shape[0] < P or features.dtype != torch.float32:
                raise L.MCAVError("save_npz: features must be float32 [>= %d, C_out]" % P)
            extra = features[:P].cpu().numpy()
        for (lo, hi), path in zip(self.ranges(P), paths):
            arrays = dict(voxels=vox[lo:hi], coords=coords[lo:hi], num_points=num[lo:hi])
            if extra is not None:
                arrays["features"] = extra[lo:hi]
            with open(path, "wb") as f:
                np.savez(f, **arrays)


def pillarize(points, offsets, grid=None, max_points=32, capacity=None, decorate=False, out=None, provenance=False):
    """A cloud batch -> pillars (mcav_pillarize).  points: [n_max, 4] float32 (x, y, z, i) and offsets: int32 [B + 1] on the GPU, as a
    CloudBatch holds them (rows at and beyond offsets[B] are never read).  grid: a PillarGrid (default: PointPillars' KITTI grid).
    max_points: N, the slots of a pillar, 1..64: the first N points of the cell in cloud order.  capacity: the rows of the output, default
    min(n_max, B * ny * nx) -- every pillar there can be; with fewer, the pillars beyond are dropped and offsets stay exact.
    decorate: C = 9 instead of 4: PointPillars' offsets from the pillar's mean (3) and from the cell's centre (2).
    out: a PillarBatch to reuse with its workspace (needed under graph capture).  -> PillarBatch; no host synchronisation.
    provenance: also fill out.slot_points, int32 [capacity, N]: the row of `points` every slot holds, -1 in the zero-padded slots
    (mcav_pillarize_indexed; everything else is the same, bit for bit); pillarize_backward then works on the result.
    Differentiable: with grad mode on and points that require a gradient (a differentiable project_batch's) the call is a node of the
    autograd graph -- out.voxels carries the grad_fn, out.slot_points is filled -- whose backward is pillarize_backward
    (mcav_pillarize_bwd).  The PillarBatch must not be filled again before backward runs."""
    if not torch.is_tensor(points) or not torch.is_tensor(offsets):
        raise L.MCAVError("pillarize: points and offsets must be tensors on the GPU")
    if points.dim() != 2 or points.shape[1] != 4:
        raise L.MCAVError("pillarize: points must be [n, 4] (x, y, z, i), got %s" % (tuple(points.shape),))
    if offsets.dim() != 1 or offsets.numel() < 2:
        raise L.MCAVError("pillarize: offsets must be [B + 1], got %s" % (tuple(offsets.shape),))
    grid = PillarGrid() if grid is None else grid
    if not isinstance(grid, PillarGrid):
        raise L.MCAVError("pillarize: grid must be a PillarGrid, got %r" % (grid,))
    N = int(max_points)
    if not 1 <= N <= 64:
        raise L.MCAVError("pillarize: max_points must be in 1..64, got %r" % (max_points,))
    points, offsets = L.dev(points, "points"), L.dev(offsets, "offsets", torch.int32)
    n_max, B = points.shape[0], offsets.numel() - 1
    if n_max == 0:
        raise L.MCAVError("pillarize: points holds no rows")
    C = 9 if decorate else 4
    cells = B * grid.ny * grid.nx
    capacity = min(n_max, cells) if capacity is None else int(capacity)
    if capacity < 1:
        raise L.MCAVError("pillarize: capacity must be positive, got %d" % capacity)
    dev = points.device
    if out is None:
        out = PillarBatch(B, capacity, N, C, dev)
    elif (not isinstance(out, PillarBatch) or len(out) != B or out.voxels.device != dev or tuple(out.voxels.shape[1:]) != (N, C)):
        raise L.MCAVError("pillarize: out must be a PillarBatch of %d images with [*, %d, %d] voxels on %s" % (B, N, C, dev))
    else:
        L.dev(out.voxels, "out.voxels")
        for t, name, shape in ((out.coords, "out.coords", (out.voxels.shape[0], 4)), (out.num_points, "out.num_points", (out.voxels.shape[0],)),
                               (out.offsets, "out.offsets", (B + 1,))):
            if L.dev(t, name, torch.int32).device != dev or tuple(t.shape) != shape:
                raise L.MCAVError("pillarize: %s must be %s on %s, got %s on %s" % (name, list(shape), dev, list(t.shape), t.device))
        capacity = out.voxels.shape[0]
    hl = L.lib()
    nbytes = hl.mcav_pillarize_workspace_bytes(B, n_max, grid.ny, grid.nx)
    if nbytes == 0:
        raise L.MCAVError("pillarize: %d images of %d x %d cells with %d rows are refused (B <= 65535, fewer than 2^31 cells and rows)"
                          % (B, grid.ny, grid.nx, n_max))
    out._host, out.grid = None, grid
    out._ws = grown(out._ws, nbytes, dev)

    def run(slots):
        with torch.cuda.device(dev):
            head = (L.ptr(points), L.ptr(offsets), B, n_max, *grid.scalars(), grid.nx, grid.ny, N, PILLAR_DECORATE if decorate else 0,
                    L.ptr(out.voxels), L.ptr(out.coords), L.ptr(out.num_points), capacity, L.ptr(out.offsets))
            tail = (L.ptr(out._ws), out._ws.numel(), L.stream())
            if slots is not None:
                L.check(hl.mcav_pillarize_indexed(*head, L.ptr(slots), *tail), "mcav_pillarize_indexed")
            else:
                L.check(hl.mcav_pillarize(*head, *tail), "mcav_pillarize")

    # what the backward reads: the selection and the counts this call leaves
    out.voxels, out.slot_points = recorded(
        points, out, out.voxels, out.slot_points, index_shape=(capacity, N), provenance=provenance, run=run, saved=(out.num_points, out.offsets),
        record=lambda slots: dict(slot_points=slots, num_points=out.num_points, offsets=out.offsets, n_max=n_max, B=B, shape=(capacity, N, C)),
        backward=_pillarize_backward, again="backward: the PillarBatch was filled again after this forward")
    return out


def pillarize_backward(pillars, grad_voxels, out=None):
    """The backward of pillarize as a plain call (mcav_pillarize_bwd; a memset and one launch, no host synchronisation).  pillars: a
    PillarBatch filled by pillarize with provenance=True (or by a differentiable call), its num_points, offsets and slot_points still
    holding what they held; grad_voxels: [capacity, N, C] float32 (rows behind the pillar count are never read).  -> d_points [n_max, 4]
    float32, every row written: a row that no slot holds gets +0.0.  With decorated columns the offsets from the pillar's mean pass their
    gradient on to every point of the pillar; which point lands in which slot is piecewise constant and has no gradient.  out: a tensor
    to fill (else a new one)."""
    if not isinstance(pillars, PillarBatch):
        raise L.MCAVError("pillarize_backward: pillars must be a PillarBatch, got %r" % type(pillars).__name__)
    if pillars._fwd is None or pillars.slot_points is None:
        raise L.MCAVError("pillarize_backward: the PillarBatch holds no provenance (pillarize(..., provenance=True) records it)")
    return _pillarize_backward(pillars._fwd, grad_voxels, out)


def _pillarize_backward(f, grad_voxels, out):
    (cap, N, C), n_max, B, dev = f["shape"], f["n_max"], f["B"], f["slot_points"].device
    if not torch.is_tensor(grad_voxels) or tuple(grad_voxels.shape) != (cap, N, C):
        raise L.MCAVError("pillarize_backward: grad_voxels must be [%d, %d, %d]" % (cap, N, C))
    if L.dev(grad_voxels, "grad_voxels").device != dev:
        raise L.MCAVError("pillarize_backward: grad_voxels is on %s, the pillars on %s" % (grad_voxels.device, dev))
    if out is None:
        out = torch.empty((n_max, 4), dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or tuple(out.shape) != (n_max, 4) or L.dev(out, "out").device != dev:
        raise L.MCAVError("pillarize_backward: out must be float32 %s on %s" % ([n_max, 4], dev))
    with torch.cuda.device(dev):
        L.check(L.lib().mcav_pillarize_bwd(L.ptr(grad_voxels), L.ptr(f["slot_points"]), L.ptr(f["num_points"]), L.ptr(f["offsets"]), B, cap, N,
                                           PILLAR_DECORATE if C == 9 else 0, L.ptr(out), n_max, L.stream()), "mcav_pillarize_bwd")
    return out


class VoxelGrid:
    """The cells of occupancy: ranges x, y, z in metres (velodyne frame) and the cell's size (vx, vy, vz).  nx = round((x1 - x0) / vx), ny
    and nz likewise; nz, the canvas' channels, lies in 1..64.  The default is PIXOR's grid: 700 x 800 x 35 cells of 0.1 m.  Empty,
    reversed or non-finite ranges and sizes are refused.  The kernels take the scalars as float32."""

    def __init__(self, x=(0.0, 70.0), y=(-40.0, 40.0), z=(-2.5, 1.0), size=(0.1, 0.1, 0.1)):
        try:
            vals = [float(v) for group in (x, y, z, size) for v in group]
            if [len(group) for group in (x, y, z, size)] != [2, 2, 2, 3]:
                raise ValueError
        except (TypeError, ValueError):
            raise L.MCAVError("VoxelGrid: x, y, z are (low, high) pairs and size is (vx, vy, vz), got %r %r %r %r" % (x, y, z, size))
        with np.errstate(over="ignore"):
            f32 = np.array(vals, np.float64).astype(np.float32)
        if not np.isfinite(f32).all():
            raise L.MCAVError("VoxelGrid: every range and size must be finite (in float32), got %r" % (vals,))
        self.x, self.y, self.z, self.size = tuple(vals[0:2]), tuple(vals[2:4]), tuple(vals[4:6]), tuple(vals[6:9])
        if not (f32[6:] > 0).all():
            raise L.MCAVError("VoxelGrid: the cell size must be positive, got %r" % (self.size,))
        if not (f32[1] > f32[0] and f32[3] > f32[2] and f32[5] > f32[4]):
            raise L.MCAVError("VoxelGrid: empty range in x %r, y %r or z %r" % (self.x, self.y, self.z))
        self.nx, self.ny, self.nz = (int(round((r[1] - r[0]) / s)) for r, s in zip((self.x, self.y, self.z), self.size))
        if self.nx < 1 or self.ny < 1 or not 1 <= self.nz <= 64 or self.nx * self.ny * self.nz >= 2 ** 31:
            raise L.MCAVError("VoxelGrid: %d x %d x %d cells (nz must be in 1..64, fewer than 2^31 in all)" % (self.nx, self.ny, self.nz))

    def scalars(self):
        """x0, y0, z0, vx, vy, vz, nx, ny, nz as the C calls take them"""
        return self.x[0], self.y[0], self.z[0], self.size[0], self.size[1], self.size[2], self.nx, self.ny, self.nz

    def __repr__(self):
        return "VoxelGrid(x=%r, y=%r, z=%r, size=%r) [%d x %d x %d]" % (self.x, self.y, self.z, self.size, self.nx, self.ny, self.nz)


class OccupancyBatch:
    """What occupancy fills and keeps, on the device: `canvas` [B, nz, ny, nx] float32, `point_count` int32 [n_max] with provenance (the
    points that share each kept row's cell, 0 for a dropped row), the grid and sigma2 of the last call, and the call's workspace."""

    def __init__(self, batch, grid, device):
        self.canvas = torch.empty((int(batch), grid.nz, grid.ny, grid.nx), dtype=torch.float32, device=device)
        self.grid, self.sigma2, self.point_count, self._ws = grid, None, None, None
        self._fwd, self._stamp = None, 0                                # what occupancy_backward reads; calls so far


def occupancy(points, offsets, grid=None, sigma2=0.01, out=None, provenance=False):
    """A cloud batch -> its soft-occupancy canvas [B, nz, ny, nx] float32 (mcav_cloud_occupancy), z bins as channels.  points: [n_max, 4]
    float32 (x, y, z, i) and offsets: int32 [B + 1] on the GPU, as a CloudBatch holds them (rows at and beyond offsets[B] are never
    read).  grid: a VoxelGrid (default: PIXOR's 700 x 800 x 35 cells of 0.1 m).  canvas[b, iz, iy, ix] = the mean over the cell's points of
    exp(-|p - c|^2 / sigma2), c the cell's centre, plus 1/26 of the same mean of each of its 26 neighbours' points against c; sums are
    64-bit integers of 2^-40, so the canvas does not depend on the order of the rows.  sigma2: the squared width in m^2 (default 0.01).
    Every element is written; no host synchronisation.  out: an OccupancyBatch to reuse with its workspace (needed under graph capture);
    the return value is its `canvas`.
    provenance: also fill out.point_count, int32 [n_max] (the canvas is the same, bit for bit); occupancy_backward then works on `out`.
    Differentiable: with grad mode on and points that require a gradient (a differentiable project_batch's) the call is a node of the
    autograd graph whose backward is occupancy_backward (mcav_cloud_occupancy_bwd): columns x, y, z of the rows get a gradient, the counts
    and the fixed-point rounding are piecewise constant.  The OccupancyBatch must not be filled again before backward runs."""
    if not torch.is_tensor(points) or not torch.is_tensor(offsets):
        raise L.MCAVError("occupancy: points and offsets must be tensors on the GPU")
    if points.dim() != 2 or points.shape[1] != 4:
        raise L.MCAVError("occupancy: points must be [n, 4] (x, y, z, i), got %s" % (tuple(points.shape),))
    if offsets.dim() != 1 or offsets.numel() < 2:
        raise L.MCAVError("occupancy: offsets must be [B + 1], got %s" % (tuple(offsets.shape),))
    grid = VoxelGrid() if grid is None else grid
    if not isinstance(grid, VoxelGrid):
        raise L.MCAVError("occupancy: grid must be a VoxelGrid, got %r" % (grid,))
    sigma2 = float(sigma2)
    if not (np.isfinite(np.float32(sigma2)) and np.float32(sigma2) > 0):
        raise L.MCAVError("occupancy: sigma2 must be finite and positive (in float32), got %r" % (sigma2,))
    points, offsets = L.dev(points, "points"), L.dev(offsets, "offsets", torch.int32)
    n_max, B, dev = points.shape[0], offsets.numel() - 1, points.device
    if n_max == 0:
        raise L.MCAVError("occupancy: points holds no rows")
    shape = (B, grid.nz, grid.ny, grid.nx)
    if out is None:
        out = OccupancyBatch(B, grid, dev)
    elif not isinstance(out, OccupancyBatch) or tuple(out.canvas.shape) != shape or L.dev(out.canvas, "out.canvas").device != dev:
        raise L.MCAVError("occupancy: out must be an OccupancyBatch with a %s canvas on %s" % (list(shape), dev))
    hl = L.lib()
    nbytes = hl.mcav_cloud_occupancy_workspace_bytes(B, n_max, grid.nz, grid.ny, grid.nx)
    if nbytes == 0:
        raise L.MCAVError("occupancy: %d images of %d x %d x %d cells with %d rows are refused (B <= 65535, fewer than 2^31 cells and rows)"
                          % (B, grid.nz, grid.ny, grid.nx, n_max))
    out.grid, out.sigma2 = grid, sigma2
    ws = out._ws = grown(out._ws, nbytes, dev)

    def run(count):
        with torch.cuda.device(dev):
            L.check(hl.mcav_cloud_occupancy(L.ptr(points), L.ptr(offsets), B, n_max, *grid.scalars(), sigma2, L.ptr(out.canvas), L.ptr(count),
                                            L.ptr(ws), ws.numel(), L.stream()), "mcav_cloud_occupancy")

    out.canvas, out.point_count = recorded(
        points, out, out.canvas, out.point_count, index_shape=(n_max,), provenance=provenance, run=run, saved=(points, offsets),
        record=lambda count: dict(points=points.detach(), offsets=offsets, point_count=count, grid=grid, sigma2=sigma2, shape=shape, n_max=n_max),
        backward=_occupancy_backward, again="backward: the OccupancyBatch was filled again after this forward")
    return out.canvas


def occupancy_backward(record, grad_canvas, out=None):
    """The backward of occupancy as a plain call (mcav_cloud_occupancy_bwd; one launch, no host synchronisation).  record: an
    OccupancyBatch filled by occupancy with provenance=True (or by a differentiable call), or its record `._fwd`; the points, offsets and
    point_count still hold what they held.  grad_canvas: [B, nz, ny, nx] float32.  -> d_points [n_max, 4] float32, every row written:
    columns x, y, z of a kept row get the float64 sum of its 27 terms' derivatives, rounded once; column 3, dropped rows and rows behind
    the count get +0.0.  out: a tensor to fill (else a new one)."""
    if isinstance(record, OccupancyBatch):
        record = record._fwd
        if record is None:
            raise L.MCAVError("occupancy_backward: the OccupancyBatch holds no provenance (occupancy(..., provenance=True) records it)")
    if not isinstance(record, dict) or record.get("point_count") is None:
        raise L.MCAVError("occupancy_backward: record must be an OccupancyBatch or its record, got %r" % type(record).__name__)
    return _occupancy_backward(record, grad_canvas, out)


def _occupancy_backward(f, grad_canvas, out):
    points, grid, n_max, shape = f["points"], f["grid"], f["n_max"], f["shape"]
    dev = points.device
    if not torch.is_tensor(grad_canvas) or tuple(grad_canvas.shape) != shape:
        raise L.MCAVError("occupancy_backward: grad_canvas must be %s" % (list(shape),))
    if L.dev(grad_canvas, "grad_canvas").device != dev:
        raise L.MCAVError("occupancy_backward: grad_canvas is on %s, the cloud on %s" % (grad_canvas.device, dev))
    if out is None:
        out = torch.empty((n_max, 4), dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or tuple(out.shape) != (n_max, 4) or L.dev(out, "out").device != dev:
        raise L.MCAVError("occupancy_backward: out must be float32 %s on %s" % ([n_max, 4], dev))
    with torch.cuda.device(dev):
        L.check(L.lib().mcav_cloud_occupancy_bwd(L.ptr(points), L.ptr(f["offsets"]), L.ptr(f["point_count"]), L.ptr(grad_canvas), shape[0], n_max,
                                                 *grid.scalars(), f["sigma2"], L.ptr(out), L.stream()), "mcav_cloud_occupancy_bwd")
    return out
