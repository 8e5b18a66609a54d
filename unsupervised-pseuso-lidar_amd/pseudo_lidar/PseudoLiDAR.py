"""Depth image -> pseudo-LiDAR point cloud on the GPU (reference pseudo-lidar/utils/PseudoLiDAR.py; its ROS node is out of scope).

Same class surface: `PseudoLiDAR(calib_dir, sparsity)` reads `calib_velo_to_cam.txt` / `calib_cam_to_cam.txt` exactly as the
reference (:12-29, :48-67), `.T` / `.P` hold the 4x4 and 3x4 matrices, `project_PL(depth_img)` returns the [n, 4] float64 cloud.
`project_PL` accepts a [rows, cols] CUDA tensor (float32, e.g. the depth network's 1/(10 disp + 0.01) map) and returns a CUDA
tensor: un-projection, rigid transform, the x >= 0 & z < 1 m cut and the order-preserving compaction run in three small kernels
(mcav_pseudo_lidar_project); only the point count comes back to the host.  `from_matrices` builds one without calibration files.

`project_batch(m)` is the product form: a batch of the network's disparities (or of depths) at the network's resolution -> one
`CloudBatch` of float32 x, y, z, i rows (KITTI .bin / sensor_msgs/PointCloud2 layout) with the resize to the calibration's resolution
inside, per-image calibration, and either the dense cloud or one return per (beam, azimuth) cell of a LiDAR-like grid
(`beam_tables`).  mcav_pl_batch_project: nothing comes back to the host until `counts()`, `split()` or `save_bin()` ask for it.
"""
import ctypes

import numpy as np
import torch

from mcav import lib as L

L.register({
    "mcav_pseudo_lidar_workspace_bytes": (L.c_sz, [L.c_i, L.c_i]),
    "mcav_pseudo_lidar_project": (L.c_i, [L.c_p, L.c_i, L.c_i, L.c_p, L.c_p, L.c_i, L.c_p, L.c_sz, L.c_p, L.c_p, L.c_sz, L.c_p]),
    "mcav_pl_batch_workspace_bytes": (L.c_sz, [L.c_i] * 5),
    "mcav_pl_beam_tables_check": (L.c_i, [L.c_p, L.c_i, L.c_p, L.c_i]),
    "mcav_pl_batch_project": (L.c_i, [L.c_p] + [L.c_i] * 5 + [L.c_p] * 5 + [L.c_i, L.c_i, L.c_f, ctypes.c_double, ctypes.c_double, L.c_i, L.c_i,
                                      L.c_p, L.c_sz, L.c_p, L.c_p, L.c_sz, L.c_p]),
})

PLB_INPUT_DEPTH = 1                            # include/mcav_depth.h MCAV_PLB_INPUT_DEPTH


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


class CloudBatch:
    """The clouds of a batch: `points` [capacity, 4] float32 (x, y, z, i) and `offsets` int32 [B + 1] on the device; image b owns
    points[offsets[b]:offsets[b+1]].  Rows beyond the capacity were not written (offsets stay exact).  Nothing is read back until asked."""

    def __init__(self, batch, capacity, device):
        self.points = torch.empty((int(capacity), 4), dtype=torch.float32, device=device)
        self.offsets = torch.zeros(int(batch) + 1, dtype=torch.int32, device=device)
        self._host = None
        self._meta_bytes, self._meta, self._ws = None, None, None       # project_batch's calibration table and workspace

    def __len__(self):
        return self.offsets.numel() - 1

    def counts(self):
        """offsets on the host (numpy int64 [B + 1]): the one read-back of the batch, kept until the next projection into this object."""
        if self._host is None:
            self._host = self.offsets.cpu().numpy().astype(np.int64)
        return self._host

    def split(self):
        """-> B views of `points`, one per image (clipped to the capacity)"""
        o = np.minimum(self.counts(), self.points.shape[0])
        return [self.points[int(o[b]):int(o[b + 1])] for b in range(len(self))]

    def save_bin(self, paths):
        """One device -> host copy of the used prefix, then one KITTI .bin (float32 x y z i) per image."""
        paths = list(paths)
        if len(paths) != len(self):
            raise L.MCAVError("save_bin: %d paths for %d clouds" % (len(paths), len(self)))
        o = self.counts()
        if int(o[-1]) > self.points.shape[0]:
            raise L.MCAVError("save_bin: the batch has %d points, the buffer holds %d" % (int(o[-1]), self.points.shape[0]))
        host = self.points[:int(o[-1])].cpu().numpy()
        for b, path in enumerate(paths):
            host[int(o[b]):int(o[b + 1])].tofile(path)


class PseudoLiDAR:
    def __init__(self, calib_dir, sparsity):
        self.T, self.P = self.get_trans_proj(calib_dir)
        self.sparsity = sparsity

    @classmethod
    def from_matrices(cls, T, P, sparsity):
        self = object.__new__(cls)
        self.T, self.P = np.asarray(T, dtype=np.float64), np.asarray(P, dtype=np.float64)
        self.sparsity = sparsity
        return self

    def read_calib_file(self, filepath):
        """key: floats ... per line; non-float values (dates) are skipped (reference :12-29)."""
        data = {}
        with open(filepath, "r") as f:
            for line in f.readlines():
                line = line.rstrip()
                if len(line) == 0:
                    continue
                key, value = line.split(":", 1)
                try:
                    data[key] = np.array([float(x) for x in value.split()])
                except ValueError:
                    pass
        return data

    def get_trans_proj(self, calib_dir):
        velo = self.read_calib_file(calib_dir + "calib_velo_to_cam.txt")
        cam = self.read_calib_file(calib_dir + "calib_cam_to_cam.txt")
        T = np.vstack([np.concatenate((velo["R"].reshape(3, 3), velo["T"].reshape(3, 1)), axis=1), [0, 0, 0, 1]])
        return T, cam["P_rect_02"].reshape(3, 4)

    def project_PL(self, depth_img):
        depth = L.dev(torch.as_tensor(depth_img).to(torch.float32).contiguous(), "depth_img")
        if depth.dim() != 2:
            raise L.MCAVError("project_PL: depth_img must be [rows, cols]")
        rows, cols = depth.shape
        h = L.lib()
        ws = L.workspace(h.mcav_pseudo_lidar_workspace_bytes(rows, cols), depth.device, "pseudo_lidar")
        cloud = torch.empty((rows * cols, 4), dtype=torch.float64, device=depth.device)
        count = torch.zeros(1, dtype=torch.int32, device=depth.device)
        T = np.ascontiguousarray(self.T, dtype=np.float64)
        P = np.ascontiguousarray(self.P, dtype=np.float64)
        L.check(h.mcav_pseudo_lidar_project(L.ptr(depth), rows, cols, T.ctypes.data_as(ctypes.c_void_p), P.ctypes.data_as(ctypes.c_void_p),
                                            int(self.sparsity or 0), L.ptr(cloud), rows * cols, L.ptr(count), L.ptr(ws), ws.numel(), L.stream()),
                "mcav_pseudo_lidar_project")
        valid = int(count.item())
        step = int(self.sparsity) if self.sparsity else 1
        return cloud[:(valid + step - 1) // step]

    def project_batch(self, m, sizes=None, P=None, T=None, input="disparity", scale=1.0, intensity=None, max_height=1.0, max_depth=None,
                      beams=None, out=None, padded=None):
        """m: [B, h, w] or [B, 1, h, w] float32 on the GPU -- the network's sigmoid disparity, or depths with input="depth".
        sizes: B pairs (Hb, Wb), the resolution P describes (default: (h, w)); padded: (Hg, Wg) bounding them (default: the largest).
        P [3, 4] / [B, 3, 4], T [4, 4] / [B, 4, 4]: default the instance's.  scale multiplies the depth (pred_depth_scale_factor).
        intensity: a plane shaped as m for the 4th column (default 0).  max_height: the reference's max_high cut; max_depth: None = off.
        beams: a beam_tables result = one return per cell instead of the dense cloud; self.sparsity applies to the dense cloud only.
        out: a CloudBatch to reuse (needed under graph capture).  -> CloudBatch; no host synchronisation."""
        if not torch.is_tensor(m):
            raise L.MCAVError("project_batch: m must be a tensor on the GPU")
        if m.dim() == 4 and m.shape[1] == 1:
            m = m[:, 0]
        if m.dim() != 3:
            raise L.MCAVError("project_batch: m must be [B, h, w] or [B, 1, h, w], got %s" % (tuple(m.shape),))
        m = L.dev(m.contiguous() if m.is_cuda else m, "m")
        B, h, w = m.shape
        if input not in ("disparity", "depth"):
            raise L.MCAVError("project_batch: input must be 'disparity' or 'depth', got %r" % (input,))
        if intensity is not None:
            if intensity.dim() == 4 and intensity.shape[1] == 1:
                intensity = intensity[:, 0]
            if tuple(intensity.shape) != (B, h, w):
                raise L.MCAVError("project_batch: intensity must be shaped as m, got %s" % (tuple(intensity.shape),))
            intensity = L.dev(intensity.contiguous() if intensity.is_cuda else intensity, "intensity")
        sz = np.asarray([(h, w)] * B if sizes is None else (sizes.cpu() if torch.is_tensor(sizes) else sizes), dtype=np.int32).reshape(-1, 2)
        if sz.shape[0] != B or (sz < 1).any():
            raise L.MCAVError("project_batch: sizes must be %d positive (H, W) pairs, got %r" % (B, sz.tolist()))
        Hg, Wg = (int(sz[:, 0].max()), int(sz[:, 1].max())) if padded is None else (int(padded[0]), int(padded[1]))
        if (sz[:, 0] > Hg).any() or (sz[:, 1] > Wg).any():
            raise L.MCAVError("project_batch: sizes %r exceed the padded size (%d, %d)" % (sz.tolist(), Hg, Wg))
        sparsity = int(self.sparsity or 0)
        if beams is not None:
            if sparsity:
                raise L.MCAVError("project_batch: sparsity has no meaning with beams; build the PseudoLiDAR with sparsity 0")
            if not isinstance(beams, BeamTables):
                beams = BeamTables(*beams)
        try:
            Pm = np.broadcast_to(np.asarray(self.P if P is None else (P.cpu() if torch.is_tensor(P) else P), dtype=np.float64), (B, 3, 4))
            Tm = np.broadcast_to(np.asarray(self.T if T is None else (T.cpu() if torch.is_tensor(T) else T), dtype=np.float64), (B, 4, 4))
        except ValueError:
            raise L.MCAVError("project_batch: P must be [3, 4] or [B, 3, 4] and T [4, 4] or [B, 4, 4]")
        dev = m.device
        nb, na = (beams.n_beams, beams.n_azimuth) if beams is not None else (0, 0)
        # the calibration table and the sizes: one pinned buffer, one copy, made here and not inside the call
        meta = np.concatenate([np.concatenate([Pm.reshape(B, 12), Tm.reshape(B, 16)], axis=1).reshape(-1).view(np.uint8),
                               np.ascontiguousarray(sz).reshape(-1).view(np.uint8)]).tobytes()
        capacity = B * nb * na if beams is not None else B * Hg * Wg
        if out is None:
            out = CloudBatch(B, capacity, dev)
        elif not isinstance(out, CloudBatch) or len(out) != B or out.points.device != dev:
            raise L.MCAVError("project_batch: out must be a CloudBatch of %d images on %s" % (B, dev))
        hl = L.lib()
        nbytes = hl.mcav_pl_batch_workspace_bytes(B, Hg, Wg, nb, na)
        if nbytes == 0:
            raise L.MCAVError("project_batch: a batch of %d x %d x %d pixels (%d x %d cells) is beyond the call's 2^31 limit" % (B, Hg, Wg, nb, na))
        out._host = None
        # the object keeps its table and workspace: a second call with the same calibration (a replayed capture's warm-up) copies and
        # allocates nothing
        if out._meta_bytes != meta:
            out._meta = torch.frombuffer(bytearray(meta), dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)
            out._meta_bytes = meta
        if out._ws is None or out._ws.numel() < nbytes:
            out._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ws, meta = out._ws, out._meta
        elev, azim = beams.on(dev) if beams is not None else (None, None)
        with torch.cuda.device(dev):
            L.check(hl.mcav_pl_batch_project(L.ptr(m), B, h, w, Hg, Wg, L.c_p(meta.data_ptr() + 224 * B), L.c_p(meta.data_ptr()),
                                             L.ptr(intensity), L.ptr(elev), L.ptr(azim), nb, na, float(scale), float(max_height),
                                             float("inf") if max_depth is None else float(max_depth), sparsity,
                                             PLB_INPUT_DEPTH if input == "depth" else 0, L.ptr(out.points), out.points.shape[0],
                                             L.ptr(out.offsets), L.ptr(ws), ws.numel(), L.stream()), "mcav_pl_batch_project")
        return out
