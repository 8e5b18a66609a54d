"""geometry/velodyne.py -- KITTI Eigen ground truth from raw Velodyne scans, on the GPU.

monodepth2 scores its Eigen-split results against depth maps made by projecting each frame's raw scan into the image
(kitti_utils.generate_depth_map, run once per frame on the CPU by export_gt_depth.py).  Here the projection is one kernel call per batch
(include/mcav_depth.h: mcav_velo_depth_map; the definition is tests/velo_ref.py), so the maps are built beside the batch, with no
preprocessing step and no .npz file.  The reference reads these scans too (geometry/oxts_parser.py: load_velo_scan).

    P, (H, W) = velo_to_image(calib_dir)                              # host numpy, monodepth2's composition
    gt = depth_maps(points, offsets, P, sizes)                        # [B, 1, Hg, Wg] float32 on the device, zero-padded
    depth = generate_depth_map(calib_dir, velo_filename)              # monodepth2's signature: [H, W] float32 numpy
    few = select_beams(scan, keep=(5, 7, 9, 11))                       # a 4-beam scanner out of KITTI's 64 beams (host numpy)
    sparse = sparse_maps(points, offsets, P, sizes, h, w)             # [B, h, w]: the scans on the network's grid, for pseudo_lidar.gdc
"""
import ctypes
import os

import numpy as np
import torch

from mcav import lib as L

L.register({
    "mcav_velo_depth_map": (L.c_i, [L.c_p] * 5 + [L.c_i, L.c_i, L.c_i, ctypes.c_longlong, L.c_i, L.c_p, L.c_p]),
})

VELO_DEPTH_FROM_X = 1                          # include/mcav_depth.h MCAV_VELO_DEPTH_FROM_X


def load_velodyne_points(path):
    """A KITTI raw .bin scan -> float32 [N, 4] (x, y, z, reflectance), as the reference's load_velo_scan reads it."""
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def velo_to_image(calib_dir, cam=2):
    """-> (P, (H, W)): the 3x4 float64 velodyne -> image matrix of camera `cam` and the rectified image size, from a KITTI date directory's
    calib_cam_to_cam.txt and calib_velo_to_cam.txt, composed as monodepth2 does: P_rect_0cam . R_cam2rect . velo2cam (np.dot), with
    R_cam2rect the 4x4 identity holding R_rect_00 and velo2cam = [R | T; 0 0 0 1].  (H, W) is S_rect_02 reversed, for either camera, as in
    monodepth2."""
    from dataloaders import read_calib_file          # (here: dataloaders imports this module at load time)
    cam2cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    v2c = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    velo2cam = np.vstack((np.hstack((v2c["R"].reshape(3, 3), v2c["T"][..., np.newaxis])), np.array([0, 0, 0, 1.0])))
    R_cam2rect = np.eye(4)
    R_cam2rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    P_rect = cam2cam["P_rect_0%d" % int(cam)].reshape(3, 4)
    P = np.dot(np.dot(P_rect, R_cam2rect), velo2cam)
    H, W = (int(v) for v in cam2cam["S_rect_02"][::-1])
    return P, (H, W)


def depth_maps(points, offsets, P, sizes, Hg=None, Wg=None, flip=None, depth_from_x=False, device=None):
    """Sparse depth maps of a batch of scans (mcav_velo_depth_map).  points: float32 [N, 4], the scans concatenated (host or device);
    offsets: B + 1 integers, scan b is points[offsets[b]:offsets[b+1]]; P: [B, 3, 4] or [B, 12] float64; sizes: B pairs (H, W); Hg, Wg: the
    padded size (default: the largest); flip: B flags (the map of a flipped image is mirrored within its width); depth_from_x: depth = the
    point's x (monodepth2's vel_depth=True) instead of its camera z.  offsets and sizes are read on the host.
    -> [B, 1, Hg, Wg] float32 on the device, 0 where no point lands and in the padding."""
    offsets = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
    sizes = np.asarray(sizes.cpu() if torch.is_tensor(sizes) else sizes, dtype=np.int32).reshape(-1, 2)
    B = sizes.shape[0]
    if B < 1 or offsets.shape != (B + 1,) or (np.diff(offsets) < 0).any() or offsets[0] < 0:
        raise L.MCAVError("depth_maps: offsets must be %d non-decreasing integers >= 0, got %r" % (B + 1, offsets.tolist()))
    if (sizes < 1).any():
        raise L.MCAVError("depth_maps: sizes must be positive (H, W) pairs, got %r" % (sizes.tolist(),))
    Hg = int(sizes[:, 0].max()) if Hg is None else int(Hg)
    Wg = int(sizes[:, 1].max()) if Wg is None else int(Wg)
    if (sizes[:, 0] > Hg).any() or (sizes[:, 1] > Wg).any():
        raise L.MCAVError("depth_maps: sizes %r exceed the padded size (%d, %d)" % (sizes.tolist(), Hg, Wg))
    dev = torch.device(device) if device is not None else (points.device if torch.is_tensor(points) and points.is_cuda else
                                                            torch.device("cuda", torch.cuda.current_device()))
    pts = torch.as_tensor(points)
    if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 4:
        raise L.MCAVError("depth_maps: points must be float32 [N, 4], got %s %s" % (pts.dtype, tuple(pts.shape)))
    if int(offsets[-1]) > pts.shape[0]:
        raise L.MCAVError("depth_maps: offsets end at %d, past the %d points" % (int(offsets[-1]), pts.shape[0]))
    pts = L.dev(pts.to(dev, non_blocking=True).contiguous(), "points")
    Pm = np.ascontiguousarray(np.asarray(P.cpu() if torch.is_tensor(P) else P, dtype=np.float64).reshape(B, 12))
    fl = None
    if flip is not None:
        fl = np.asarray(flip.cpu() if torch.is_tensor(flip) else flip).astype(np.uint8).reshape(B)
    meta = torch.from_numpy(np.concatenate([offsets.view(np.uint8), Pm.view(np.uint8).reshape(-1), sizes.view(np.uint8).reshape(-1)] +
                                           ([fl] if fl is not None else [])).copy())
    meta = meta.pin_memory().to(dev, non_blocking=True)
    o_off, o_P, o_sz = 0, 8 * (B + 1), 8 * (B + 1) + 96 * B
    o_fl = o_sz + 8 * B
    out = torch.empty((B, 1, Hg, Wg), dtype=torch.float32, device=dev)
    base = meta.data_ptr()
    h = L.lib()
    max_points = int(np.diff(offsets).max())
    flags = VELO_DEPTH_FROM_X if depth_from_x else 0
    with torch.cuda.device(dev):
        L.check(h.mcav_velo_depth_map(L.ptr(pts), L.c_p(base + o_off), L.c_p(base + o_P), L.c_p(base + o_sz),
                                      L.c_p(base + o_fl) if fl is not None else L.c_p(0), B, Hg, Wg, max_points, flags, L.ptr(out),
                                      L.stream()), "mcav_velo_depth_map")
    return out


def select_beams(points, keep, of=64, fov=(-24.9, 2.0)):
    """The rows of a scan that lie on the beams `keep`: elevation = atan2(z, hypot(x, y)) in degrees, float64, binned into `of` equal bins
    over fov = (lowest, highest) (bin = floor((elevation - lowest) / (highest - lowest) * of); bin 0 is the lowest beam); rows outside
    the field of view or with a NaN belong to no beam.  Host, numpy, deterministic; the rows stay in order.  It emulates a cheap 4-beam
    scanner from KITTI's 64-beam HDL-64E scans (Pseudo-LiDAR++ section 5)."""
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise L.MCAVError("select_beams: points must be [N, >= 3], got %s" % (pts.shape,))
    of, lo, hi = int(of), float(fov[0]), float(fov[1])
    if of < 1 or not hi > lo:
        raise L.MCAVError("select_beams: of must be positive and fov ascending, got %r, %r" % (of, fov))
    keep = np.unique(np.asarray(list(keep), dtype=np.int64))
    if keep.size and (keep[0] < 0 or keep[-1] >= of):
        raise L.MCAVError("select_beams: keep must name beams in 0..%d, got %r" % (of - 1, keep.tolist()))
    xyz = pts[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        elev = np.degrees(np.arctan2(xyz[:, 2], np.hypot(xyz[:, 0], xyz[:, 1])))
        pos = np.floor((elev - lo) / (hi - lo) * of)
        inside = (pos >= 0) & (pos < of)
    beam = np.where(inside, pos, -1).astype(np.int64)
    return pts[np.isin(beam, keep) & inside]


def sparse_maps(points, offsets, P, sizes, h, w, **kw):
    """depth_maps on the network's h x w grid: P [B, 3, 4] is the velodyne -> image matrix at the resolutions `sizes` (B pairs (Hb, Wb));
    its first row is scaled by w / Wb and its second by h / Hb, and every map is h x w.  -> [B, h, w] float32 on the device, 0 where no
    point lands: the `sparse` input of pseudo_lidar.gdc."""
    sz = np.asarray(sizes.cpu() if torch.is_tensor(sizes) else sizes, dtype=np.float64).reshape(-1, 2)
    Pm = np.array(np.asarray(P.cpu() if torch.is_tensor(P) else P, dtype=np.float64).reshape(sz.shape[0], 3, 4))
    Pm[:, 0, :] *= (float(w) / sz[:, 1])[:, None]
    Pm[:, 1, :] *= (float(h) / sz[:, 0])[:, None]
    return depth_maps(points, offsets, Pm, [(int(h), int(w))] * sz.shape[0], **kw)[:, 0]


def generate_depth_map(calib_dir, velo_filename, cam=2, vel_depth=False):
    """monodepth2's kitti_utils.generate_depth_map: the scan projected into camera `cam`'s image, [H, W] metres, 0 without a point.
    One GPU call and one read-back.  Returns float32 (monodepth2 returns float64; its export_gt_depth.py stores float32).  On columns 0
    and W-1 this is the plain per-pixel minimum, where monodepth2's duplicate handling depends on the point order (include/mcav_depth.h)."""
    P, (H, W) = velo_to_image(calib_dir, cam)
    pts = load_velodyne_points(velo_filename)
    out = depth_maps(torch.from_numpy(pts), [0, pts.shape[0]], P[None], [(H, W)], depth_from_x=vel_depth)
    return out[0, 0].cpu().numpy()
