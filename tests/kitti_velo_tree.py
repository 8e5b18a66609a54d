"""A KITTI-raw-shaped tree for datasets.groundtruth: velodyne: kitti_tree.make_tree plus, per date directory, the R_rect_00 and S_rect_02
lines of calib_cam_to_cam.txt, a calib_velo_to_cam.txt with KITTI's R and T, and one velodyne_points/data/<frame>.bin scan per frame.
A scan is a seeded sweep plus a few hundred point_at points inside the tree's small image (with the full-resolution P_rect_02 few sweep
points land in the 1/8-size image), some of them sharing a pixel."""
import os

import numpy as np

import velo_ref as V
from kitti_tree import P_RECT, SIZES, make_tree


def tree_P(date):
    """The velodyne -> image matrix of the values as written into the tree (monodepth2's composition)."""
    f = lambda vals: [float("%.6e" % v) for v in vals]
    return V.compose(f(P_RECT[date]), f(V.R_RECT_00), f(V.R_VELO), f(V.T_VELO))


def make_velo_tree(root, frames=5, seed=0, sweep=20000, extra=300):
    """-> (split file path, rows as make_tree gives them, {image_02 path: .bin path})."""
    split, rows = make_tree(root, frames, seed)
    rng = np.random.RandomState(seed + 200)
    scans = {}
    for k, date in enumerate(("2011_09_26", "2011_09_28")):
        ddir = os.path.join(root, "KITTI", date)
        h, w = SIZES[date]
        with open(os.path.join(ddir, "calib_cam_to_cam.txt"), "a") as f:
            f.write("R_rect_00: " + " ".join("%.6e" % v for v in V.R_RECT_00) + "\n")
            f.write("S_rect_02: %.6e %.6e\n" % (w, h))
        with open(os.path.join(ddir, "calib_velo_to_cam.txt"), "w") as f:
            f.write("calib_time: 15-Mar-2012 11:37:16\n")
            f.write("R: " + " ".join("%.6e" % v for v in V.R_VELO) + "\n")
            f.write("T: " + " ".join("%.6e" % v for v in V.T_VELO) + "\n")
        P = tree_P(date)
        drive = os.path.join(ddir, "%s_drive_0001_sync" % date)
        vdir = os.path.join(drive, "velodyne_points", "data")
        os.makedirs(vdir)
        for i in range(frames):
            us, vs = rng.randint(0, w, extra), rng.randint(0, h, extra)
            k2 = min(40, extra // 2)
            us[extra // 2:extra // 2 + k2], vs[extra // 2:extra // 2 + k2] = us[:k2], vs[:k2]        # up to 40 pixels hit twice
            pts = [V.point_at(P, u, v, d) for u, v, d in zip(us, vs, rng.uniform(2.0, 80.0, extra))]
            scan = np.concatenate([V.scan(seed * 1000 + k * 100 + i, sweep), np.stack(pts)])
            scan = scan[rng.permutation(len(scan))]
            path = os.path.join(vdir, "%010d.bin" % i)
            scan.tofile(path)
            scans[os.path.join(drive, "image_02", "data", "%010d.png" % i)] = path
    return split, rows, scans


def velo_config(split, root, H=24, W=80, batch=2):
    from kitti_tree import config_for
    cfg = config_for(split, root, H, W, batch)
    cfg["datasets"]["groundtruth"] = "velodyne"
    return cfg
