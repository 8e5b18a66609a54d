"""A KITTI-raw-shaped tree for mono + stereo training (loss.stereo): kitti_tree.make_tree plus each image_02 frame's image_03 twin and the
P_rect_03 line of every calib_cam_to_cam.txt (KITTI's values: the right colour camera ~0.53 m to the right of the left one)."""
import os

import numpy as np

from kitti_tree import SIZES, make_tree

P_RECT_03 = {"2011_09_26": [721.5377, 0.0, 609.5593, -339.5242, 0.0, 721.5377, 172.854, 2.199936, 0.0, 0.0, 1.0, 0.002729905],
             "2011_09_28": [707.0493, 0.0, 604.0814, -334.1081, 0.0, 707.0493, 180.5066, 0.3394072, 0.0, 0.0, 1.0, 0.002729659]}


def make_stereo_tree(root, frames=5, seed=0):
    """-> (split file path, rows as make_tree gives them, {image_02 path: image_03 path})."""
    from PIL import Image
    split, rows = make_tree(root, frames, seed)
    rng = np.random.RandomState(seed + 100)
    twins = {}
    for date in ("2011_09_26", "2011_09_28"):
        ddir = os.path.join(root, "KITTI", date)
        with open(os.path.join(ddir, "calib_cam_to_cam.txt"), "a") as f:
            f.write("P_rect_03: " + " ".join("%.6e" % v for v in P_RECT_03[date]) + "\n")
        left = os.path.join(ddir, "%s_drive_0001_sync" % date, "image_02", "data")
        right = left.replace("image_02", "image_03")
        os.makedirs(right)
        h, w = SIZES[date]
        for i in range(frames):
            name = "%010d.png" % i
            Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(right, name))
            twins[os.path.join(left, name)] = os.path.join(right, name)
    return split, rows, twins


def baseline_by_formula(date):
    """t_i = K^-1 P_rect_0i[:, 3], b = t_2.x - t_3.x, from the values written into the tree."""
    from kitti_tree import P_RECT
    t = []
    for P in (P_RECT[date], P_RECT_03[date]):
        P = np.array(P, dtype=np.float64).reshape(3, 4)
        t.append(np.linalg.inv(P[:, :3]) @ P[:, 3])
    return float(t[0][0] - t[1][0])


def stereo_config(split, root, H=24, W=80, batch=2):
    from kitti_tree import config_for
    cfg = config_for(split, root, H, W, batch)
    cfg["loss"] = dict(cfg.get("loss") or {}, stereo=True)
    return cfg
