"""Records what a library answers for every descriptor of tests/conv_plan_cases.py -> tests/golden/conv_plan_parent.npz.

Run once, without a GPU, against a library built from the commit BEFORE the dispatch was moved into csrc/conv_plan.h (MCAV_LIB_PATH selects it):

    MCAV_LIB_PATH=/path/to/parent/libmcav_depth.so python tests/golden/make_conv_plan_golden.py

Only the four planner queries that commit already had are asked, through plain ctypes (the package's own binding would look for entries the old
library lacks).  Without a device the planner counts 256 compute units, which is also the MI355X's.  Integer arrays only."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "unsupervised-pseuso-lidar_amd")]

import conv_plan_cases as K  # noqa: E402
from mcav import nn as N  # noqa: E402


def main():
    h = ctypes.CDLL(os.environ["MCAV_LIB_PATH"])
    h.mcav_wgrad_workspace_bytes.restype = ctypes.c_size_t
    _, ig = K.igemm_sweep(N)
    _, wg = K.wgrad_sweep(N)
    out = dict(
        igemm_mtiles=np.array([h.mcav_igemm_mtiles(ctypes.byref(d)) for d in ig], np.int32),
        igemm_uses_bf16=np.array([h.mcav_igemm_uses_bf16(ctypes.byref(d)) for d in ig], np.int8),
        wgrad_workspace_bytes=np.array([h.mcav_wgrad_workspace_bytes(ctypes.byref(d)) for d in wg], np.int64),
        wgrad_uses_bf16=np.array([h.mcav_wgrad_uses_bf16(ctypes.byref(d)) for d in wg], np.int8),
    )
    path = os.path.join(HERE, "conv_plan_parent.npz")
    np.savez_compressed(path, **out)
    print("%s: %d igemm cases (%d refused), %d wgrad cases (%d refused)" % (path, len(ig), int((out["igemm_mtiles"] < 0).sum()), len(wg),
                                                                            int((out["wgrad_workspace_bytes"] == 0).sum())))


if __name__ == "__main__":
    main()
