"""CPU: the data side of mono + stereo training (loss.stereo): the metric baseline from calib_cam_to_cam.txt, UnSupKittiFiles' image_03 twins
on a KITTI-shaped tree, and the configuration errors."""
import os

import numpy as np
import pytest
import torch

from kitti_stereo_tree import baseline_by_formula, make_stereo_tree, stereo_config


def test_baseline_of_the_2011_09_26_calibration():
    from dataloaders import stereo_baseline_of
    from kitti_stereo_tree import P_RECT_03
    from kitti_tree import P_RECT
    calib = {"P_rect_02": np.array(P_RECT["2011_09_26"]), "P_rect_03": np.array(P_RECT_03["2011_09_26"])}
    b = stereo_baseline_of(calib)
    assert abs(b - 0.5327) < 5e-4, b                        # KITTI's left-right colour baseline
    assert abs(b - baseline_by_formula("2011_09_26")) < 1e-12
    with pytest.raises(ValueError, match="P_rect_03"):
        stereo_baseline_of({"P_rect_02": calib["P_rect_02"]})


def test_dataset_loads_the_image_03_twins_and_baselines(tmp_path):
    from PIL import Image
    from dataloaders import UnSupKittiDataset, read_calib_file, find_calib_dir
    split, rows, twins = make_stereo_tree(str(tmp_path))
    ds = UnSupKittiDataset(stereo_config(split, str(tmp_path)))
    assert ds.stereo and len(ds) == len(rows)
    for i, r in enumerate(rows):
        s = ds[i]
        assert s["stereo"].dtype == torch.uint8
        assert np.array_equal(s["stereo"].numpy(), np.asarray(Image.open(twins[r[0]])))
        date = os.path.basename(os.path.normpath(find_calib_dir(r[0])))
        assert s["stereo_baseline"].dtype == torch.float32
        assert abs(float(s["stereo_baseline"]) - baseline_by_formula(date)) < 1e-6
        assert "P_rect_03" in read_calib_file(find_calib_dir(r[0]) + "calib_cam_to_cam.txt")
    # without the key nothing changes: no stereo fields
    from kitti_tree import config_for
    plain = UnSupKittiDataset(config_for(split, str(tmp_path)))
    assert not plain.stereo and "stereo" not in plain[0] and "stereo_baseline" not in plain[0]


def test_missing_image_03_is_a_configuration_error(tmp_path):
    from dataloaders import UnSupKittiDataset
    split, rows, twins = make_stereo_tree(str(tmp_path))
    os.remove(twins[rows[2][0]])
    with pytest.raises(ValueError, match="image_03"):
        UnSupKittiDataset(stereo_config(split, str(tmp_path)))


def test_config_validation():
    import yaml
    from conftest import PKG
    from dataloaders import UnSupKittiDataset, stereo_from_config
    cfg = yaml.full_load(open(os.path.join(PKG, "configs", "basic_config.yaml")))
    cfg["datasets"]["dataset"] = ["synthetic"]
    assert stereo_from_config(cfg) is False
    cfg["loss"] = {"stereo": True}
    with pytest.raises(ValueError, match="synthetic"):
        UnSupKittiDataset(cfg)
    cfg["loss"] = {"stereo": "yes"}
    with pytest.raises(ValueError, match="loss.stereo"):
        stereo_from_config(cfg)


def test_losses_reject_stereo_inputs_without_the_attribute():
    from mcav import lib as L
    from losses import Losses
    t = torch.zeros(1, 3, 8, 16)
    d = [[torch.zeros(1, 1, 8, 16)], [torch.zeros(1, 1, 8, 16)]]
    with pytest.raises(L.MCAVError, match="stereo"):
        Losses().forward(t, [t, t], d, torch.zeros(1, 2, 6), torch.eye(3).repeat(1, 1, 1), None, stereo=t, stereo_baseline=torch.ones(1))
