from .PseudoLiDAR import (BeamTables, CloudBatch, GDCResult, GroundScale, OccupancyBatch, PillarBatch, PillarGrid, PseudoLiDAR,  # noqa: F401
                          VoxelGrid, beam_tables, gdc, ground_scale, occupancy, occupancy_backward, pillarize, pillarize_backward,
                          project_batch_backward)
from .PillarFeatureNet import (PillarFeatureLayer, PillarFeatureNet, fold_batch, pillar_moments,  # noqa: F401
                               pillar_moments_backward)
from .boxes import DetectionBatch, boxes_iou3d, boxes_iou_bev, nms  # noqa: F401
