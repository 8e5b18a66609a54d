from .PseudoLiDAR import (BeamTables, CloudBatch, GDCResult, GroundScale, PillarBatch, PillarGrid, PseudoLiDAR, beam_tables,  # noqa: F401
                          gdc, ground_scale, pillarize, pillarize_backward, project_batch_backward)
from .PillarFeatureNet import (PillarFeatureLayer, PillarFeatureNet, fold_batch, pillar_moments,  # noqa: F401
                               pillar_moments_backward)
