from .PseudoLiDAR import (BeamTables, CloudBatch, GroundScale, PillarBatch, PillarGrid, PseudoLiDAR, beam_tables, ground_scale,  # noqa: F401
                          pillarize)
