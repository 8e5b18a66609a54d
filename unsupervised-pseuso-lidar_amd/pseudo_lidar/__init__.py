from .PseudoLiDAR import BeamTables, CloudBatch, GroundScale, PseudoLiDAR, beam_tables, ground_scale  # noqa: F401
