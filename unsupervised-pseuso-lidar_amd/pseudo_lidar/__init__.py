from .PseudoLiDAR import BeamTables, CloudBatch, PseudoLiDAR, beam_tables  # noqa: F401
