"""Measures of a result's quality, counted on the device: ``davis`` (the DAVIS J and F measures) and ``mots`` (the KITTI-MOTS sMOTSA,
MOTSA and MOTSP)."""
