"""Measures of a result's quality, counted on the device: ``davis`` (the DAVIS J and F measures), ``mots`` (the KITTI-MOTS sMOTSA,
MOTSA and MOTSP) and ``ytvis`` (the YouTube-VIS mask AP and AR over tracks).  The names below are ``ytvis``'s; the other two modules
are imported by name (``evaluation.davis``, ``evaluation.mots``), as before."""
from .ytvis import YtvisEvaluator, evaluate_results, ground_truth_from_json, make_validator  # noqa: F401
