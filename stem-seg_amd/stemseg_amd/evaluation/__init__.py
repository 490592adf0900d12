"""Measures of a result's quality, counted on the device: ``davis`` (the DAVIS J and F measures)."""
