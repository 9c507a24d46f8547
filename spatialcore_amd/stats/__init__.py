"""MI355X-native counterpart of ``spatialcore.stats`` (reference src/spatialcore/stats/__init__.py): the one analysis
function the reference's vignettes take from it."""

from spatialcore_amd.stats.classify import classify_by_threshold

__all__ = ["classify_by_threshold"]
