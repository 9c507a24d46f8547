"""spatialcore_amd.annotation -- the reference's ``spatialcore.annotation`` hot path on the MI355X: CellTypist-style
training and prediction."""
from spatialcore_amd.annotation.annotate import annotate_celltypist
from spatialcore_amd.annotation.confidence import transform_confidence
from spatialcore_amd.annotation.model import CellTypeModel
from spatialcore_amd.annotation.training import train_celltypist_model

__all__ = ["CellTypeModel", "annotate_celltypist", "train_celltypist_model", "transform_confidence"]
