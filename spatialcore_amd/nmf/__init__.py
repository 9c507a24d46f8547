"""MI355X-native ``spatialcore.nmf`` (the module the reference's roadmap names after ``spatialcore.spatial``):
non-negative matrix factorisation of the cells x genes matrix into gene programs and per-cell usages, as sklearn's
``NMF(solver="mu")`` computes it."""

from spatialcore_amd.nmf.factorize import fit_nmf, project_nmf

__all__ = ["fit_nmf", "project_nmf"]
