"""MI355X-native ``spatialcore.nmf`` (the module the reference's roadmap names after ``spatialcore.spatial``):
non-negative matrix factorisation of the cells x genes matrix into gene programs and per-cell usages, as sklearn's
``NMF(solver="mu")`` computes it (``fit_nmf``, ``project_nmf``), and its spatial form, graph-regularised NMF on the
cells' neighbour graph (``fit_spatial_nmf``)."""

from spatialcore_amd.nmf.factorize import fit_nmf, project_nmf
from spatialcore_amd.nmf.spatial import fit_spatial_nmf

__all__ = ["fit_nmf", "project_nmf", "fit_spatial_nmf"]
