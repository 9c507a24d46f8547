"""MI355X-native principal component analysis of the cells x genes matrix: the step between normalisation and
neighbours.  Exact covariance PCA as sklearn's ``PCA(svd_solver="covariance_eigh")`` computes it; the result feeds
``diffusion_map(adata, use_rep="X_pca")``."""

from spatialcore_amd.pca.decompose import pca, project_pca

__all__ = ["pca", "project_pca"]
