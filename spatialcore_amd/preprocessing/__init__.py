"""spatialcore_amd.preprocessing -- what comes before pca: choosing the genes (sc_hvg_pearson)."""
from spatialcore_amd.preprocessing.hvg import highly_variable_genes

__all__ = ["highly_variable_genes"]
