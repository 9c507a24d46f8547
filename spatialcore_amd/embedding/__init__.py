"""Low-dimensional layouts of the cells' neighbour graph on the GPU."""

from spatialcore_amd.embedding.layout import umap

__all__ = ["umap"]
