"""The exact nearest-neighbour graph of a representation on the GPU, stored as scanpy's ``pp.neighbors`` stores its
graph: ``louvain`` and ``diffusion_map`` take it by ``graph="connectivities"``."""

from spatialcore_amd.neighbors.graph import neighbors

__all__ = ["neighbors"]
