"""The exact nearest-neighbour graph of a representation on the GPU, stored as scanpy's ``pp.neighbors`` stores its
graph: ``louvain`` and ``diffusion_map`` take it by ``graph="connectivities"``; and the same search
between two sets of cells: ``ingest`` maps new cells onto an annotated reference."""

from spatialcore_amd.neighbors.graph import neighbors
from spatialcore_amd.neighbors.ingest import ingest, query_neighbors

__all__ = ["neighbors", "ingest", "query_neighbors"]
