"""The cell-cell graphs of the spatial modules: the coordinates and the symmetric union of the exact kNN lists that
``fit_spatial_nmf`` (nmf/spatial.py) and ``aggregate_neighbors`` (spatial/hops.py) build by default.  A caller's own graph
is read by _cell_graph.py."""

from __future__ import annotations

from typing import Optional

import numpy as np
from scipy import sparse

K_NEIGHBORS_MAX = 65536   # sc_knn_2d's limit


def _coordinates(adata, spatial_key) -> np.ndarray:
    if not isinstance(spatial_key, str) or spatial_key not in adata.obsm:
        raise ValueError(f"adata.obsm[{spatial_key!r}] not found. Spatial coordinates are required unless graph= is given.")
    xy = np.asarray(adata.obsm[spatial_key])
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError(f"only 2-D coordinates are supported (adata.obsm[{spatial_key!r}] has shape {xy.shape})")
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if not np.all(np.isfinite(xy)):
        raise ValueError(f"adata.obsm[{spatial_key!r}] contains NaN or infinite values")
    return xy


def union_of_knn(lists: np.ndarray, rows: Optional[np.ndarray], n: int) -> sparse.csr_matrix:
    """The symmetric union of neighbour lists with weight 1.0: ``lists`` (m, k) holds positions into ``rows`` (None: the
    cells themselves); entry (i, j) is stored if j is a neighbour of i or i one of j.  Canonical CSR, n x n."""
    m, k = lists.shape
    src = np.repeat(np.arange(m, dtype=np.int64), k)
    dst = lists.astype(np.int64).ravel()
    if rows is not None:
        src, dst = rows[src], rows[dst]
    A = sparse.coo_matrix((np.ones(2 * src.size), (np.concatenate([src, dst]), np.concatenate([dst, src]))), shape=(n, n)).tocsr()
    A.sum_duplicates()     # an edge both lists hold, or one list holds twice, is one entry
    A.sort_indices()
    A.data[:] = 1.0
    return A


def knn_union_graph(ctx, xy: np.ndarray, groups, n_neighbors: int, n: int) -> sparse.csr_matrix:
    """``union_of_knn`` of the exact 2-D search inside every group of ``groups`` = [(name, rows or None for all cells)]:
    cells of different groups never connect."""
    parts = []
    for _, rows in groups:
        lists = ctx.knn(xy if rows is None else xy[rows], int(n_neighbors))
        parts.append(union_of_knn(lists, rows, n))
    A = parts[0] if len(parts) == 1 else sum(parts[1:], parts[0]).tocsr()
    A.sort_indices()
    return A
