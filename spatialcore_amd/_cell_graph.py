"""The readers of a caller's cell-cell graph: an ``obsp`` name or a scipy sparse matrix, cells x cells, as a canonical CSR.

They share the ``obsp`` lookup; what each accepts differs on purpose:

    reader            values                          symmetry                                other
    symmetric_graph   positive                        symmetric, names the first offender     (louvain, umap)
    kernel_matrix     non-negative, zeros dropped     symmetric                               no empty row (diffusion_map)
    given_graph       as symmetric_graph              as symmetric_graph                      diagonal removed first (fit_spatial_nmf)
    pattern_graph     weights ignored                 any pattern, directed or not            diagonal and stored zeros dropped
                                                                                              (aggregate_neighbors)"""

from __future__ import annotations

import numpy as np
from scipy import sparse


def _lookup(adata, graph, arg: str = "graph"):
    """``graph`` itself, or the ``obsp`` entry it names."""
    if isinstance(graph, str):
        if graph not in adata.obsp:
            raise ValueError(f"{arg}={graph!r} is not an entry of adata.obsp (available: {sorted(adata.obsp)})")
        graph = adata.obsp[graph]
    return graph


def symmetric_graph(adata, graph, n: int) -> sparse.csr_matrix:
    """The caller's graph as a canonical float64 CSR: n x n, finite, positive, symmetric in structure and value.  A failure
    of the symmetry names the first offending entry in row order."""
    graph = _lookup(adata, graph)
    if not sparse.issparse(graph):
        raise ValueError("graph must be None, the name of an adata.obsp entry or a scipy sparse matrix")
    if graph.ndim != 2 or graph.shape != (n, n):
        raise ValueError(f"graph must be {n} x {n} (cells x cells), got {graph.shape}")
    if np.issubdtype(graph.dtype, np.complexfloating):
        raise ValueError("graph must be real")
    A = sparse.csr_matrix(graph, dtype=np.float64, copy=True)
    A.sum_duplicates()
    A.sort_indices()
    if A.nnz > 2**31 - 1:
        raise ValueError("at most 2^31 - 1 stored entries are supported")
    if A.nnz and not np.all(np.isfinite(A.data)):
        bad = int(np.flatnonzero(~np.isfinite(A.data))[0])
        raise ValueError(f"graph contains NaN or infinite values (first: stored entry {bad})")
    if A.nnz and A.data.min() <= 0:
        bad = int(np.flatnonzero(A.data <= 0)[0])
        row = int(np.searchsorted(A.indptr, bad, side="right") - 1)
        raise ValueError(f"graph must be positive: entry ({row}, {int(A.indices[bad])}) is {float(A.data[bad])!r}")
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    T = A.T.tocsr()
    T.sort_indices()
    if T.nnz != A.nnz or not np.array_equal(T.indptr, A.indptr) or not np.array_equal(T.indices, A.indices):
        here = rows * n + A.indices
        there = np.repeat(np.arange(n, dtype=np.int64), np.diff(T.indptr)) * n + T.indices
        bad = int(np.flatnonzero(~np.isin(here, there))[0])    # as many entries either way: one of A's has no mirror
        raise ValueError(f"graph must be symmetric: entry ({int(rows[bad])}, {int(A.indices[bad])}) is stored, "
                         f"({int(A.indices[bad])}, {int(rows[bad])}) is not")
    if not np.array_equal(T.data, A.data):
        bad = int(np.flatnonzero(T.data != A.data)[0])
        raise ValueError(f"graph must be symmetric: entry ({int(rows[bad])}, {int(A.indices[bad])}) is {float(A.data[bad])!r}, "
                         f"({int(A.indices[bad])}, {int(rows[bad])}) is {float(T.data[bad])!r}")
    return A


def kernel_matrix(adata, graph, n: int) -> sparse.csr_matrix:
    """The caller's kernel matrix as a canonical float64 CSR: n x n, symmetric, positive stored values, no empty row."""
    graph = _lookup(adata, graph)
    if not sparse.issparse(graph):
        raise ValueError("graph must be the name of an adata.obsp entry or a scipy sparse matrix")
    if graph.shape != (n, n):
        raise ValueError(f"graph must be {n} x {n} (cells x cells), got {graph.shape}")
    if np.issubdtype(graph.dtype, np.complexfloating):
        raise ValueError("graph must be real")
    A = sparse.csr_matrix(graph, dtype=np.float64, copy=True)
    A.sum_duplicates()
    if A.nnz and not np.all(np.isfinite(A.data)):
        raise ValueError("graph contains NaN or infinite values")
    if A.nnz and A.data.min() < 0:
        raise ValueError("graph must be non-negative")
    A.eliminate_zeros()
    A.sort_indices()
    if (A != A.T).nnz:
        raise ValueError("graph must be symmetric (it is the kernel matrix of an undirected graph)")
    empty = np.flatnonzero(np.diff(A.indptr) == 0)
    if empty.size:
        raise ValueError(f"graph has {empty.size} empty rows (first: {int(empty[0])}): every cell needs a neighbour")
    return A


def given_graph(adata, graph, n: int):
    """The caller's graph without its diagonal, then validated by ``symmetric_graph``, and its source."""
    source = f"obsp[{graph!r}]" if isinstance(graph, str) else "matrix"
    graph = _lookup(adata, graph)
    if sparse.issparse(graph) and graph.ndim == 2 and graph.shape == (n, n):
        coo = sparse.coo_matrix(graph)
        off = coo.row != coo.col
        graph = sparse.csr_matrix((coo.data[off], (coo.row[off], coo.col[off])), shape=(n, n))
    return symmetric_graph(adata, graph, n), source


def pattern_graph(adata, graph, n: int):
    """A caller's graph as the pattern the shells are taken on: any square pattern, directed or not; weights are ignored,
    the diagonal and stored zeros are dropped.  Canonical CSR (int64 indptr, int32 indices) and its source."""
    source = f"obsp[{graph!r}]" if isinstance(graph, str) else "matrix"
    graph = _lookup(adata, graph, "connectivity_key")
    if not sparse.issparse(graph):
        raise ValueError(f"connectivity_key must be None, the name of an adata.obsp entry or a scipy sparse matrix, got {type(graph).__name__}")
    if graph.ndim != 2 or graph.shape != (n, n):
        raise ValueError(f"the graph ({source}) must be cells x cells = ({n}, {n}), got {graph.shape}")
    coo = sparse.coo_matrix(graph)
    keep = (coo.row != coo.col) & (coo.data != 0)
    A = sparse.csr_matrix((np.ones(int(keep.sum())), (coo.row[keep], coo.col[keep])), shape=(n, n))
    A.sum_duplicates()     # an entry stored twice is one entry
    A.sort_indices()
    A.data[:] = 1.0
    return A, source
