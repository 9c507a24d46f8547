"""neighbors: the exact nearest-neighbour graph of a representation as a first-class object.

The search (sc_knn_dense_gram: a Gram-form filter on the fp64 matrix cores with a proven error bound, an exact re-rank
and an exact fallback -- the lists of sc_knn_dense bit for bit) and the connectivities (sc_diffmap_graph, or sc_fuzzy_graph
for ``method="umap"``) run in HIP; the host checks the arguments and assembles the two sparse matrices.  There is no CPU
fallback."""

from __future__ import annotations

from typing import Optional

import numpy as np
from scipy import sparse

from spatialcore_amd import _lib
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd._rep_graph import _check_key, check_n_neighbors, representation, resident_graph

logger = get_logger("neighbors")

METHODS = ("gauss", "umap")


def neighbors(adata, n_neighbors: int = 15, use_rep: str = "X_pca", *, method: str = "gauss", key_added: Optional[str] = None,
              copy: bool = False, device: int = 0):
    """Exact ``n_neighbors`` nearest neighbours of every cell in ``adata.obsm[use_rep]`` (Euclidean), on the GPU, stored
    the way scanpy's ``pp.neighbors`` stores its graph so that ``louvain(graph=...)`` and ``diffusion_map(graph=...)``
    share one search.

    ``n_neighbors`` counts OTHER cells, as in ``louvain`` and ``diffusion_map``; scanpy's count includes the cell itself
    (its ``n_neighbors=16`` is ``n_neighbors=15`` here).  ``use_rep`` names a float32 / float64 (anything else is
    converted to float64) finite ``obsm`` entry with 1..64 columns; 2 <= ``n_neighbors`` <= 32 and below the number of
    cells.  The neighbours of a cell are the ``n_neighbors`` other cells smallest in (squared distance, index), the
    squared distance added in column order in fp64: the lists ``louvain(graph=None)`` and ``diffusion_map(graph=None)``
    build on too, through the same search (spatialcore_amd/_rep_graph.py).

    Writes ``obsp["distances"]`` (float64 CSR, exactly ``n_neighbors`` stored entries per row, columns sorted, values
    ``sqrt(d2)``; a zero distance is an explicit stored entry), ``obsp["connectivities"]`` (the symmetric union of the
    lists with ``diffusion_map``'s kernel weights: the matrix ``louvain(graph=None)`` clusters) and ``uns["neighbors"]`` =
    {``connectivities_key``, ``distances_key``, ``params`` (``n_neighbors``, ``method``, ``metric`` =
    "euclidean", ``use_rep``, ``n_features``), ``search`` (``path``, ``list_length``, ``rows_certified``,
    ``rows_fallback``: how the search went, not what it found)}; with ``key_added="x"`` the keys are
    ``obsp["x_distances"]``, ``obsp["x_connectivities"]`` and ``uns["x"]``.  Appends the usual entry to
    ``uns["spatialcore_metadata"]``.  A cell whose local scale is zero (more than half of its neighbours are exact
    duplicates of it) raises ``ValueError`` and nothing is written.

    ``method="umap"`` stores UMAP's fuzzy simplicial set instead (sc_fuzzy_graph: ``smooth_knn_dist``, the membership
    strengths and the probabilistic union ``p_ij + p_ji - p_ij p_ji`` with umap-learn's defaults, on the same union of the
    lists): the graph scanpy's ``pp.neighbors`` stores by default.  ``params["method"]`` is then "umap"; rho and sigma are
    not stored, and duplicates are legal (their memberships are 1).  It is restated from the published algorithm; parity
    with umap-learn's or scanpy's values is not pinned.  Any metric but Euclidean is out of scope."""
    if key_added is not None:
        _check_key("key_added", key_added)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    n = int(adata.n_obs)
    k = check_n_neighbors(n_neighbors, n)
    R = representation(adata, use_rep)

    ctx = _lib.default_context(device)
    logger.info(f"neighbors: {n:,} cells x {R.shape[1]} features, {k} neighbours")
    found = resident_graph(ctx, R, k, method, fetch=True)      # a zero local scale raises here, before anything is written
    idx, d2, search = found["idx"], found["d2"], found["search"]
    indptr, indices, w = ctx.diffmap_graph_get()
    logger.info(f"neighbors: path {search['path']}, {search['rows_fallback']:,} rows through the exact fallback, "
                f"{indices.size:,} stored connectivities")

    order = np.argsort(idx, axis=1, kind="stable")
    cols = np.take_along_axis(idx, order, axis=1)
    dist = np.sqrt(np.take_along_axis(d2, order, axis=1))
    distances = sparse.csr_matrix((dist.ravel(), cols.ravel().astype(np.int32), np.arange(n + 1, dtype=np.int64) * k), shape=(n, n))
    connectivities = sparse.csr_matrix((w, indices, indptr), shape=(n, n))

    adata = adata.copy() if copy else adata
    uns_key = "neighbors" if key_added is None else key_added
    dist_key = "distances" if key_added is None else key_added + "_distances"
    conn_key = "connectivities" if key_added is None else key_added + "_connectivities"
    params = {"n_neighbors": k, "method": method, "metric": "euclidean", "use_rep": use_rep, "n_features": int(R.shape[1])}
    adata.obsp[dist_key] = distances
    adata.obsp[conn_key] = connectivities
    adata.uns[uns_key] = {"connectivities_key": conn_key, "distances_key": dist_key, "params": params, "search": search}
    update_metadata(adata, "neighbors", {**params, "key_added": key_added},
                    {"obsp": [dist_key, conn_key], "uns": uns_key})
    return adata
