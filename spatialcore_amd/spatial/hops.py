"""aggregate_neighbors: CellCharter's neighbourhood aggregation (Varrone et al., Nature Genetics 2024;
``cellcharter.gr.aggregate_neighbors``, the ``cellcharter`` flavour of squidpy's ``calculate_niche``), restated from the
published algorithm (sc_hop_*); parity with a cellcharter run is not pinned.

For every cell and every hop distance l the mean (and, on request, the variance) of an embedding over the cells at graph
distance exactly l, concatenated to the cell's own row.  The host validates and builds the graph; the hop expansion and
the aggregation run in HIP, in fp64 and in one documented summation order.  There is no CPU fallback."""

from __future__ import annotations

import numbers
from typing import Optional, Sequence, Union

import numpy as np

from spatialcore_amd import _lib
from spatialcore_amd._batches import batch_groups
from spatialcore_amd._cell_graph import pattern_graph      # its name stays importable from here
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd._spatial_graph import K_NEIGHBORS_MAX, _coordinates, knn_union_graph

logger = get_logger("hops")

LAYER_MAX = 16
D_MAX = 64   # sc_hop_aggregate's limit, and that of neighbors, harmony_integrate and diffusion_map
AGGREGATIONS = ("mean", "var")


def _check_layers(n_layers):
    """The requested layers, ascending."""
    if isinstance(n_layers, numbers.Integral) and not isinstance(n_layers, bool):
        if not 0 <= n_layers <= LAYER_MAX:
            raise ValueError(f"n_layers must be an integer in 0..{LAYER_MAX} or a sequence of such layers, got {n_layers!r}")
        return list(range(int(n_layers) + 1))
    if isinstance(n_layers, (str, bytes)) or not hasattr(n_layers, "__iter__"):
        raise ValueError(f"n_layers must be an integer in 0..{LAYER_MAX} or a sequence of such layers, got {n_layers!r}")
    layers = list(n_layers)
    if not layers or any(not isinstance(v, numbers.Integral) or isinstance(v, bool) or not 0 <= v <= LAYER_MAX for v in layers):
        raise ValueError(f"n_layers must hold at least one layer, each an integer in 0..{LAYER_MAX}, got {layers!r}")
    if len(set(int(v) for v in layers)) != len(layers):
        raise ValueError(f"n_layers holds a layer twice: {layers!r}")
    return sorted(int(v) for v in layers)


def _check_aggregations(aggregations):
    aggs = [aggregations] if isinstance(aggregations, str) else list(aggregations) if hasattr(aggregations, "__iter__") else None
    if not aggs or any(not isinstance(a, str) or a not in AGGREGATIONS for a in aggs):
        raise ValueError(f'aggregations={aggregations!r} is not supported; supported: "mean", "var" or a sequence of the two')
    if len(set(aggs)) != len(aggs):
        raise ValueError(f"aggregations holds an aggregation twice: {aggs!r}")
    return aggs


def _representation(adata, use_rep) -> np.ndarray:
    if not isinstance(use_rep, str) or use_rep not in adata.obsm:
        raise ValueError(f"use_rep={use_rep!r} is not an entry of adata.obsm (available: {sorted(adata.obsm)})")
    X = np.asarray(adata.obsm[use_rep])
    if X.ndim != 2 or X.dtype not in (np.float32, np.float64):
        raise ValueError(f"adata.obsm[{use_rep!r}] must be a 2-D float32 or float64 array, got {X.dtype} with shape {X.shape}")
    if not 1 <= X.shape[1] <= D_MAX:
        raise ValueError(f"adata.obsm[{use_rep!r}] has {X.shape[1]} columns; 1..{D_MAX} are supported (reduce it first, e.g. with pca)")
    if not np.all(np.isfinite(X)):
        raise ValueError(f"adata.obsm[{use_rep!r}] contains NaN or infinite values")
    return np.ascontiguousarray(X)


def _sample_codes(adata, sample_key) -> np.ndarray:
    if not isinstance(sample_key, str) or sample_key not in adata.obs:
        raise ValueError(f"sample_key={sample_key!r} is not a column of adata.obs")
    return np.unique(np.asarray(adata.obs[sample_key]).astype(str), return_inverse=True)[1]


def aggregate_neighbors(adata, n_layers: Union[int, Sequence[int]] = 3, aggregations: Union[str, Sequence[str]] = "mean",
                        connectivity_key=None, use_rep: str = "X_pca", sample_key: Optional[str] = None,
                        out_key: str = "X_cellcharter", copy: bool = False, *, spatial_key: str = "spatial", n_neighbors: int = 6,
                        device: int = 0):
    """Neighbourhood aggregation of an embedding over the hops of a cell-cell graph (CellCharter): the features a
    clusterer turns into spatial domains, e.g. ``identify_niches(k, neighborhood_key=out_key)`` or
    ``neighbors(use_rep=out_key)`` then ``louvain``.

    Shell l of cell i holds the cells whose shortest path from i along stored entries has exactly l edges; layer 0 is the
    cell's own row.  ``n_layers``: an int L asks for the layers 0..L, a sequence of distinct ints >= 0 for exactly those
    (hops up to its maximum, at most 16, are computed).  ``aggregations``: ``"mean"``, ``"var"`` (the published
    E[x^2] - E[x]^2 over the shell) or a sequence of the two.  An empty shell (an isolated cell, a hop past the cell's
    component) gives zeros.

    Graph: with ``connectivity_key=None`` the one ``fit_spatial_nmf`` builds, the symmetric union of the exact
    ``n_neighbors`` nearest-neighbour lists of ``obsm[spatial_key]`` (2-D), searched inside every ``sample_key`` group
    (an ``obs`` column) so that slides whose coordinates overlap never connect.  ``connectivity_key`` may name an ``obsp``
    entry or be a scipy sparse matrix: cells x cells, any pattern, directed or not; weights are ignored, the diagonal
    and stored zeros dropped.  With such a graph ``sample_key`` only checks: an entry joining two samples is refused.

    ``use_rep``: an ``obsm`` entry, float32 or float64, 1..64 columns, finite.  The default is ``X_pca`` where cellcharter
    takes ``adata.X``: reduce the expression first (``pca``, ``harmony_integrate``).

    Writes ``adata.obsm[out_key]``, float64, cells x d (number of blocks): the layers in ascending order, inside a layer
    >= 1 the aggregations in the order given, layer 0 as the one block X; and ``adata.uns[out_key]`` = {``params``,
    ``graph`` = {``source``, ``n_neighbors``, ``stored_entries``}, ``layers``, ``aggregations``, ``n_features``, and per
    hop 1..max: ``shell_entries`` (stored entries of the shell), ``shell_max`` (its largest row), ``shell_empty`` (cells
    whose shell is empty)}; appends the usual entry to ``uns["spatialcore_metadata"]``.  The result is a function of the
    arguments alone, bit for bit."""
    layers = _check_layers(n_layers)
    aggs = _check_aggregations(aggregations)
    if not isinstance(out_key, str) or not out_key:
        raise ValueError(f"out_key must be a non-empty string, got {out_key!r}")
    X = _representation(adata, use_rep)
    n, d = X.shape
    groups, xy, A = None, None, None
    if connectivity_key is not None:
        A, source = pattern_graph(adata, connectivity_key, n)
        if sample_key is not None:
            codes = _sample_codes(adata, sample_key)
            rows = np.repeat(np.arange(n), np.diff(A.indptr))
            bad = np.flatnonzero(codes[rows] != codes[A.indices])
            if bad.size:
                raise ValueError(f"the graph ({source}) joins cells of different samples of adata.obs[{sample_key!r}]: "
                                 f"{bad.size} stored entries, the first at ({rows[bad[0]]}, {A.indices[bad[0]]})")
    else:
        if not isinstance(n_neighbors, numbers.Integral) or isinstance(n_neighbors, bool) or not 1 <= n_neighbors <= K_NEIGHBORS_MAX:
            raise ValueError(f"n_neighbors must be an integer in 1..{K_NEIGHBORS_MAX}, got {n_neighbors!r}")
        xy = _coordinates(adata, spatial_key)
        groups = batch_groups(adata, sample_key, "sample_key") if sample_key is not None else [(None, None)]
        smallest = min(n if rows is None else rows.size for _, rows in groups)
        if n_neighbors >= smallest:
            raise ValueError(f"n_neighbors={n_neighbors} needs more than the {smallest} cells of the smallest "
                             f"{'sample' if sample_key is not None else 'data set'}")
        source = "knn_union" if sample_key is None else f"knn_union within obs[{sample_key!r}]"
    top = max(layers)
    blocks = sum(1 if l == 0 else len(aggs) for l in layers)
    logger.info(f"Neighbourhood aggregation: {n:,} cells x {d} features, layers {layers}, {'+'.join(aggs)}")
    ctx = _lib.default_context(device)
    if A is None:
        A = knn_union_graph(ctx, xy, groups, n_neighbors, n)
    out = np.empty((n, d * blocks), dtype=np.float64)
    entries, longest, empty = [], [], []
    col = 0
    if layers[0] == 0:
        out[:, :d] = X
        col = d
    if top >= 1:
        ctx.hop_begin(A.indptr, A.indices, n)
        try:
            degree = np.diff(A.indptr)
            stats = (int(A.nnz), int(degree.max()), int(np.count_nonzero(degree == 0)))
            for l in range(1, top + 1):
                if l > 1:
                    stats = ctx.hop_next()
                entries.append(stats[0]), longest.append(stats[1]), empty.append(stats[2])
                if l in layers:
                    for a in aggs:
                        out[:, col:col + d] = ctx.hop_aggregate(X, a)
                        col += d
        finally:
            ctx.hop_end()
    adata = adata.copy() if copy else adata
    params = {"n_layers": layers, "aggregations": aggs, "use_rep": use_rep, "sample_key": sample_key, "out_key": out_key,
              "connectivity_key": connectivity_key if isinstance(connectivity_key, str) else None,
              "spatial_key": spatial_key if connectivity_key is None else None,
              "n_neighbors": int(n_neighbors) if connectivity_key is None else None}
    adata.obsm[out_key] = out
    adata.uns[out_key] = {
        "params": params, "layers": layers, "aggregations": aggs, "n_features": d,
        "graph": {"source": source, "n_neighbors": int(n_neighbors) if connectivity_key is None else None, "stored_entries": int(A.nnz)},
        "shell_entries": entries, "shell_max": longest, "shell_empty": empty}
    update_metadata(adata, "aggregate_neighbors", params, {"obsm": out_key, "uns": out_key})
    return adata
