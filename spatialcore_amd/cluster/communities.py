"""louvain: deterministic Louvain communities of the cells' neighbour graph (sc_louvain_*).

This is Louvain with a connectivity split, not Leiden: synchronous modularity moves with an alternating direction rule,
then every community of the best partition is cut into its connected components before the graph is aggregated.  Edge
weights are quantised to integers in [1, 65535] and every comparison is decided in exact integer arithmetic on the
device, so the labels are a function of the arguments alone, bit for bit; there is no ``random_state``.  Parity with
scanpy / igraph / leidenalg is not pinned: they visit the vertices in a seeded random order.  There is no CPU fallback."""

from __future__ import annotations

import numbers

import numpy as np
import pandas as pd

from spatialcore_amd import _lib
from spatialcore_amd._cell_graph import symmetric_graph      # its name stays importable from here
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd._rep_graph import K_MAX, _check_key, representation, resident_graph

logger = get_logger("cluster")

G_ONE = 1 << 16                       # the resolution's fixed point
RESOLUTION_MIN, RESOLUTION_MAX = 2.0 ** -16, 128.0
Q_MAX = 65535
WEIGHTS = ("kernel", "binary")


# ---- arguments and host checks -----------------------------------------------------------------------------------------------
def resolution_units(resolution) -> int:
    """``g = rint(resolution 2^16)``; the effective resolution is ``g / 2^16``."""
    if not isinstance(resolution, numbers.Real) or isinstance(resolution, bool) or not np.isfinite(resolution) \
            or not RESOLUTION_MIN <= resolution <= RESOLUTION_MAX:
        raise ValueError(f"resolution must be a number in [2^-16, 128], got {resolution!r}")
    return int(np.rint(float(resolution) * G_ONE))


def quantise_weights(w):
    """``q = max(1, rint(w / w_max 65535))`` as uint16 and the scale ``w_max / 65535`` one unit of q stands for."""
    w = np.asarray(w, dtype=np.float64)
    if w.size == 0:
        return np.zeros(0, dtype=np.uint16), 1.0
    w_max = float(w.max())
    q = np.maximum(1.0, np.rint(w / w_max * float(Q_MAX)))
    return q.astype(np.uint16), w_max / Q_MAX


def _check_arguments(resolution, weights, max_rounds, key_added, copy) -> int:
    g = resolution_units(resolution)
    if weights not in WEIGHTS:
        raise ValueError(f"weights must be one of {WEIGHTS}, got {weights!r}")
    if not isinstance(max_rounds, numbers.Integral) or isinstance(max_rounds, bool) or not 1 <= max_rounds <= 2**31 - 1:
        raise ValueError(f"max_rounds must be an integer in 1..2^31 - 1, got {max_rounds!r}")
    _check_key("key_added", key_added)
    if not isinstance(copy, (bool, np.bool_)):
        raise ValueError(f"copy must be True or False, got {copy!r}")
    return g


# ---- the hierarchy --------------------------------------------------------------------------------------------------------------
def run_levels(ctx, n: int):
    """Every level of the hierarchy begun on ``ctx``: (final labels, the levels' records, labels included)."""
    levels = []
    while True:
        lv = ctx.louvain_level()
        levels.append(lv)
        if lv["finished"]:
            break
    return ctx.louvain_labels(n), levels


def louvain(adata, resolution: float = 1.0, *, graph=None, use_rep: str = "X_pca", n_neighbors: int = 15,
            weights: str = "kernel", max_rounds: int = 500, key_added: str = "louvain", copy: bool = False, device: int = 0):
    """Unsupervised graph clustering of the cells: Louvain modularity optimisation with a connectivity split, on the GPU.

    ``graph=None`` builds the exact ``n_neighbors``-nearest-neighbour graph of ``obsm[use_rep]`` (at most 64 columns,
    2 <= ``n_neighbors`` <= 32) and its symmetric union with ``diffusion_map``'s kernel weights, by the search and the
    graph of ``neighbors`` (spatialcore_amd/_rep_graph.py): what ``graph="connectivities"`` reads back; ``weights="binary"`` gives
    every edge of that union the weight 1.  ``graph`` may instead name an ``obsp`` entry or be a scipy sparse matrix:
    cells x cells, finite, positive, symmetric in structure and value (diagonal entries are legal, empty rows and several
    components too); ``use_rep``, ``n_neighbors`` and ``weights="kernel"`` are then ignored, ``weights="binary"`` still
    replaces the values by 1.  Weights are quantised to ``q = max(1, rint(w / w_max 65535))`` and ``resolution``, in
    [2^-16, 128], to a multiple of 2^-16.  A level that ends at ``max_rounds`` logs a warning and is still a valid result.

    Writes ``obs[key_added]`` (an ordered Categorical of "0", "1", ... by descending cluster size) and ``uns[key_added]`` =
    {``params``, ``levels`` (``n_vertices``, ``rounds``, ``n_communities``, ``modularity`` per level), ``modularity``,
    ``hit_max_rounds``}, and appends the usual entry to ``uns["spatialcore_metadata"]``.  The result is a function of the
    arguments alone, bit for bit.  This is not Leiden, and parity with scanpy / igraph / leidenalg is not pinned."""
    g = _check_arguments(resolution, weights, max_rounds, key_added, copy)
    n = int(adata.n_obs)
    if not 1 <= n <= 2**31 - 1:
        raise ValueError(f"louvain needs 1 <= cells <= 2^31 - 1, got {n}")
    A = R = None
    if graph is not None:
        A = symmetric_graph(adata, graph, n)
        q, scale = (np.ones(A.nnz, dtype=np.uint16), 1.0) if weights == "binary" else quantise_weights(A.data)
    else:
        if not isinstance(n_neighbors, numbers.Integral) or isinstance(n_neighbors, bool) or not 2 <= n_neighbors <= K_MAX:
            raise ValueError(f"n_neighbors must be an integer in 2..{K_MAX}, got {n_neighbors!r}")
        R = representation(adata, use_rep)
        if n <= n_neighbors:
            raise ValueError(f"n_neighbors={n_neighbors} needs more than {n_neighbors} cells, got {n}")
    ctx = _lib.default_context(device)
    try:
        if A is not None:
            ctx.louvain_begin(A.indptr, A.indices, q, g, int(max_rounds))
            n_edges = int(A.nnz)
        else:
            n_edges = resident_graph(ctx, R, int(n_neighbors))["n_edges"]
            if weights == "binary":
                q, scale = None, 1.0
            else:
                q, scale = quantise_weights(ctx.louvain_resident_weights())
            ctx.louvain_begin_resident(q, g, int(max_rounds))
        labels, levels = run_levels(ctx, n)
    finally:
        ctx.louvain_end()
    M = int(q.sum(dtype=np.uint64)) if q is not None else n_edges
    denom = float(G_ONE * M * M)
    hit = any(lv["hit_max_rounds"] for lv in levels)
    for k, lv in enumerate(levels):
        if lv["hit_max_rounds"]:
            logger.warning(f"louvain: level {k} ended at max_rounds={max_rounds} before the modularity stopped improving")
    n_clusters = int(labels.max()) + 1
    adata = adata.copy() if copy else adata
    names = [str(c) for c in range(n_clusters)]
    adata.obs[key_added] = pd.Categorical.from_codes(labels.astype(np.int64), categories=names, ordered=True)
    source = graph if isinstance(graph, str) else ("<matrix>" if graph is not None else None)
    params = {"resolution": g / G_ONE, "n_neighbors": int(n_neighbors) if A is None else None,
              "use_rep": use_rep if A is None else None, "graph": source, "weights": weights, "weight_scale": float(scale),
              "max_rounds": int(max_rounds)}
    adata.uns[key_added] = {
        "params": params,
        "levels": [{"n_vertices": lv["n_vertices"], "rounds": lv["rounds"], "n_communities": lv["n_communities"],
                    "modularity": lv["qnum"] / denom if M else 0.0} for lv in levels],
        "modularity": levels[-1]["qnum"] / denom if M else 0.0,
        "hit_max_rounds": bool(hit),
    }
    logger.info(f"louvain: {n:,} cells, {n_edges:,} stored entries -> {n_clusters} clusters in {len(levels)} levels "
                f"({', '.join(str(lv['rounds']) for lv in levels)} rounds), modularity {adata.uns[key_added]['modularity']:.4f}")
    update_metadata(adata, "louvain", {**params, "key_added": key_added, "n_clusters": n_clusters},
                    {"obs": key_added, "uns": key_added})
    return adata
