"""fit_spatial_nmf: graph-regularised NMF (GNMF; Cai, He, Han & Huang, IEEE TPAMI 2011) on the spatial graph of the
cells (sc_nmf_fit_graph).

    F(W, H) = 1/2 ||X - W H||_F^2 + (spatial_alpha / 2) tr(W^T L W),   L = diag(d) - A

The host resolves the genes, hands the library a canonical CSR and a symmetric cell-cell graph (by default the union of
the exact 2-D kNN lists, searched on the device) and replays sklearn's ``init="random"``; every iteration and every
evaluation of the objective runs in HIP, in fp64 and in one documented summation order.  There is no CPU fallback."""

from __future__ import annotations

import numbers
from typing import Optional, Sequence, Union

import numpy as np

from spatialcore_amd import _lib
from spatialcore_amd._batches import batch_groups
from spatialcore_amd._cell_graph import given_graph as _given_graph      # its earlier name stays importable from here
from spatialcore_amd._logging import get_logger
from spatialcore_amd._sparse_input import gene_columns
from spatialcore_amd._spatial_graph import K_NEIGHBORS_MAX, _coordinates, knn_union_graph
from spatialcore_amd._spatial_graph import union_of_knn  # noqa: F401  (its name stays importable from here)
from spatialcore_amd.nmf import factorize

logger = get_logger("nmf")


def _check_alpha(spatial_alpha) -> float:
    if (not isinstance(spatial_alpha, numbers.Real) or isinstance(spatial_alpha, bool) or not np.isfinite(spatial_alpha)
            or spatial_alpha < 0):
        raise ValueError(f"spatial_alpha must be a finite number >= 0, got {spatial_alpha!r}")
    return float(spatial_alpha)


def fit_spatial_nmf(adata, n_components: int, spatial_alpha: float = 1.0, *, graph=None, spatial_key: str = "spatial",
                    n_neighbors: int = 6, batch_key: Optional[str] = None, genes: Optional[Union[str, Sequence[str]]] = None,
                    layer: Optional[str] = None, init: str = "random", max_iter: int = 200, tol: float = 1e-4, random_state=0,
                    W=None, H=None, key_added: str = "spatial_nmf", copy: bool = False, device: int = 0):
    """Spatial non-negative matrix factorisation: ``fit_nmf``'s Frobenius factorisation with a Laplacian penalty
    ``(spatial_alpha / 2) tr(W^T L W)`` on the usages over a cell-cell graph, so neighbouring cells get similar usages.
    The multiplicative update of Cai et al. (2011); the objective never rises.  ``spatial_alpha = 0`` gives ``fit_nmf``'s
    factors byte for byte.

    Graph: with ``graph=None`` the symmetric union of the exact ``n_neighbors`` nearest-neighbour lists of
    ``obsm[spatial_key]`` (2-D), weight 1.0; with ``batch_key`` the search runs inside every batch (an ``obs`` column),
    so slides whose coordinates overlap never connect.  ``graph`` may instead name an ``obsp`` entry or be a scipy sparse
    matrix: cells x cells, symmetric, positive; its diagonal is dropped.  Isolated cells get the plain update.

    The matrix, ``genes``, ``layer``, ``init`` (``"random"`` or ``"custom"`` with ``W`` and ``H``), ``max_iter``, ``tol``
    and ``random_state`` are ``fit_nmf``'s.  The objective is evaluated every tenth iteration; with ``tol > 0`` the loop
    stops when its drop, relative to the start, falls below ``tol``.

    Nothing is normalised, inside the loop or after it: the penalty rewards a small W, so W may shrink and H grow with
    ``spatial_alpha`` (their product does not).  Compare usages across runs after scaling the columns of W.

    Writes ``adata.obsm["X_" + key_added]`` and ``adata.uns[key_added]`` = ``fit_nmf``'s keys (``reconstruction_err`` is
    ``||X - W H||_F``, ``error_trace`` its values at the checks) plus ``spatial_alpha``, ``penalty`` = ``tr(W^T L W)``,
    ``objective_trace`` (``sqrt(2 F)`` at the start and at every check) and ``graph`` = {``source``, ``n_neighbors``,
    ``stored_entries``}, and appends the usual entry to ``uns["spatialcore_metadata"]``.  The result is a function of the
    arguments alone, bit for bit."""
    K = factorize._check_components(n_components)
    lam = _check_alpha(spatial_alpha)
    factorize._check_common("frobenius", max_iter, tol)
    if not isinstance(init, str) or init not in factorize.INITS:
        raise ValueError(f'init={init!r} is not supported; supported: "random" or "custom"')
    if init == "custom" and (W is None or H is None):
        raise ValueError('init="custom" needs both W (cells x n_components) and H (n_components x genes)')
    if init != "custom" and (W is not None or H is not None):
        raise ValueError('W and H are only used with init="custom"')
    if graph is not None and batch_key is not None:
        raise ValueError("batch_key restricts the kNN search and has no meaning with graph=; give one of them")
    n = int(adata.n_obs)
    groups, xy, A = None, None, None
    if graph is not None:
        A, source = _given_graph(adata, graph, n)
    else:
        if not isinstance(n_neighbors, numbers.Integral) or isinstance(n_neighbors, bool) or not 1 <= n_neighbors <= K_NEIGHBORS_MAX:
            raise ValueError(f"n_neighbors must be an integer in 1..{K_NEIGHBORS_MAX}, got {n_neighbors!r}")
        xy = _coordinates(adata, spatial_key)
        groups = batch_groups(adata, batch_key) if batch_key is not None else [(None, None)]
        smallest = min(n if rows is None else rows.size for _, rows in groups)
        if n_neighbors >= smallest:
            raise ValueError(f"n_neighbors={n_neighbors} needs more than the {smallest} cells of the smallest "
                             f"{'batch' if batch_key is not None else 'data set'}")
        source = "knn_union" if batch_key is None else f"knn_union within obs[{batch_key!r}]"
    names, cols = gene_columns(adata, genes)
    Xc, dtype = factorize._matrix(adata, layer, cols)
    G = Xc.shape[1]
    if init == "custom":
        W0, H0 = factorize._check_factor(W, (n, K), "W"), factorize._check_factor(H, (K, G), "H")
    else:
        factorize._random_state(random_state)   # its type, before anything is drawn
    logger.info(f"Spatial NMF (frobenius, graph-regularised, alpha={lam:g}): {n:,} cells x {G} genes, {K} components")
    ctx = _lib.default_context(device)
    if A is None:
        A = knn_union_graph(ctx, xy, groups, n_neighbors, n)
    if init == "random":
        W0, H0 = factorize.random_init(factorize._scale(Xc, K), n, G, K, random_state)
    res = ctx.nmf_fit_graph(Xc.indptr, Xc.indices, Xc.data, G, A.indptr, A.indices, A.data, lam, W0, H0, int(max_iter), float(tol))
    adata = adata.copy() if copy else adata
    params = {"n_components": K, "spatial_alpha": lam, "beta_loss": "frobenius", "init": init, "solver": "mu",
              "max_iter": int(max_iter), "tol": float(tol),
              "random_state": random_state if isinstance(random_state, numbers.Integral) else None, "layer": layer,
              "spatial_key": spatial_key if graph is None else None, "n_neighbors": int(n_neighbors) if graph is None else None,
              "batch_key": batch_key}
    factorize._store(adata, "fit_spatial_nmf", key_added, res, res["H"], names, dtype, params)
    adata.uns[key_added].update({
        "spatial_alpha": lam, "penalty": float(res["penalty"]), "objective_trace": res["objective_trace"],
        "graph": {"source": source, "n_neighbors": int(n_neighbors) if graph is None else None, "stored_entries": int(A.nnz)}})
    return adata
