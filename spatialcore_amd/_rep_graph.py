"""Representation -> neighbour lists -> weighted graph resident on the device: the step ``neighbors``, ``louvain(graph=None)``
and ``diffusion_map(graph=None)`` share, with the limits and host checks of its arguments.

The search is sc_knn_dense_gram at the library's own choice of path: below its size rule the direct kernels of
sc_knn_dense, above it the certified Gram-form filter; the lists are those of sc_knn_dense bit for bit either way."""

from __future__ import annotations

import numbers

import numpy as np
from scipy import sparse

D_MAX = 64
K_MIN, K_MAX = 2, 32
COMPS_MIN, COMPS_MAX = 2, 64
_SUPPORTED = (f"a finite float32 or float64 representation with 1..{D_MAX} columns, {K_MIN} <= n_neighbors <= {K_MAX}, "
              f"{COMPS_MIN} <= n_comps <= {COMPS_MAX}, both below the number of cells, one connected graph")


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _check_key(name: str, value) -> str:
    if not isinstance(value, str) or not value:
        raise ValueError(f"{name} must be a non-empty string, got {value!r}")
    return value


def check_n_neighbors(n_neighbors, n: int) -> int:
    if not _is_int(n_neighbors) or not K_MIN <= n_neighbors <= K_MAX or n_neighbors >= n:
        raise ValueError(f"n_neighbors must be an integer in {K_MIN}..{K_MAX} and below the {n} cells, got "
                         f"{n_neighbors!r}; supported: {_SUPPORTED}")
    return int(n_neighbors)


def representation(adata, use_rep) -> np.ndarray:
    if not isinstance(use_rep, str) or use_rep not in adata.obsm:
        raise ValueError(f"use_rep={use_rep!r} is not an entry of adata.obsm (available: {sorted(adata.obsm)}); "
                         f"supported: {_SUPPORTED}")
    R = adata.obsm[use_rep]
    R = R.toarray() if sparse.issparse(R) else np.asarray(getattr(R, "values", R))
    if R.ndim != 2 or R.dtype == object or not (np.issubdtype(R.dtype, np.number) or R.dtype == bool) \
            or np.issubdtype(R.dtype, np.complexfloating):
        raise ValueError(f"obsm[{use_rep!r}] must be a real 2-D array, got shape {R.shape} of {R.dtype}; supported: {_SUPPORTED}")
    if not 1 <= R.shape[1] <= D_MAX:
        raise ValueError(f"obsm[{use_rep!r}] has {R.shape[1]} columns; supported: {_SUPPORTED}")
    if R.dtype not in (np.float32, np.float64):
        R = R.astype(np.float64)
    R = np.ascontiguousarray(R)
    if not np.all(np.isfinite(R)):
        raise ValueError(f"obsm[{use_rep!r}] contains NaN or infinite values; supported: {_SUPPORTED}")
    if R.size and np.abs(R).max() >= 2.0 ** 500:
        raise ValueError(f"obsm[{use_rep!r}] holds values of magnitude 2^500 or more, whose squared distances overflow")
    return R


def resident_graph(ctx, R: np.ndarray, k: int, method: str = "gauss", fetch: bool = False) -> dict:
    """The exact ``k`` nearest neighbours of every row of ``R`` and, on their symmetric union, ``diffusion_map``'s kernel
    weights (``method="gauss"``) or UMAP's fuzzy simplicial set (``"umap"``), left resident on ``ctx`` for
    ``diffmap_graph_get``, ``louvain_begin_resident`` and the Lanczos steps.  A zero local scale raises in the "gauss" graph.
    Returns ``n_edges``, ``n_components``, ``search`` (how the search went) and, with ``fetch``, the lists ``idx`` and ``d2``."""
    idx, d2, search = ctx.knn_dense_gram(R, k, fetch=fetch)
    info = ctx.fuzzy_graph() if method == "umap" else ctx.diffmap_graph()
    return {"n_edges": int(info["n_edges"]), "n_components": int(info["n_components"]), "search": search, "idx": idx, "d2": d2}
