"""ingest: map cells onto an annotated reference by their exact nearest reference cells.

The search (sc_knn_cross: the kernels of ``neighbors`` in their cross form -- the queries are a second array and no
candidate is excluded) and the two gathers (sc_cross_vote: labels by vote, sc_cross_regress: embeddings by neighbour
average) run in HIP; the host checks the arguments, turns ``obs`` columns into codes and back, and writes the results.
There is no CPU fallback."""

from __future__ import annotations

import numbers
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd
from scipy import sparse

from spatialcore_amd import _lib
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd._rep_graph import _check_key, representation

logger = get_logger("ingest")

K_MIN, K_MAX = 1, 32
C_MAX = 64
WEIGHTS = ("uniform", "distance")


def _names(what: str, value) -> List[str]:
    """``obs`` / ``obsm`` as given -> a list of distinct non-empty strings (None: empty)."""
    if value is None:
        return []
    names = [value] if isinstance(value, str) else list(value)
    for name in names:
        _check_key(f"an entry of {what}", name)
    if len(set(names)) != len(names):
        raise ValueError(f"{what} names a key twice: {names}")
    return names


def _both_representations(adata, adata_ref, use_rep) -> Tuple[np.ndarray, np.ndarray]:
    R = representation(adata_ref, use_rep)
    if use_rep not in adata.obsm:
        raise ValueError(f"use_rep={use_rep!r} is an entry of adata_ref.obsm but not of adata.obsm (available: "
                         f"{sorted(adata.obsm)}): project the new cells into the reference's representation first, "
                         f"e.g. project_pca(adata, adata_ref)")
    Q = representation(adata, use_rep)
    if Q.shape[1] != R.shape[1]:
        raise ValueError(f"obsm[{use_rep!r}] has {Q.shape[1]} columns in adata and {R.shape[1]} in adata_ref")
    if Q.shape[0] < 1:
        raise ValueError("adata holds no cells")
    return Q, R


def _check_k(n_neighbors, n_ref: int) -> int:
    if not isinstance(n_neighbors, numbers.Integral) or isinstance(n_neighbors, bool) or not K_MIN <= n_neighbors <= K_MAX \
            or n_neighbors > n_ref:
        raise ValueError(f"n_neighbors must be an integer in {K_MIN}..{K_MAX} and at most the {n_ref} reference cells, got "
                         f"{n_neighbors!r}")
    return int(n_neighbors)


def _codes(adata_ref, col: str) -> Tuple[np.ndarray, pd.Index]:
    """Column ``col`` of ``adata_ref.obs`` as (int32 codes, categories): a categorical keeps its categories in their
    order, the unused ones included; strings, bools and integers get their sorted unique values."""
    if col not in adata_ref.obs:
        raise ValueError(f"obs column {col!r} is not in adata_ref.obs (available: {sorted(adata_ref.obs.columns)})")
    s = adata_ref.obs[col]
    if s.isna().any():
        raise ValueError(f"adata_ref.obs[{col!r}] has missing values (first at row {int(np.flatnonzero(s.isna().values)[0])})")
    if isinstance(s.dtype, pd.CategoricalDtype):
        return np.asarray(s.cat.codes, dtype=np.int32), s.cat.categories
    values = s.values
    kind = np.asarray(values).dtype.kind
    if kind == "O" or pd.api.types.is_string_dtype(s.dtype):
        if not all(isinstance(v, str) for v in values):
            raise ValueError(f"adata_ref.obs[{col!r}] must be categorical, string, bool or integer; it holds other objects")
        values = np.asarray(values, dtype=object).astype(str)
    elif kind not in "biu":
        raise ValueError(f"adata_ref.obs[{col!r}] must be categorical, string, bool or integer, got {s.dtype}")
    cats, inverse = np.unique(np.asarray(values), return_inverse=True)
    return inverse.astype(np.int32).ravel(), pd.Index(cats)


def _ref_matrix(adata_ref, key: str) -> np.ndarray:
    if key not in adata_ref.obsm:
        raise ValueError(f"obsm key {key!r} is not in adata_ref.obsm (available: {sorted(adata_ref.obsm)})")
    Y = adata_ref.obsm[key]
    Y = Y.toarray() if sparse.issparse(Y) else np.asarray(getattr(Y, "values", Y))
    if Y.ndim != 2 or Y.dtype == object or not (np.issubdtype(Y.dtype, np.number) or Y.dtype == bool) \
            or np.issubdtype(Y.dtype, np.complexfloating):
        raise ValueError(f"adata_ref.obsm[{key!r}] must be a real 2-D array, got shape {Y.shape} of {Y.dtype}")
    if not 1 <= Y.shape[1] <= C_MAX:
        raise ValueError(f"adata_ref.obsm[{key!r}] has {Y.shape[1]} columns; 1..{C_MAX} are supported")
    if Y.dtype not in (np.float32, np.float64):
        Y = Y.astype(np.float64)
    Y = np.ascontiguousarray(Y)
    if not np.all(np.isfinite(Y)):
        raise ValueError(f"adata_ref.obsm[{key!r}] contains NaN or infinite values")
    return Y


def query_neighbors(adata, adata_ref, n_neighbors: int = 15, use_rep: str = "X_pca", *, device: int = 0):
    """For every cell of ``adata`` its ``n_neighbors`` nearest cells of ``adata_ref`` in ``obsm[use_rep]`` (Euclidean),
    exactly, on the GPU: ``(indices int32, distances float64)``, both ``(n_obs, n_neighbors)``, nearest first, ties to the
    lower reference index -- the contract of sklearn's ``NearestNeighbors(algorithm="brute").fit(ref).kneighbors(query)``.
    A distance is ``sqrt(d2)`` of the squared distance added in column order in fp64.  1 <= ``n_neighbors`` <= 32 counts
    reference cells and may equal their number; a cell present in both objects finds itself at distance 0.  A pure
    function of its arguments: it writes nothing to either object."""
    Q, R = _both_representations(adata, adata_ref, use_rep)
    k = _check_k(n_neighbors, R.shape[0])
    idx, d2, _ = _lib.default_context(device).knn_cross(R, Q, k)
    return idx, np.sqrt(d2)


def ingest(adata, adata_ref, obs: Union[None, str, Sequence[str]] = None, obsm: Union[None, str, Sequence[str]] = None, *,
           use_rep: str = "X_pca", n_neighbors: int = 15, weights: str = "uniform", key_added: str = "ingest",
           store_proba: bool = False, copy: bool = False, device: int = 0):
    """Map the cells of ``adata`` onto the annotated reference ``adata_ref`` (scanpy's ``tl.ingest``): every cell finds
    its ``n_neighbors`` nearest REFERENCE cells in ``obsm[use_rep]`` -- which both objects must hold with the same
    column count (``project_pca(adata, adata_ref)`` puts new cells into a reference's PCA) -- and takes labels from them
    by vote and embeddings by their average.

    ``obs``: a column of ``adata_ref.obs`` or a list of them, categorical, string, bool or integer, without missing
    values.  Writes ``adata.obs[col]`` as a Categorical with the reference's categories in the reference's order, unused
    ones included (sorted unique values for a column that is not categorical), ``adata.obs[col + "_confidence"]``
    (float64: the winning class's share of the vote) and, with ``store_proba``, ``adata.obsm[col + "_proba"]`` (float64,
    one column per category).  ``weights="uniform"``: the class with the most neighbours, the first category on ties;
    ``"distance"``: sklearn's ``weights="distance"`` (1 / distance; a cell at distance 0 from reference cells takes
    their vote alone).  ``obsm``: a key of ``adata_ref.obsm`` or a list of them (real, 2-D, at most 64 columns, e.g.
    ``"X_umap"`` or ``"X_pca_harmony"``).  Writes ``adata.obsm[key]`` (float64): the neighbours' weighted average.  At
    least one of ``obs`` and ``obsm`` is required.

    Always writes ``adata.obs[key_added + "_distance"]`` (the distance to the nearest reference cell: how far a cell lies
    from the atlas), ``adata.uns[key_added]`` = {``params``, ``n_ref``, ``obs``, ``obsm``, ``search`` (as
    ``neighbors``'s)} and the usual entry of ``uns["spatialcore_metadata"]``.  Nothing is written if anything raises.

    Differences from scanpy's ``ingest``: an embedding is the neighbour average, which is umap-learn's ``transform``
    INITIALISATION -- no refinement epochs follow; ``n_neighbors`` counts reference cells; only the Euclidean metric."""
    _check_key("key_added", key_added)
    obs_cols, obsm_keys = _names("obs", obs), _names("obsm", obsm)
    if not obs_cols and not obsm_keys:
        raise ValueError("ingest needs at least one of obs (columns of adata_ref.obs) and obsm (keys of adata_ref.obsm)")
    if weights not in WEIGHTS:
        raise ValueError(f"weights must be one of {WEIGHTS}, got {weights!r}")
    Q, R = _both_representations(adata, adata_ref, use_rep)
    k = _check_k(n_neighbors, R.shape[0])
    coded = [(col,) + _codes(adata_ref, col) for col in obs_cols]
    mats = [(key, _ref_matrix(adata_ref, key)) for key in obsm_keys]

    ctx = _lib.default_context(device)
    logger.info(f"ingest: {Q.shape[0]:,} cells onto {R.shape[0]:,} reference cells x {R.shape[1]} features, {k} neighbours")
    _, d2, search = ctx.knn_cross(R, Q, k)
    new_obs, new_obsm = {}, {}
    for col, codes, cats in coded:
        label, conf, proba = ctx.cross_vote(codes, len(cats), weights, proba=bool(store_proba))
        new_obs[col] = pd.Categorical.from_codes(label, categories=cats)
        new_obs[col + "_confidence"] = conf
        if store_proba:
            new_obsm[col + "_proba"] = proba
    for key, Y in mats:
        new_obsm[key] = ctx.cross_regress(Y, weights)
    new_obs[key_added + "_distance"] = np.sqrt(d2[:, 0])

    adata = adata.copy() if copy else adata
    for name, values in new_obs.items():
        adata.obs[name] = values
    for name, values in new_obsm.items():
        adata.obsm[name] = values
    params = {"n_neighbors": k, "weights": weights, "metric": "euclidean", "use_rep": use_rep, "n_features": int(R.shape[1])}
    adata.uns[key_added] = {"params": params, "n_ref": int(R.shape[0]), "obs": list(obs_cols), "obsm": list(obsm_keys),
                            "search": search}
    update_metadata(adata, "ingest", {**params, "obs": list(obs_cols), "obsm": list(obsm_keys), "key_added": key_added,
                                      "store_proba": bool(store_proba)},
                    {"obs": list(new_obs), "obsm": list(new_obsm), "uns": key_added})
    return adata
