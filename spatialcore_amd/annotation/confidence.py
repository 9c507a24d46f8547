"""transform_confidence: the reference's confidence transforms of a decision-score matrix (annotation/confidence.py:37-168),
evaluated by the device epilogue that annotate_celltypist fuses into its row pass (sc_annot_transform)."""

from __future__ import annotations

import numpy as np

from spatialcore_amd import _lib

METHODS = ("raw", "zscore", "softmax", "minmax")


def check_method(method) -> str:
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f"Unknown confidence method: {method}. Expected one of: raw, zscore, softmax, minmax")
    return method


def transform_confidence(decision_scores, method: str = "zscore", *, device: int = 0) -> np.ndarray:
    """Confidence of the winning (first largest) score of every row of an (n_cells, n_types) matrix: ``"raw"`` the score
    itself, ``"zscore"`` ``expit((max - mean) / std)`` (a std below 1e-10 counts as 1), ``"softmax"`` its softmax
    probability, ``"minmax"`` its position in the row's range (a range below 1e-10 counts as 1).  float32 scores are
    widened exactly and everything is computed in fp64; the result is float64."""
    S = np.asarray(decision_scores)
    if S.ndim != 2:
        raise ValueError(f"Expected 2D array of shape (n_cells, n_types), got shape {S.shape}")
    n_cells, n_types = S.shape
    if n_types < 2:
        raise ValueError(f"Expected at least 2 cell types, got {n_types}")
    check_method(method)
    if n_types > 256:
        raise ValueError(f"at most 256 cell types are supported, got {n_types}")
    if S.dtype == object or not np.issubdtype(S.dtype, np.number):
        raise ValueError("decision_scores must be numeric")
    if S.dtype not in (np.float32, np.float64):
        S = S.astype(np.float64)
    if not np.all(np.isfinite(S)):
        raise ValueError("decision_scores contains NaN or infinite values")
    if n_cells == 0:
        return np.empty(0, dtype=np.float64)
    return _lib.default_context(device).annot_transform(S)[method].copy()
