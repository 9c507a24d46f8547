"""gaussian_mixture: spatial domains as the components of a multivariate Gaussian mixture on the GPU (sc_mixture_*,
DESIGN.md 4.6y) -- the clusterer CellCharter (Varrone et al., Nature Genetics 2024) runs on the features of
``aggregate_neighbors``.

``gaussian_mixture`` is sklearn 1.7.2's ``GaussianMixture(init_params="kmeans").fit_predict`` for full and diagonal
covariances, step for step and in fp64; parity with sklearn is pinned by the tests.  ``gaussian_mixture_autok`` restates
CellCharter's ``ClusterAutoK`` stability rule from its published description: cellcharter (and its pycave mixture) is
not installed here, so neither the agreement of the rule nor that of the fitted mixtures with a cellcharter run is
pinned.  The EM passes over the cells run in HIP; there is no CPU fallback."""

from __future__ import annotations

import numbers
import warnings
from typing import Optional, Tuple

import numpy as np
import pandas as pd

from spatialcore_amd import _lib
from spatialcore_amd._kmeans_draws import kmeans_draws
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata

logger = get_logger("mixture")

COVARIANCE_TYPES = ("full", "diag")
KMEANS_MAX_ITER = 300   # sklearn's KMeans defaults, which GaussianMixture's initialisation uses
KMEANS_TOL = 1e-4


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _check_key(name: str, value, optional: bool = False) -> None:
    if value is None and optional:
        return
    if not isinstance(value, str) or not value:
        raise ValueError(f"{name} must be a non-empty string, got {value!r}")


def _check_fit_arguments(n_clusters, covariance_type, n_init, max_iter, tol, reg_covar, random_state) -> None:
    if not _is_int(n_clusters) or not 1 <= n_clusters <= _lib.MIX_K_MAX:
        raise ValueError(f"n_clusters must be an integer in 1 .. {_lib.MIX_K_MAX}, got {n_clusters!r}")
    if covariance_type in ("tied", "spherical"):
        raise ValueError(f"covariance_type={covariance_type!r} is not supported: only 'full' and 'diag' are")
    if covariance_type not in COVARIANCE_TYPES:
        raise ValueError(f"covariance_type must be 'full' or 'diag', got {covariance_type!r}")
    if not _is_int(n_init) or not 1 <= n_init <= _lib.MIX_N_INIT_MAX:
        raise ValueError(f"n_init must be an integer in 1 .. {_lib.MIX_N_INIT_MAX}, got {n_init!r}")
    if not _is_int(max_iter) or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
    for name, v in (("tol", tol), ("reg_covar", reg_covar)):
        if not isinstance(v, numbers.Real) or isinstance(v, bool) or not np.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    if not _is_int(random_state) or not 0 <= random_state < 2 ** 32:
        raise ValueError(f"random_state must be an integer in 0 .. 2^32 - 1, got {random_state!r}")


def _representation(adata, use_rep, n_clusters: int = 1, dims: Optional[int] = None) -> np.ndarray:
    _check_key("use_rep", use_rep)
    if use_rep not in adata.obsm:
        raise ValueError(f"obsm[{use_rep!r}] not found (run aggregate_neighbors first, or pass use_rep)")
    X = adata.obsm[use_rep]
    X = X.toarray() if hasattr(X, "toarray") else np.asarray(X)
    if X.ndim != 2 or X.dtype not in (np.float32, np.float64):
        raise ValueError(f"obsm[{use_rep!r}] must be a 2-D float32 or float64 array, got {X.dtype} {X.shape}")
    n, D = X.shape
    if not 1 <= D <= _lib.MIX_D_MAX:
        raise ValueError(f"obsm[{use_rep!r}] has {D} columns, need 1 .. {_lib.MIX_D_MAX}")
    if dims is not None and D != dims:
        raise ValueError(f"obsm[{use_rep!r}] has {D} columns, the mixture was fitted on {dims}")
    if n < 1 or n_clusters > n:
        raise ValueError(f"n_clusters ({n_clusters}) cannot exceed the number of cells ({n})")
    if not np.isfinite(X).all():
        raise ValueError(f"obsm[{use_rep!r}] holds non-finite values")
    return np.ascontiguousarray(X)


def n_parameters(K: int, D: int, covariance_type: str) -> int:
    """sklearn's GaussianMixture._n_parameters."""
    cov = K * D * (D + 1) // 2 if covariance_type == "full" else K * D
    return int(cov + D * K + K - 1)


def information_criteria(loglik: float, n: int, K: int, D: int, covariance_type: str) -> Tuple[float, float]:
    """(bic, aic) as sklearn's GaussianMixture.bic / .aic from the mean log-likelihood of the n cells."""
    p = n_parameters(K, D, covariance_type)
    return -2.0 * loglik * n + p * np.log(n), -2.0 * loglik * n + 2.0 * p


def fowlkes_mallows(a, b) -> float:
    """Fowlkes-Mallows index of two labellings (non-negative integer codes), as sklearn.metrics.fowlkes_mallows_score: from
    the contingency table in exact int64 (``bincount`` of ``a * K2 + b``)."""
    a, b = np.asarray(a, dtype=np.int64).ravel(), np.asarray(b, dtype=np.int64).ravel()
    if a.size != b.size or a.size == 0:
        raise ValueError("fowlkes_mallows: the labellings must have the same non-zero length")
    if a.min() < 0 or b.min() < 0:
        raise ValueError("fowlkes_mallows: labels must be non-negative integers")
    K1, K2 = int(a.max()) + 1, int(b.max()) + 1
    c = np.bincount(a * K2 + b, minlength=K1 * K2).reshape(K1, K2)
    n = a.size
    tk = int((c * c).sum()) - n
    pk = int((c.sum(axis=1) ** 2).sum()) - n
    qk = int((c.sum(axis=0) ** 2).sum()) - n
    return float(np.sqrt(tk / pk) * np.sqrt(tk / qk)) if tk != 0 else 0.0


def autok_rule(labels_by_k: dict, lo: int, hi: int):
    """CellCharter's stability rule on ``labels_by_k[K]`` = the labellings of the runs at K, K = lo - 1 .. hi + 1:
    s(K) = the mean Fowlkes-Mallows index over all run pairs (one at K, one at K + 1), stability(K) = (s(K - 1) + s(K)) / 2
    for K = lo .. hi; the chosen K is the smallest of maximal stability.  Returns (best_k, stability, similarity)."""
    sim = {}
    for K in range(lo - 1, hi + 1):
        vals = [fowlkes_mallows(a, b) for a in labels_by_k[K] for b in labels_by_k[K + 1]]
        sim[K] = float(np.mean(vals))
    stability = {K: (sim[K - 1] + sim[K]) / 2.0 for K in range(lo, hi + 1)}
    best = min(K for K in stability if stability[K] == max(stability.values()))
    return best, stability, sim


def _fit(ctx, X: np.ndarray, K: int, covariance_type: str, n_init: int, max_iter: int, tol: float, reg_covar: float,
         random_state: int, want_proba: bool) -> dict:
    X64 = X.astype(np.float64, copy=False)            # arithmetic is fp64 whatever the input type, k-means included
    km_tol = float(np.mean(np.var(X64, axis=0)) * KMEANS_TOL)   # sklearn's KMeans._tolerance and centring
    x_mean = X64.mean(axis=0)
    draws = kmeans_draws(random_state, n_init, K) if K > 1 else None
    return ctx.mixture_fit(X, K, covariance_type, n_init, KMEANS_MAX_ITER, km_tol, x_mean, draws, max_iter, tol, reg_covar,
                           return_proba=want_proba)


def _warn_unconverged(fit: dict) -> None:
    if not fit["converged"][fit["best"]]:
        from sklearn.exceptions import ConvergenceWarning   # only where it is raised: importing the module needs no scikit-learn

        warnings.warn("Best performing initialization did not converge. Try different init parameters, or increase "
                      "max_iter, tol, or check for degenerate data.", ConvergenceWarning, stacklevel=3)


def _entry(fit: dict, params: dict, n: int, D: int) -> dict:
    best = fit["best"]
    K, cov_type = params["n_clusters"], params["covariance_type"]
    bic, aic = information_criteria(fit["loglik"], n, K, D, cov_type)
    return {
        "params": params,
        "weights": fit["weights"][best].copy(),
        "means": fit["means"][best].copy(),
        "covariances": fit["covariances"][best].copy(),
        "lower_bound": fit["lower_bound"].copy(),
        "n_iter": fit["n_iter"].astype(np.int64),
        "converged": fit["converged"].copy(),
        "best_run": int(best),
        "loglik": float(fit["loglik"]),
        "bic": float(bic),
        "aic": float(aic),
        "sizes": np.bincount(fit["labels"], minlength=K).astype(np.int64),
    }


def _write_labels(adata, key: str, labels: np.ndarray, K: int) -> None:
    adata.obs[key] = pd.Categorical.from_codes(labels, categories=[str(k) for k in range(K)], ordered=True)


def gaussian_mixture(adata, n_clusters: int, use_rep: str = "X_cellcharter", key_added: str = "spatial_cluster",
                     covariance_type: str = "full", n_init: int = 1, max_iter: int = 100, tol: float = 1e-3,
                     reg_covar: float = 1e-6, random_state: int = 0, proba_key: Optional[str] = None, copy: bool = False, *,
                     device: int = 0):
    """Cluster ``obsm[use_rep]`` into ``n_clusters`` domains with a Gaussian mixture: sklearn 1.7.2's
    ``GaussianMixture(n_components, covariance_type, n_init, max_iter, tol, reg_covar, init_params="kmeans",
    random_state).fit_predict`` for ``covariance_type`` ``"full"`` and ``"diag"``, in fp64 whatever the input type.

    Writes ``obs[key_added]`` (ordered Categorical ``"0" .. "K-1"``: the category is the component index, so it lines up with
    the stored parameters) and ``uns[key_added]``: ``params``, the best run's ``weights`` (K), ``means`` (K, D) and
    ``covariances`` (K, D, D) or (K, D); per run ``lower_bound``, ``n_iter``, ``converged``; ``best_run``; ``bic`` / ``aic``
    (sklearn's formulas) and ``sizes``.  ``proba_key`` stores the responsibilities (n, K) float64 in ``obsm``.  A fit that
    does not converge warns with sklearn's ``ConvergenceWarning``; a covariance that is not positive definite raises
    ``ValueError`` with sklearn's message.  Limits: 1 <= D <= 256, 1 <= K <= min(64, n), n_init <= 10."""
    _check_fit_arguments(n_clusters, covariance_type, n_init, max_iter, tol, reg_covar, random_state)
    _check_key("key_added", key_added)
    _check_key("proba_key", proba_key, optional=True)
    X = _representation(adata, use_rep, n_clusters)
    n, D = X.shape
    ctx = _lib.default_context(device)
    fit = _fit(ctx, X, int(n_clusters), covariance_type, int(n_init), int(max_iter), float(tol), float(reg_covar),
               int(random_state), proba_key is not None)
    _warn_unconverged(fit)
    params = {"n_clusters": int(n_clusters), "use_rep": use_rep, "key_added": key_added, "covariance_type": covariance_type,
              "n_init": int(n_init), "max_iter": int(max_iter), "tol": float(tol), "reg_covar": float(reg_covar),
              "random_state": int(random_state)}
    adata = adata.copy() if copy else adata
    _write_labels(adata, key_added, fit["labels"], int(n_clusters))
    adata.uns[key_added] = _entry(fit, params, n, D)
    outputs = {"obs": key_added, "uns": key_added}
    if proba_key is not None:
        adata.obsm[proba_key] = fit["proba"]
        outputs["obsm"] = proba_key
    logger.info(f"gaussian_mixture: {n:,} cells, D={D}, K={n_clusters} ({covariance_type}), "
                f"lower bound {fit['lower_bound'][fit['best']]:.6g}")
    update_metadata(adata, "gaussian_mixture", params, outputs)
    return adata if copy else None


def _model_entry(model, key_added) -> dict:
    entry = model
    if hasattr(model, "uns"):
        key = key_added if key_added is not None else "spatial_cluster"
        if key not in model.uns:
            raise ValueError(f"model.uns[{key!r}] not found: pass the uns entry of gaussian_mixture, or its key as key_added")
        entry = model.uns[key]
    if not isinstance(entry, dict) or not all(k in entry for k in ("params", "weights", "means", "covariances")):
        raise ValueError("model must be the uns entry gaussian_mixture wrote (params, weights, means, covariances) or an "
                         "AnnData carrying it")
    cov_type = entry["params"].get("covariance_type")
    if cov_type not in COVARIANCE_TYPES:
        raise ValueError(f"model: covariance_type must be 'full' or 'diag', got {cov_type!r}")
    w, mu, cov = (np.asarray(entry[k], dtype=np.float64) for k in ("weights", "means", "covariances"))
    K = w.size
    if w.ndim != 1 or not 1 <= K <= _lib.MIX_K_MAX or mu.ndim != 2 or mu.shape[0] != K:
        raise ValueError(f"model: weights must be (K,) and means (K, D) with K <= {_lib.MIX_K_MAX}, got {w.shape} and {mu.shape}")
    D = mu.shape[1]
    if cov.shape != ((K, D, D) if cov_type == "full" else (K, D)):
        raise ValueError(f"model: covariances have shape {cov.shape}, which does not fit {cov_type!r} with K={K}, D={D}")
    if not (np.isfinite(w).all() and (w > 0).all() and np.isfinite(mu).all() and np.isfinite(cov).all()):
        raise ValueError("model: weights must be finite and > 0, means and covariances finite")
    return entry


def predict_gaussian_mixture(adata, model, use_rep: Optional[str] = None, key_added: Optional[str] = None,
                             proba_key: Optional[str] = None, copy: bool = False, *, device: int = 0):
    """Apply a fitted mixture to other cells, as ``project_pca`` does for ``pca``.  ``model`` is the ``uns`` entry
    ``gaussian_mixture`` wrote, or an AnnData carrying it (under ``key_added``, default ``"spatial_cluster"``); ``use_rep`` and
    ``key_added`` default to the fit's.  Writes ``obs[key_added]``, optionally ``obsm[proba_key]``, and ``uns[key_added]``:
    the parameters with ``loglik``, the mean log-likelihood of these cells, and their ``sizes``.  On the fitted cells the
    labels and responsibilities are the fit's, byte for byte."""
    _check_key("use_rep", use_rep, optional=True)
    _check_key("key_added", key_added, optional=True)
    _check_key("proba_key", proba_key, optional=True)
    entry = _model_entry(model, key_added)
    p = entry["params"]
    use_rep = use_rep if use_rep is not None else p.get("use_rep")
    key_added = key_added if key_added is not None else p.get("key_added", "spatial_cluster")
    w, mu, cov = (np.asarray(entry[k], dtype=np.float64) for k in ("weights", "means", "covariances"))
    K, D = mu.shape
    X = _representation(adata, use_rep, 1, dims=D)
    ctx = _lib.default_context(device)
    labels, proba, loglik = ctx.mixture_predict(X, p["covariance_type"], w, mu, cov, return_proba=proba_key is not None)
    adata = adata.copy() if copy else adata
    _write_labels(adata, key_added, labels, K)
    params = dict(p, use_rep=use_rep, key_added=key_added)
    adata.uns[key_added] = {"params": params, "weights": w.copy(), "means": mu.copy(), "covariances": cov.copy(),
                            "loglik": float(loglik), "sizes": np.bincount(labels, minlength=K).astype(np.int64)}
    outputs = {"obs": key_added, "uns": key_added}
    if proba_key is not None:
        adata.obsm[proba_key] = proba
        outputs["obsm"] = proba_key
    update_metadata(adata, "predict_gaussian_mixture", params, outputs)
    return adata if copy else None


def _check_autok_arguments(n_clusters, max_runs) -> Tuple[int, int]:
    ok = isinstance(n_clusters, (tuple, list)) and len(n_clusters) == 2 and all(_is_int(v) for v in n_clusters)
    if not ok or not 2 <= n_clusters[0] <= n_clusters[1] or n_clusters[1] + 1 > _lib.MIX_K_MAX:
        raise ValueError(f"n_clusters must be (lo, hi) with 2 <= lo <= hi <= {_lib.MIX_K_MAX - 1}, got {n_clusters!r}")
    if not _is_int(max_runs) or not 1 <= max_runs <= 100:
        raise ValueError(f"max_runs must be an integer in 1 .. 100, got {max_runs!r}")
    return int(n_clusters[0]), int(n_clusters[1])


def gaussian_mixture_autok(adata, n_clusters: Tuple[int, int] = (2, 10), max_runs: int = 5, use_rep: str = "X_cellcharter",
                           key_added: str = "spatial_cluster", covariance_type: str = "full", max_iter: int = 100,
                           tol: float = 1e-3, reg_covar: float = 1e-6, random_state: int = 0, copy: bool = False, *,
                           device: int = 0):
    """Choose the number of domains by the stability of the clustering: CellCharter's ``ClusterAutoK``, restated from its
    published description (cellcharter is not installed here, so the rule's agreement with cellcharter's is not pinned; its
    early stopping is not restated).

    For ``n_clusters = (lo, hi)`` every K in ``lo - 1 .. hi + 1`` is fitted ``max_runs`` times (run r with
    ``random_state + r``, ``n_init=1``).  s(K) is the mean over all ``max_runs**2`` run pairs of the Fowlkes-Mallows index
    between a labelling at K and one at K + 1; stability(K) = (s(K - 1) + s(K)) / 2; the chosen K is the smallest K of maximal
    stability.  Writes the best run (largest lower bound) at that K as ``gaussian_mixture`` does, and
    ``uns[key_added + "_autok"]``: ``n_clusters`` (the K of ``stability``), ``stability``, ``similarity`` (per adjacent pair
    K, K + 1 from lo - 1), every run's ``lower_bound`` and ``bic`` (rows K = lo - 1 .. hi + 1), and ``best_k``."""
    lo, hi = _check_autok_arguments(n_clusters, max_runs)
    _check_fit_arguments(hi + 1, covariance_type, 1, max_iter, tol, reg_covar, random_state)
    if not _is_int(random_state) or random_state + max_runs > 2 ** 32:
        raise ValueError("random_state + max_runs must stay within 2^32")
    _check_key("key_added", key_added)
    X = _representation(adata, use_rep, hi + 1)
    n, D = X.shape
    ctx = _lib.default_context(device)
    ks = list(range(lo - 1, hi + 2))
    fits = {K: [_fit(ctx, X, K, covariance_type, 1, int(max_iter), float(tol), float(reg_covar), int(random_state) + r, False)
                for r in range(max_runs)] for K in ks}
    best_k, stability, sim = autok_rule({K: [f["labels"] for f in fits[K]] for K in ks}, lo, hi)
    lbs = np.array([[f["lower_bound"][0] for f in fits[K]] for K in ks])
    bics = np.array([[information_criteria(f["loglik"], n, K, D, covariance_type)[0] for f in fits[K]] for K in ks])
    run = int(np.argmax(lbs[ks.index(best_k)]))           # the first of equal runs
    fit = fits[best_k][run]
    _warn_unconverged(fit)
    params = {"n_clusters": best_k, "use_rep": use_rep, "key_added": key_added, "covariance_type": covariance_type,
              "n_init": 1, "max_iter": int(max_iter), "tol": float(tol), "reg_covar": float(reg_covar),
              "random_state": int(random_state) + run}
    adata = adata.copy() if copy else adata
    _write_labels(adata, key_added, fit["labels"], best_k)
    adata.uns[key_added] = _entry(fit, params, n, D)
    adata.uns[key_added + "_autok"] = {
        "n_clusters": np.arange(lo, hi + 1, dtype=np.int64),
        "stability": np.array([stability[K] for K in range(lo, hi + 1)]),
        "similarity": np.array([sim[K] for K in range(lo - 1, hi + 1)]),
        "fitted_k": np.array(ks, dtype=np.int64),
        "lower_bound": lbs,
        "bic": bics,
        "best_k": int(best_k),
        "max_runs": int(max_runs),
    }
    logger.info(f"gaussian_mixture_autok: K={best_k} of {lo}..{hi} (stability {stability[best_k]:.4f})")
    update_metadata(adata, "gaussian_mixture_autok", dict(params, n_clusters_range=[lo, hi], max_runs=int(max_runs)),
                    {"obs": key_added, "uns": [key_added, key_added + "_autok"]})
    return adata if copy else None
