"""classify_by_threshold on the GPU (reference src/spatialcore/stats/classify.py:419-894 = CL,
src/spatialcore/stats/_thresholding.py = TH): metagene score, then a KS or Gaussian-mixture cutoff.

The per-cell work runs in libspatialcore_hip.so (sc_metagene_score, sc_ks_*, sc_gmm_*).  The host does
what the reference does on O(1) or O(1000) values: the percentile interpolation of the two KS fallbacks on order
statistics read back from the device, and the 1000-point crossing search of the two-component cutoff from the fitted
parameters.  Decided differences from the reference are listed in INTEGRATION.md.
"""

from __future__ import annotations

import warnings
from pathlib import Path
from typing import List, Optional, Union

import numpy as np

from spatialcore_amd import _lib
from spatialcore_amd._kmeans_draws import kmeans_draws
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata

logger = get_logger(__name__.replace("spatialcore_amd.", ""))

METAGENE_METHODS = list(_lib.METAGENE_METHODS)
THRESHOLD_METHODS = ["ks", "gmm"]
GMM_N_INIT, GMM_MAX_ITER, GMM_TOL, GMM_REG_COVAR = 10, 100, 1e-3, 1e-6   # GaussianMixture(n_init=10) and its defaults (TH:271-276)
KMEANS_MAX_ITER = 300                                                     # KMeans' default, as the mixture's initialisation calls it


def _extract_features(adata, feature_columns: List[str]) -> np.ndarray:
    """One column per feature (CL:56-166): ``"obsm_key:column"`` (index, or gene name through
    ``uns["<base>_params"]["genes"]``), else ``obs``, else ``var_names`` (sparse or dense ``X``), else the first
    column of ``obsm[name]``."""
    columns = []
    for name in feature_columns:
        if ":" in name:
            obsm_key, spec = name.split(":", 1)
            if obsm_key not in adata.obsm:
                raise ValueError(f"obsm key '{obsm_key}' not found in adata.obsm. "
                                 f"Available keys: {list(adata.obsm.keys())}")
            table = adata.obsm[obsm_key]
            if spec.isdigit():
                j = int(spec)
                if j >= table.shape[1]:
                    raise ValueError(f"Column index {j} out of range for obsm['{obsm_key}'] "
                                     f"with {table.shape[1]} columns")
            else:
                params_key = f"{obsm_key.rsplit('_', 1)[0]}_params"
                if params_key not in adata.uns:
                    raise ValueError(f"Cannot look up column '{spec}' by name: "
                                     f"'{params_key}' not found in adata.uns. "
                                     f"Use numeric index instead (e.g., '{obsm_key}:0').")
                genes = adata.uns[params_key].get("genes", [])
                if spec not in genes:
                    raise ValueError(f"Column '{spec}' not found in {params_key}['genes']. "
                                     f"Available: {genes[:10]}{'...' if len(genes) > 10 else ''}")
                j = genes.index(spec)
            columns.append(table[:, j])
            logger.debug(f"Extracted column {j} from obsm['{obsm_key}']")
        elif name in adata.obs.columns:
            columns.append(adata.obs[name].values.astype(float))
            logger.debug(f"Found '{name}' in adata.obs")
        elif name in adata.var_names:
            j = adata.var_names.get_loc(name)
            col = adata.X[:, j]
            columns.append(col.toarray().flatten() if hasattr(adata.X, "toarray") else np.asarray(col).flatten())
            logger.debug(f"Found '{name}' in adata.var_names (gene expression)")
        elif name in adata.obsm:
            table = adata.obsm[name]
            columns.append(table if table.ndim == 1 else table[:, 0])
            logger.debug(f"Found '{name}' in adata.obsm")
        else:
            raise ValueError(f"Feature '{name}' not found in adata.obs, adata.var_names, "
                             f"or adata.obsm.\n"
                             f"Available obs columns (first 10): {list(adata.obs.columns)[:10]}\n"
                             f"Available genes (first 10): {list(adata.var_names)[:10]}")
    return np.column_stack(columns)


def _request_problem(feature_columns, metagene_method, threshold_method, pseudocount, background_quantile,
                     probability_cutoff, plot, output_dir) -> Optional[str]:
    """The reference's argument checks in its order (CL:616-658); the text of the first that fails."""
    if not isinstance(feature_columns, list) or len(feature_columns) == 0:
        return "feature_columns must be a non-empty list of feature names."
    if metagene_method not in METAGENE_METHODS:
        return f"Invalid metagene_method '{metagene_method}'. Must be one of: {METAGENE_METHODS}"
    if threshold_method not in THRESHOLD_METHODS:
        return f"Invalid threshold_method '{threshold_method}'. Must be one of: {THRESHOLD_METHODS}"
    if pseudocount <= 0:
        return f"pseudocount must be > 0, got {pseudocount}"
    if not 0 < background_quantile < 1:
        return f"background_quantile must be in (0, 1), got {background_quantile}"
    if not 0 < probability_cutoff < 1:
        return f"probability_cutoff must be in (0, 1), got {probability_cutoff}"
    if plot and output_dir is None:
        return "output_dir is required when plot=True. Provide a directory path or set plot=False."
    return None


def sample_indices(n_valid: int, size: int, seed: int) -> np.ndarray:
    """The reference's ``np.random.seed(seed); np.random.choice(n_valid, size, replace=False)`` (CL:750-756) from a
    private RandomState: the same indices, numpy's global generator untouched."""
    return np.random.RandomState(seed).choice(n_valid, size=size, replace=False)


class _OrderStatistics:
    """numpy's ``np.percentile(sorted, q)`` (method "linear") from the two order statistics it interpolates, with the
    types numpy itself computes in: a scalar q on float32 data stays float32, a list of q gives float64."""

    def __init__(self, n: int, dtype):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.requests = {}

    def plan(self, name, q):
        quantiles = np.asanyarray(np.true_divide(q, self.dtype.type(100)))
        virtual = np.asanyarray((self.n - 1) * quantiles)
        prev = np.floor(virtual).astype(np.intp)
        nxt = prev + 1
        above = virtual >= self.n - 1
        prev = np.where(above, self.n - 1, np.maximum(prev, 0))
        nxt = np.where(above, self.n - 1, np.maximum(nxt, 0))
        gamma = np.asanyarray(virtual - np.floor(virtual).astype(np.intp), dtype=virtual.dtype)
        self.requests[name] = (prev, nxt, gamma)

    def ranks(self) -> np.ndarray:
        out = [0, self.n - 1]
        for prev, nxt, _ in self.requests.values():
            out += list(np.atleast_1d(prev)) + list(np.atleast_1d(nxt))
        return np.array(out, dtype=np.int64)

    def load(self, values: np.ndarray):
        """values: the order statistics at ranks(), fp64 (each exactly a score)."""
        self.first, self.last = (self.dtype.type(v) for v in values[:2])
        at = 2
        self.bounds = {}
        for name, (prev, _, _) in self.requests.items():
            k = np.atleast_1d(prev).size
            lo = values[at:at + k].astype(self.dtype).reshape(np.shape(prev))
            hi = values[at + k:at + 2 * k].astype(self.dtype).reshape(np.shape(prev))
            self.bounds[name] = (lo, hi)
            at += 2 * k

    def percentile(self, name):
        lo, hi = self.bounds[name]
        t = self.requests[name][2]
        diff = np.subtract(hi, lo)
        out = np.asanyarray(np.add(lo, diff * t))
        np.subtract(hi, diff * (1 - t), out=out, where=t >= 0.5, casting="unsafe", dtype=type(out.dtype))
        return out[()] if out.ndim == 0 else out


def _threshold_ks(ctx, scores: np.ndarray, background_quantile: float):
    """threshold_ks (TH:102-198): sort, background moments, D and its argmax, deviation scores and labels on the
    device; the zero-variance and the below-background fallbacks here, on order statistics."""
    order = _OrderStatistics(scores.size, scores.dtype)
    order.plan("iqr", [25, 75])
    order.plan("p90", 90)
    prep = ctx.ks_prepare(scores, background_quantile, ranks=order.ranks())
    order.load(prep["order"])
    bg_mean, bg_std = prep["bg_mean"], prep["bg_std"]
    if bg_std < 1e-10:
        q25, q75 = order.percentile("iqr")
        iqr = q75 - q25
        if iqr > 1e-10:
            bg_std = float(iqr / 1.35)
        else:
            bg_std = float(max((order.last - order.first) * 0.1, 1e-6))
    _, threshold, _ = ctx.ks_argmax(bg_mean, bg_std)
    if threshold <= bg_mean:
        threshold = float(order.percentile("p90"))
    deviation, labels, n_high = ctx.ks_classify(scores, threshold, float(order.last))
    params = {"background_mean": bg_mean, "background_std": bg_std, "background_quantile": background_quantile}
    return threshold, deviation, labels, n_high, params


def _weighted_log_prob(x, weights, means, variances):
    p = 1.0 / np.sqrt(variances)
    y = x[:, None] * p[None, :] - (means * p)[None, :]
    return (-0.5 * (np.log(2 * np.pi) + y * y) + np.log(p)[None, :]) + np.log(weights)[None, :]


def _gmm_cutoff(weights, means, variances, n_components: int):
    """The score threshold of TH:283-328 from the fitted parameters, the components whose responsibilities add up to
    P(high) (in the order the reference adds them), the argsort of the means and the reference's high_component_idx."""
    order = np.argsort(means)
    if n_components == 2:
        high = int(np.argmax(means))
        low = 1 - high
        grid = np.linspace(means[low], means[high], 1000)
        wl = _weighted_log_prob(grid, weights, means, variances)
        m = wl.max(axis=1)
        lse = np.log(np.exp(wl[:, 0] - m) + np.exp(wl[:, 1] - m)) + m
        diff = np.exp(wl[:, high] - lse) - 0.5
        cross = np.where(np.diff(np.sign(diff)))[0]
        threshold = float(grid[cross[0]]) if len(cross) > 0 else float((means[low] + means[high]) / 2)
        return threshold, [high], order, high
    threshold = float((means[order[0]] + means[order[1]]) / 2)
    return threshold, [int(k) for k in order[1:]], order, int(order[1])


def _threshold_gmm(ctx, fit_scores: np.ndarray, all_scores: np.ndarray, probability_cutoff: float, n_components: int,
                   seed: int):
    """threshold_gmm (TH:201-344) and the re-scoring of every cell after a fit on a sample (CL:780-795)."""
    X = fit_scores.reshape(-1, 1)
    km_tol = float(np.mean(np.var(X, axis=0)) * 1e-4)      # sklearn's KMeans._tolerance and centring, on the input
    x_mean = X.mean(axis=0)
    draws = kmeans_draws(seed, GMM_N_INIT, n_components)
    fit = ctx.gmm_fit(fit_scores, n_components, GMM_N_INIT, KMEANS_MAX_ITER, km_tol, x_mean, draws, GMM_MAX_ITER,
                      GMM_TOL, GMM_REG_COVAR)
    best = fit["best"]
    weights, means, variances = fit["weights"][best], fit["means"][best], fit["variances"][best]
    threshold, high, order, high_idx = _gmm_cutoff(weights, means, variances, n_components)
    prob, labels, n_high = ctx.gmm_posterior(all_scores, weights, means, variances, high, probability_cutoff)
    params = {
        "gmm_means": means.tolist(),
        "gmm_stds": np.sqrt(variances).tolist(),
        "gmm_weights": weights.tolist(),
        "n_components": n_components,
        "sorted_component_indices": order.tolist(),
        "high_component_idx": high_idx,
        "probability_cutoff": probability_cutoff,
        "gmm_n_iter": int(fit["n_iter"][best]),
        "gmm_converged": bool(fit["converged"][best]),
        "gmm_lower_bound": float(fit["lower_bound"][best]),
    }
    return threshold, prob, labels, n_high, params


def classify_by_threshold(
    adata,
    feature_columns: List[str],
    metagene_method: str = "shifted_geometric_mean",
    threshold_method: str = "gmm",
    pseudocount: float = 0.1,
    background_quantile: float = 0.5,
    probability_cutoff: float = 0.3,
    n_components: int = 2,
    max_cells: Optional[int] = 20000,
    column_prefix: str = "threshold",
    seed: int = 42,
    plot: bool = True,
    output_dir: Optional[Union[str, Path]] = None,
    n_sample_plot: int = 20000,
    copy: bool = False,
    *,
    device: int = 0,
):
    """Classify cells as low / high by thresholding one feature or the metagene score of several (CL:419-894).

    Writes ``obs[{prefix}_score]``, ``obs[{prefix}_probability]`` (float64; NaN for cells with a NaN/Inf feature) and
    ``obs[{prefix}_cluster]`` (int64: 0 low, 1 high, -1 invalid), ``uns[{prefix}_params]`` and one provenance entry.
    ``threshold_method="ks"`` labels ``score >= threshold``; ``"gmm"`` labels ``P(high) > probability_cutoff``, and
    with ``n_components >= 3`` P(high) adds every component but the lowest.  ``max_cells=None`` (extension) fits the
    mixture on every valid cell.  No figure is drawn: ``plot=True`` needs ``output_dir`` as in the reference and
    logs one warning.
    """
    problem = _request_problem(feature_columns, metagene_method, threshold_method, pseudocount, background_quantile,
                               probability_cutoff, plot, output_dir)
    if problem:
        raise ValueError(problem)
    adata = adata.copy() if copy else adata
    logger.info(f"Classifying by threshold: {len(feature_columns)} feature(s), "
                f"metagene={metagene_method}, threshold={threshold_method}")
    logger.info(f"Features: {feature_columns}")
    features = _extract_features(adata, feature_columns)
    if features.dtype not in (np.float32, np.float64):
        features = features.astype(np.float64)
    n_cells = adata.n_obs

    ctx = _lib.default_context(device)
    mg = ctx.metagene_score(features, metagene_method, pseudocount)
    valid, n_valid = mg["valid"], mg["n_valid"]
    n_invalid = n_cells - n_valid
    if n_invalid > 0:
        logger.warning(f"{n_invalid} cells have NaN/Inf values and will be marked as cluster=-1")
    if n_valid < 100:
        raise ValueError(f"Only {n_valid} valid cells (non-NaN/Inf). "
                         "Need at least 100 cells for threshold detection.")
    logger.info(f"Valid cells: {n_valid:,} / {n_cells:,}")
    if mg["n_negative"] > 0 and metagene_method in ("shifted_geometric_mean", "geometric_mean"):
        raise ValueError(
            f"Feature values contain negative numbers, which are incompatible with "
            f"metagene_method='{metagene_method}' (log of negative values is undefined). "
            f"Use metagene_method='arithmetic_mean' or 'median' instead.\n\n"
            f"Common cases with negative values:\n"
            f"  - Local Moran's I (negative = spatial outlier)\n"
            f"  - Z-scores or scaled expression data\n"
            f"  - Differential expression log-fold changes")
    scores = mg["score"][valid]
    logger.info(f"Metagene scores: min={mg['min']:.4f}, max={mg['max']:.4f}, mean={mg['mean']:.4f}")

    pct_all_zero = 100 * mg["n_below"] / n_valid
    if pct_all_zero >= 50.0 and threshold_method == "gmm":
        warnings.warn(
            f"{pct_all_zero:.1f}% of cells have zero expression for all markers. "
            f"GMM will likely separate zeros from non-zeros rather than finding "
            f"a meaningful biological threshold. Consider using threshold_method='ks' "
            f"which is designed for sparse marker detection.",
            UserWarning,
            stacklevel=2,
        )

    if threshold_method == "ks":
        threshold, probability, labels, n_high, method_params = _threshold_ks(ctx, scores, background_quantile)
    else:
        sample_size = n_valid if max_cells is None else min(n_valid, max_cells)
        if sample_size < n_valid:
            fit_scores = scores[sample_indices(n_valid, sample_size, seed)]
            logger.debug(f"Downsampled to {sample_size:,} cells for GMM fitting")
        else:
            fit_scores = scores
        threshold, probability, labels, n_high, method_params = _threshold_gmm(
            ctx, fit_scores, scores, probability_cutoff, n_components, seed)
    logger.info(f"Threshold: {threshold:.4f}")

    score_col, prob_col, cluster_col = (f"{column_prefix}_{s}" for s in ("score", "probability", "cluster"))
    score_all = np.full(n_cells, np.nan, dtype=np.float64)
    prob_all = np.full(n_cells, np.nan, dtype=np.float64)
    cluster_all = np.full(n_cells, -1, dtype=np.int64)
    score_all[valid] = scores
    prob_all[valid] = probability
    cluster_all[valid] = labels
    adata.obs[score_col] = score_all
    adata.obs[prob_col] = prob_all
    adata.obs[cluster_col] = cluster_all

    n_high = int(n_high)
    n_low = n_valid - n_high
    logger.info(f"Cluster 0 (low): {n_low:,} cells ({100 * n_low / n_valid:.1f}%)")
    logger.info(f"Cluster 1 (high): {n_high:,} cells ({100 * n_high / n_valid:.1f}%)")

    uns_key = f"{column_prefix}_params"
    adata.uns[uns_key] = {
        "feature_columns": feature_columns,
        "metagene_method": metagene_method,
        "threshold_method": threshold_method,
        "threshold": threshold,
        "pseudocount": pseudocount,
        "n_high": n_high,
        "n_low": n_low,
        "n_invalid": n_invalid,
        "n_total": n_cells,
        "seed": seed,
        **method_params,
    }
    update_metadata(
        adata,
        function_name="classify_by_threshold",
        parameters={
            "feature_columns": feature_columns,
            "metagene_method": metagene_method,
            "threshold_method": threshold_method,
            "pseudocount": pseudocount,
            "background_quantile": background_quantile,
            "probability_cutoff": probability_cutoff,
            "column_prefix": column_prefix,
        },
        outputs={
            "obs_score": score_col,
            "obs_probability": prob_col,
            "obs_cluster": cluster_col,
            "uns_params": uns_key,
            "threshold": threshold,
            "n_high": n_high,
            "n_low": n_low,
        },
    )
    if plot:
        logger.warning(f"plot=True: this package draws no figure; "
                       f"{Path(output_dir) / f'{column_prefix}_gpairs.png'} is not written")
    return adata
