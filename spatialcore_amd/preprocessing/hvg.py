"""highly_variable_genes: gene selection by the variance of analytic Pearson residuals (sc_hvg_pearson).

Lause, Berens & Kobak 2021 ("Analytic Pearson residuals for normalization of single-cell RNA-seq UMI data"), the rule
scanpy exposes as ``experimental.pp.highly_variable_genes(flavor="pearson_residuals")``, restated from the published
formula.  scanpy is not a dependency of this package and parity with it is not pinned by any test: the arithmetic is
checked against a plain numpy restatement of the formula (tests/hvg_restated.py).

What touches the cells x genes pairs runs in HIP: the row sums, the per-gene sums of x and x^2, and the two sums of the
clipped residuals over ALL pairs, zeros included, without densifying anything.  The ranking of at most 32768 variances is
done here on the host.  There is no CPU fallback for the device part."""

from __future__ import annotations

import numbers
from typing import Optional

import numpy as np

from spatialcore_amd import _lib
from spatialcore_amd._batches import batch_groups
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd._sparse_input import canonical_csr, gene_columns

logger = get_logger("hvg")

FLAVORS = ("pearson_residuals",)
_SUPPORTED = "2 <= cells <= 2^31 - 1 (per batch), 1 <= genes <= 32768, at most 2^32 - 1 stored entries"


# ---- the host part: ranking ------------------------------------------------------------------------------------------------
def rank_by_variance(residual_variances) -> np.ndarray:
    """rank[g] = the gene's position by descending residual variance, ties to the smaller gene index (0 = the most
    variable gene)."""
    v = np.asarray(residual_variances, dtype=np.float64)
    if v.ndim != 1 or not np.all(np.isfinite(v)):
        raise ValueError("residual variances must be one finite value per gene")
    order = np.argsort(-v, kind="stable")
    rank = np.empty(v.size, dtype=np.int64)
    rank[order] = np.arange(v.size)
    return rank


def select_single(residual_variances, n_top_genes: int) -> dict:
    """The ``var`` columns of one matrix: the ``n_top_genes`` genes of lowest rank (all, if there are no more)."""
    rank = rank_by_variance(residual_variances)
    hv = rank < n_top_genes
    return {"residual_variances": np.asarray(residual_variances, dtype=np.float64).copy(),
            "highly_variable_rank": np.where(hv, rank.astype(np.float64), np.nan), "highly_variable": hv}


def select_batches(residual_variances, n_top_genes: int) -> dict:
    """The ``var`` columns of B batches from their variances (B x genes): ``rank_b[g]`` the rank inside batch b,
    ``highly_variable_nbatches[g] = #{b: rank_b[g] < n_top_genes}``, ``m[g]`` the median of those ranks (NaN if none); the
    genes are ordered by m ascending with NaN last, then nbatches descending, then gene index, and the first
    ``n_top_genes`` of that order are selected, with ``highly_variable_rank = m``."""
    V = np.asarray(residual_variances, dtype=np.float64)
    if V.ndim != 2 or V.shape[0] < 1:
        raise ValueError("residual variances must be (batches, genes)")
    B, G = V.shape
    ranks = np.stack([rank_by_variance(V[b]) for b in range(B)]).astype(np.float64)
    top = ranks < n_top_genes
    nbatches = top.sum(axis=0).astype(np.int64)
    m = np.full(G, np.nan)
    some = nbatches > 0
    kept = np.where(top, ranks, np.nan)
    m[some] = np.nanmedian(kept[:, some], axis=0)
    order = np.lexsort((np.arange(G), -nbatches, np.where(some, m, np.inf)))
    hv = np.zeros(G, dtype=bool)
    hv[order[:n_top_genes]] = True
    return {"residual_variances": V.mean(axis=0), "highly_variable_rank": np.where(hv, m, np.nan), "highly_variable": hv,
            "highly_variable_nbatches": nbatches, "highly_variable_intersection": nbatches == B}


def moments_from_sums(sum_x, sum_x2, n: int):
    """``means = sum x / n`` and ``variances = (sum x^2 / n - means^2) n / (n - 1)`` (the sample variance)."""
    sum_x, sum_x2 = np.asarray(sum_x, dtype=np.float64), np.asarray(sum_x2, dtype=np.float64)
    means = sum_x / n
    return means, (sum_x2 / n - means ** 2) * (n / (n - 1))


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def _check_flag(name: str, value) -> bool:
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, got {value!r}")
    return bool(value)


def _check_positive(name: str, value, note: str = "") -> float:
    if not isinstance(value, numbers.Real) or isinstance(value, bool) or not value > 0:
        raise ValueError(f"{name} must be a number > 0{note}, got {value!r}")
    return float(value)


def _check_part(Xc, what: str) -> None:
    """What one device call needs of its rows, checked before the device is touched; warns about cells without a count."""
    n = Xc.shape[0]
    if not 2 <= n <= 2**31 - 1:
        raise ValueError(f"{what} has {n} cells; supported: {_SUPPORTED}")
    if Xc.nnz == 0:
        raise ValueError(f"{what} is all zero: there is nothing to rank")
    empty = int(np.count_nonzero(np.diff(Xc.indptr) == 0))
    if empty:
        logger.warning(f"{what}: {empty:,} cell(s) without a count; their Pearson residuals are taken as 0 and they "
                       "still count in the number of cells")


def _device_call(ctx, Xc, theta: float, clip: Optional[float]):
    """One sc_hvg_pearson on the rows of ``Xc`` with their own sums, n and default clip."""
    n, G = Xc.shape
    return ctx.hvg_pearson(Xc.indptr, Xc.indices, Xc.data, G, theta, float(np.sqrt(n)) if clip is None else clip)


# ---- the public function -------------------------------------------------------------------------------------------------------
def highly_variable_genes(adata, *, n_top_genes: int = 2000, flavor: str = "pearson_residuals", theta: float = 100.0,
                          clip: Optional[float] = None, layer: Optional[str] = None, batch_key: Optional[str] = None,
                          subset: bool = False, copy: bool = False, device: int = 0):
    """Marks the ``n_top_genes`` genes whose analytic Pearson residuals vary most (Lause, Berens & Kobak 2021), on the GPU.

    ``adata.X`` (or ``layers[layer]``) holds raw counts: scipy sparse of any format or dense, finite and non-negative;
    values that are not integers are legal and draw one warning.  Every gene is ranked.  With ``s_i`` the sum of cell i,
    ``t_g`` the sum of gene g and ``T`` their total, ``mu = s_i t_g / T`` and the residual of a pair is
    ``(x - mu) / sqrt(mu + mu^2 / theta)`` clipped to ``[-clip, clip]``; ``theta=inf`` is the Poisson model and ``clip``
    defaults to ``sqrt(cells)``.  ``residual_variances`` is the population variance of a gene's residuals over all cells.
    A gene without a count gets 0 and ranks last.  One departure from the textbook, on purpose: a cell without a count
    gives 0 / 0 there and turns every gene into NaN; here its residuals are 0, it still counts as a cell, and a warning says
    how many there are.

    Only ``flavor="pearson_residuals"`` exists.  The rule restates the published one; scanpy is not installed where this
    package is tested, so parity with ``scanpy.experimental.pp.highly_variable_genes`` is not pinned.

    Writes ``var["means"]``, ``var["variances"]`` (sample variance of the counts, from the device's exact sums),
    ``var["residual_variances"]``, ``var["highly_variable_rank"]`` (float; 0 = most variable; NaN for genes not selected)
    and ``var["highly_variable"]``; ties go to the smaller gene index; ``n_top_genes`` >= genes selects every gene.
    ``uns["hvg"] = {"flavor", "computed_on", "params"}`` and the usual ``uns["spatialcore_metadata"]`` entry.

    ``batch_key``: a column of ``obs``; its categories are taken in sorted order and each needs at least 2 cells.  Every
    batch is ranked on its own rows with its own sums, cell count and default clip.  ``highly_variable_nbatches`` counts the
    batches in which a gene's rank is below ``n_top_genes``, ``highly_variable_intersection`` marks the genes for which
    that is every batch, ``residual_variances`` is the mean over the batches, and the genes are ordered by the median of
    their ranks below ``n_top_genes`` (genes without one last), then by the number of batches descending, then by index;
    the first ``n_top_genes`` are selected and ``highly_variable_rank`` is that median.  ``means`` and ``variances`` are
    taken over all cells.

    Returns ``adata`` (the copy with ``copy=True``); with ``subset=True`` a new object cut to the selected genes.  The
    result is a function of the arguments alone, bit for bit.  Limits: 2 <= cells <= 2^31 - 1, 1 <= genes <= 32768."""
    if flavor not in FLAVORS:
        raise ValueError(f"flavor={flavor!r} is not supported; the only flavor is 'pearson_residuals'")
    if not isinstance(n_top_genes, numbers.Integral) or isinstance(n_top_genes, bool) or n_top_genes < 1:
        raise ValueError(f"n_top_genes must be an integer >= 1, got {n_top_genes!r}")
    n_top = int(n_top_genes)
    theta = _check_positive("theta", theta, " (inf: the Poisson model)")
    clip = None if clip is None else _check_positive("clip", clip)
    subset, copy = _check_flag("subset", subset), _check_flag("copy", copy)
    if layer is not None and layer not in adata.layers:
        raise ValueError(f"layer={layer!r} is not in adata.layers")
    names, cols = gene_columns(adata, None)
    X = adata.layers[layer] if layer is not None else adata.X
    n_all = int(X.shape[0])
    if not 2 <= n_all <= 2**31 - 1:
        raise ValueError(f"highly_variable_genes needs 2 <= cells <= 2^31 - 1, got {n_all}; supported: {_SUPPORTED}")
    groups = None if batch_key is None else batch_groups(adata, batch_key)
    Xc, _ = canonical_csr(X, cols, len(adata.var_names), real=True,
                          negative="Pearson residuals need raw counts; the expression matrix has negative entries",
                          all_zero="the expression matrix is all zero: there is nothing to rank")
    if Xc.nnz > 2**32 - 1:
        raise ValueError(f"at most 2^32 - 1 stored entries are supported; supported: {_SUPPORTED}")
    if np.any(Xc.data != np.rint(Xc.data)):
        logger.warning("the expression matrix holds values that are not integers; Pearson residuals are defined on raw counts")
    n, G = Xc.shape
    logger.info(f"Pearson-residual gene selection: {n:,} cells x {G:,} genes, theta={theta:g}, "
                + ("clip=sqrt(cells)" if clip is None else f"clip={clip:g}")
                + (f", {len(groups)} batches of {batch_key!r}" if groups else ""))
    parts = [("the expression matrix", Xc)] if groups is None else [(f"batch {cat!r}", Xc[rows]) for cat, rows in groups]
    for what, Xb in parts:
        _check_part(Xb, what)
    ctx = _lib.default_context(device)
    sum_x, sum_x2, per_batch = np.zeros(G), np.zeros(G), []
    for _, Xb in parts:
        bx, bx2, _, bvar = _device_call(ctx, Xb, theta, clip)
        sum_x, sum_x2 = sum_x + bx, sum_x2 + bx2      # exact on integer counts below 2^53
        per_batch.append(bvar.copy())
    cols_out = select_single(per_batch[0], n_top) if groups is None else select_batches(np.stack(per_batch), n_top)
    means, variances = moments_from_sums(sum_x, sum_x2, n)
    adata = adata.copy() if copy else adata
    adata.var["means"] = means
    adata.var["variances"] = variances
    for key, value in cols_out.items():
        adata.var[key] = value
    params = {"n_top_genes": n_top, "theta": theta, "clip": clip, "batch_key": batch_key}
    adata.uns["hvg"] = {"flavor": flavor, "computed_on": layer if layer is not None else "adata.X", "params": params}
    update_metadata(adata, "highly_variable_genes",
                    {**params, "flavor": flavor, "layer": layer, "subset": subset, "n_genes": G,
                     "n_selected": int(cols_out["highly_variable"].sum())},
                    {"var": ["means", "variances"] + list(cols_out), "uns": "hvg"})
    if subset:
        adata = adata[:, [g for g, keep in zip(names, cols_out["highly_variable"]) if keep]].copy()
    return adata
