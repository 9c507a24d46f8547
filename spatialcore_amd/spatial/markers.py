"""Marker genes per group on MI355X: the Wilcoxon rank-sum test of scanpy's ``rank_genes_groups``.

EXTENSION -- not part of the reference's ``spatial`` surface.  The reference's domain vignette
(docs/domains/domain_detection.md, step 3) ends with ``sc.tl.rank_genes_groups(adata, groupby=..., method="wilcoxon")``;
this module answers that call without leaving the device.  The name, the keywords and the layout of
``adata.uns[key_added]`` are scanpy's as recalled from upstream (scanpy is not installed where this was written:
DESIGN.md 4.6f says what is therefore unpinned).  What IS pinned is the arithmetic, against scipy:

* ``sc_ranksum`` (include/spatialcore_hip.h, N8) returns, per gene and group, twice the sum of the average ranks as an
  exact integer -- ``scipy.stats.rankdata`` over the ranked cells -- plus the tie sums, non-zero counts and value sums;
* ``wilcoxon_tables`` turns those tables into scores, p-values, adjusted p-values and fold changes: pure host
  arithmetic, testable without a device, cross-checked against ``scipy.stats.mannwhitneyu``.
"""

from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import pandas as pd
from scipy import sparse, stats

from spatialcore_amd import _lib
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata

logger = get_logger("spatial.markers")

CORRECTION_METHODS = ("benjamini-hochberg", "bonferroni")


def _adjust(pvals: np.ndarray, corr_method: str) -> np.ndarray:
    """Benjamini-Hochberg (step-up, as statsmodels' ``fdr_bh``) or Bonferroni over all the given p-values, clipped at 1."""
    m = pvals.size
    if corr_method == "bonferroni":
        return np.minimum(pvals * m, 1.0)
    order = np.argsort(pvals, kind="stable")
    stepped = pvals[order] * m / np.arange(1, m + 1)
    stepped = np.minimum.accumulate(stepped[::-1])[::-1]
    out = np.empty(m, dtype=np.float64)
    out[order] = np.minimum(stepped, 1.0)
    return out


def wilcoxon_tables(rank2, tie_nonzero, nnz, sums, n_neg, group_n, *, report: Optional[Sequence[int]] = None,
                    tie_correct: bool = False, corr_method: str = "benjamini-hochberg", rankby_abs: bool = False,
                    n_genes: Optional[int] = None, log1p_base: Optional[float] = None) -> dict:
    """Scores, p-values and fold changes from the integer tables of ``sc_ranksum`` (pure host arithmetic, no device).

    ``rank2``: (G, K) int, twice the rank sums; ``tie_nonzero``: (G,) Python ints, sum of t^3 - t over the tie runs of
    non-zero values; ``nnz``: (G, K) non-zero counts; ``sums``: (G, K) value sums; ``n_neg``: (G,) negative counts (the
    ranks already account for them; kept for the record); ``group_n``: (K,) ranked cells per code.  Every code takes
    part in the ranking; ``report`` lists the codes that get a table (default: all), each against ALL the other ranked
    cells.  For code k with n1 cells against m = N - n1 others:

    * ``score = (R - n1 (N + 1) / 2) / sd``, ``sd = sqrt(c n1 m (N + 1) / 12)``, c = 1 or, with ``tie_correct``,
      ``1 - T / (N^3 - N)`` where T = ``tie_nonzero`` + n_zero^3 - n_zero (exact integers); NaN scores (sd = 0) become 0;
    * ``pvals = 2 * norm.sf(|score|)`` (NaN becomes 1); ``pvals_adj`` over all G genes (``corr_method``), clipped at 1;
    * ``logfoldchanges = log2((expm1(mean_k) + 1e-9) / (expm1(mean_other) + 1e-9))``, the means scaled by
      ``ln(log1p_base)`` first when a base is given;
    * ``pts`` / ``pts_rest``: the non-zero fractions of the group and of the others.

    Returns ``order`` (R, n_out) gene positions by descending score (|score| with ``rankby_abs``; equal scores by
    ascending position), truncated to ``n_genes`` AFTER the adjustment, and ``scores`` (float32), ``logfoldchanges``
    (float32), ``pvals``, ``pvals_adj`` (float64) in that order; ``pts`` and ``pts_rest`` are (R, G) in gene order.
    """
    if corr_method not in CORRECTION_METHODS:
        raise ValueError(f"corr_method must be one of {list(CORRECTION_METHODS)}, got '{corr_method}'")
    rank2 = np.asarray(rank2, dtype=np.int64)
    nnz = np.asarray(nnz, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    group_n = np.asarray(group_n, dtype=np.int64)
    G, K = rank2.shape
    report = list(range(K)) if report is None else [int(k) for k in report]
    n_out = G if n_genes is None else min(int(n_genes), G)
    N = int(group_n.sum())
    n_nonzero = nnz.sum(axis=1)
    c = np.ones(G, dtype=np.float64)
    if tie_correct:
        D = N ** 3 - N
        for g in range(G):
            nz = N - int(n_nonzero[g])
            T = int(tie_nonzero[g]) + nz ** 3 - nz
            c[g] = 1.0 - T / D if D > 0 else 0.0
    scale = 1.0 if log1p_base is None else float(np.log(log1p_base))

    out = {k: [] for k in ("order", "scores", "logfoldchanges", "pvals", "pvals_adj", "pts", "pts_rest")}
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in report:
            n1 = int(group_n[k])
            m = N - n1
            num = (rank2[:, k] - n1 * (N + 1)) / 2.0        # an exact integer or half-integer below 2^53
            sd = np.sqrt(c * (n1 * m * (N + 1) / 12.0))
            score = num / sd
            score[np.isnan(score)] = 0.0
            pvals = 2.0 * stats.norm.sf(np.abs(score))
            pvals[np.isnan(pvals)] = 1.0
            padj = _adjust(pvals, corr_method)
            other = np.delete(sums, k, axis=1).sum(axis=1)
            mean_k, mean_o = sums[:, k] / n1, other / m
            lfc = np.log2((np.expm1(mean_k * scale) + 1e-9) / (np.expm1(mean_o * scale) + 1e-9))
            key = np.abs(score) if rankby_abs else score
            order = np.argsort(-key, kind="stable")[:n_out]
            out["order"].append(order)
            out["scores"].append(score[order].astype(np.float32))
            out["logfoldchanges"].append(lfc[order].astype(np.float32))
            out["pvals"].append(pvals[order])
            out["pvals_adj"].append(padj[order])
            out["pts"].append(nnz[:, k] / n1)
            out["pts_rest"].append((n_nonzero - nnz[:, k]) / m)
    return {name: np.array(rows).reshape(len(report), -1) for name, rows in out.items()}


def _gene_batch(n_cells: int, requested: Optional[int]) -> int:
    """Genes per device batch: the fp64 tiles are 8 bytes per (cell, gene); the pair arrays have a budget of their own."""
    if requested is not None:
        if requested < 1:
            raise ValueError(f"gene_batch must be >= 1, got {requested}")
        return int(requested)
    fit = int((16 << 30) // (8 * max(n_cells, 1)))
    return max(16, fit // 16 * 16)


def _request(adata, groupby, groups, reference, genes, n_genes, corr_method, method, gene_batch):
    """Validates a ``rank_genes_groups`` request before any device work: (group names, label code per cell with -1 for
    a missing label, reported codes, reference code or None, gene names, gene columns)."""
    if method != "wilcoxon":
        raise ValueError(f"only method='wilcoxon' is supported, got '{method}'")
    if corr_method not in CORRECTION_METHODS:
        raise ValueError(f"corr_method must be one of {list(CORRECTION_METHODS)}, got '{corr_method}'")
    if groupby not in adata.obs.columns:
        raise ValueError(f"Column '{groupby}' not found in adata.obs. "
                         f"Available columns: {list(adata.obs.columns)[:10]}...")
    if n_genes is not None and n_genes < 1:
        raise ValueError(f"n_genes must be >= 1, got {n_genes}")
    _gene_batch(adata.n_obs, gene_batch)
    gene_names = list(adata.var_names) if genes is None else ([genes] if isinstance(genes, str) else list(genes))
    missing = [g for g in gene_names if g not in adata.var_names]
    if missing:
        raise ValueError(f"Genes not found in adata.var_names: {missing[:10]}")
    if len(set(gene_names)) != len(gene_names):
        raise ValueError("genes must not contain a name twice")
    if not gene_names:
        raise ValueError("genes must not be empty")
    cols = np.asarray([int(adata.var_names.get_loc(g)) for g in gene_names], dtype=np.int32)

    labels = adata.obs[groupby]
    present = ~np.asarray(labels.isna())
    as_text = np.asarray(labels.values, dtype=object)[present].astype(str)
    codes = np.full(adata.n_obs, -1, dtype=np.int32)
    if isinstance(labels.dtype, pd.CategoricalDtype):      # the categories' own order (those in use), as scanpy's fields
        used = labels.cat.remove_unused_categories()
        codes[present] = np.asarray(used.cat.codes)[present]
        names = [str(v) for v in used.cat.categories]
    else:                                                   # any other column: the labels as text, sorted
        found, names = pd.factorize(as_text, sort=True)
        codes[present] = found
        names = [str(v) for v in names]
    if isinstance(groups, str) and groups == "all":
        selected = list(range(len(names)))
    else:
        if isinstance(groups, (str, int)):
            raise ValueError(f"groups must be 'all' or a sequence of labels, got {groups!r}")
        wanted = [str(g) for g in groups]
        unknown = [g for g in wanted if g not in names]
        if unknown:
            raise ValueError(f"groups {unknown} not found in adata.obs['{groupby}'] = {names[:20]}")
        selected = sorted({names.index(g) for g in wanted})
    ref = None
    if reference != "rest":
        if str(reference) not in names:
            raise ValueError(f"reference = {reference} needs to be one of groupby = {names[:20]}.")
        ref = names.index(str(reference))
        selected = [k for k in selected if k != ref]
    if not selected:
        raise ValueError("no group is left to test")
    sizes = np.bincount(codes[codes >= 0], minlength=len(names))
    small = [names[k] for k in selected + ([ref] if ref is not None else []) if sizes[k] < 2]
    if small:
        raise ValueError(f"Could not calculate statistics for groups {', '.join(small)} "
                         "since they only contain one sample.")
    return names, codes, selected, ref, gene_names, cols


def rank_genes_groups(
    adata,
    groupby: str,
    *,
    groups: Union[str, Sequence[str]] = "all",
    reference: str = "rest",
    genes: Optional[Sequence[str]] = None,
    layer: Optional[str] = None,
    n_genes: Optional[int] = None,
    rankby_abs: bool = False,
    pts: bool = False,
    tie_correct: bool = False,
    corr_method: str = "benjamini-hochberg",
    method: str = "wilcoxon",
    key_added: str = "rank_genes_groups",
    gene_batch: Optional[int] = None,
    copy: bool = False,
    device: int = 0,
):
    """Rank genes for characterising groups: the Wilcoxon rank-sum test of scanpy's ``rank_genes_groups``.

    EXTENSION -- scanpy's function, not in the reference; the keywords are scanpy's so that the reference's domain
    vignette changes only its prefix.  Only ``method="wilcoxon"`` exists here (anything else: ``ValueError``).

    ``groupby``: column of ``adata.obs``; ``groups``: ``"all"`` or the labels to report; ``reference``: ``"rest"``
    (each group against all other cells -- unselected groups and cells with a missing label still count among them) or
    one label (every reported group against that group alone, ranks taken over the two groups only).  ``genes``:
    names to test (default all); ``layer``: matrix to read instead of ``X``; ``n_genes``: rows to keep per group
    (default all; the multiple-testing adjustment always covers every tested gene); ``rankby_abs``: order by |score|;
    ``pts``: also store the fraction of expressing cells; ``tie_correct``: tie-corrected variance; ``corr_method``:
    ``"benjamini-hochberg"`` or ``"bonferroni"``; ``gene_batch``: genes resident on the device at a time (a gene's
    result does not depend on it); ``device`` (extension): the GPU to run on.  A reported group or a reference with
    fewer than 2 cells raises ``ValueError`` and names it.

    ``adata.uns[key_added]`` holds ``params`` and the record arrays ``names`` (object), ``scores``, ``logfoldchanges``
    (float32), ``pvals``, ``pvals_adj`` (float64), one field per reported group, rows by descending score (equal
    scores by ascending gene position); with ``pts`` the DataFrames ``pts`` and ``pts_rest`` (genes x groups).  The
    statistic is exact: rank sums are integers computed on the device, identical from run to run; see
    ``wilcoxon_tables`` for the formulas.  ``logfoldchanges`` assumes log1p data, natural base unless
    ``adata.uns["log1p"]["base"]`` is set.
    """
    names, codes, selected, ref, gene_names, cols = _request(adata, groupby, groups, reference, genes, n_genes, corr_method,
                                                             method, gene_batch)
    if copy:
        adata = adata.copy()
    n_cells, G, R = adata.n_obs, len(gene_names), len(selected)
    per_batch = _gene_batch(n_cells, gene_batch)
    X = adata.layers[layer] if layer is not None else adata.X
    logger.info(f"Ranking {G} genes for {R} groups of '{groupby}' against "
                f"{'the rest' if ref is None else names[ref]}: {n_cells:,} cells, Wilcoxon rank sums on the GPU")

    # reference="rest": one ranking; the reported groups take codes 0 .. R-1 and every other cell the code R
    # reference=<group>: one ranking per reported group over (group, reference) = codes (0, 1); the other cells are left out
    if ref is None:
        relabel = np.full(len(names) + 1, R, dtype=np.int32)        # slot -1: the cells without a label
        relabel[selected] = np.arange(R, dtype=np.int32)
        rankings = [(relabel[codes], R + 1 if (relabel[codes] == R).any() else R, list(range(R)))]
    else:
        rankings = []
        for k in selected:
            relabel = np.full(len(names) + 1, -1, dtype=np.int32)
            relabel[k], relabel[ref] = 0, 1
            rankings.append((relabel[codes], 2, [0]))

    ctx = _lib.default_context(device)
    parts = [[] for _ in rankings]
    for b0 in range(0, G, per_batch):
        part = cols[b0:b0 + per_batch]
        if sparse.issparse(X):
            ctx.set_expression(X, part)
        else:
            ctx.set_expression(np.asarray(X)[:, part], np.arange(part.size, dtype=np.int32))
        for slot, (code, n_codes, _) in enumerate(rankings):
            parts[slot].append(ctx.ranksum(code, n_codes))

    base = None
    if isinstance(adata.uns.get("log1p"), dict):
        base = adata.uns["log1p"].get("base")
    table = {k: [] for k in ("order", "scores", "logfoldchanges", "pvals", "pvals_adj", "pts", "pts_rest")}
    for (code, n_codes, report), batches in zip(rankings, parts):
        merged = {k: np.concatenate([b[k] for b in batches], axis=0) for k in ("rank2", "tie_nonzero", "nnz", "sums", "n_neg")}
        t = wilcoxon_tables(merged["rank2"], merged["tie_nonzero"], merged["nnz"], merged["sums"], merged["n_neg"],
                            batches[0]["group_n"], report=report, tie_correct=tie_correct, corr_method=corr_method,
                            rankby_abs=rankby_abs, n_genes=n_genes, log1p_base=base)
        for k in table:
            table[k].extend(t[k])

    reported = [names[k] for k in selected]
    gene_arr = np.asarray(gene_names, dtype=object)
    result = {"params": {"groupby": groupby, "reference": reference, "method": method, "use_raw": False, "layer": layer,
                         "corr_method": corr_method}}
    for field, dtype, rows in (("names", object, [gene_arr[o] for o in table["order"]]), ("scores", np.float32, table["scores"]),
                               ("logfoldchanges", np.float32, table["logfoldchanges"]), ("pvals", np.float64, table["pvals"]),
                               ("pvals_adj", np.float64, table["pvals_adj"])):
        result[field] = np.rec.fromarrays([np.asarray(r, dtype=dtype) for r in rows], dtype=[(g, dtype) for g in reported])
    if pts:
        result["pts"] = pd.DataFrame(np.array(table["pts"]).T, index=gene_names, columns=reported)
        result["pts_rest"] = pd.DataFrame(np.array(table["pts_rest"]).T, index=gene_names, columns=reported)
    adata.uns[key_added] = result
    update_metadata(
        adata,
        function_name="rank_genes_groups",
        parameters={"groupby": groupby, "groups": "all" if isinstance(groups, str) else [str(g) for g in groups],
                    "reference": reference, "method": method, "layer": layer, "n_genes": n_genes, "rankby_abs": rankby_abs,
                    "pts": pts, "tie_correct": tie_correct, "corr_method": corr_method, "gene_batch": per_batch},
        outputs={"uns": key_added, "n_genes": G, "n_groups": R, "n_cells": n_cells, "groups": reported},
    )
    return adata
