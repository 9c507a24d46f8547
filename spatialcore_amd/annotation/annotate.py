"""annotate_celltypist: CellTypist-style prediction on the device (sc_annot_predict).

The sparse product against the model's table, the argmax, the probability of the winning class and the four confidence
transforms run in one HIP launch per batch; the host resolves genes and models, votes by cluster from integer codes and
writes the reference's ``obs`` / ``obsm`` / ``uns`` keys.  There is no CPU fallback and no model download."""

from __future__ import annotations

import numbers
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd

from spatialcore_amd import _lib
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd.annotation import _input
from spatialcore_amd.annotation.confidence import check_method
from spatialcore_amd.annotation.model import CellTypeModel

logger = get_logger("annotation")

ModelLike = Union[CellTypeModel, str, os.PathLike]


def _load_models(custom_model_path, model) -> List[Tuple[str, CellTypeModel]]:
    if custom_model_path is not None and model is not None:
        raise ValueError("give either custom_model_path or model, not both")
    source = model if model is not None else custom_model_path
    if source is None:
        raise ValueError(
            "annotate_celltypist needs a model: this package downloads nothing and has no tissue presets.  Pass "
            "custom_model_path='model.npz' (written by train_celltypist_model or CellTypeModel.write) or "
            "model=<CellTypeModel, path, or list of these>.")
    items = list(source) if isinstance(source, (list, tuple)) else [source]
    if not items:
        raise ValueError("model must name at least one model")
    out = []
    for k, m in enumerate(items):
        if isinstance(m, CellTypeModel):
            out.append((f"model_{k}", m))
        elif isinstance(m, (str, os.PathLike)):
            out.append((os.fspath(m), CellTypeModel.load(m)))
        else:
            raise ValueError(f"a model is a CellTypeModel or a path to one, got {type(m).__name__}")
    return out


def majority_vote(codes: np.ndarray, clusters: np.ndarray, n_labels: int, min_prop: float) -> np.ndarray:
    """Per cluster the most frequent code (ties: the smallest code); -1 where its share is below ``min_prop``."""
    _, cl = np.unique(clusters, return_inverse=True)
    table = np.zeros((int(cl.max()) + 1, n_labels), dtype=np.int64)
    np.add.at(table, (cl, codes), 1)
    winner = table.argmax(axis=1)
    share = table[np.arange(table.shape[0]), winner] / table.sum(axis=1)
    winner = np.where(share < min_prop, -1, winner)
    return winner[cl]


def ensemble(confidences: Sequence[np.ndarray]) -> np.ndarray:
    """Index of the model with the highest raw confidence per cell; the first model wins ties."""
    return np.argmax(np.stack(confidences, axis=0), axis=0)


def annotate_celltypist(adata, tissue: str = "unknown", ensemble_mode: bool = True,
                        custom_model_path: Optional[Union[str, os.PathLike]] = None, majority_voting: bool = False,
                        over_clustering: Optional[str] = None, min_prop: float = 0.0, min_gene_overlap_pct: float = 25.0,
                        min_confidence: float = 0.5, store_decision_scores: bool = True,
                        confidence_transform: Optional[str] = "zscore", batch_size: Optional[int] = None,
                        copy: bool = False, *, model: Union[None, ModelLike, Sequence[ModelLike]] = None,
                        device: int = 0):
    """Annotate cells with one CellTypist-style model or an ensemble of them.

    ``adata.X`` holds counts or log1p(10k) expression.  The data's genes that any model knows are the genes in use:
    counts are normalised over them, log1p data whose gene set shrinks is renormalised (expm1, normalise, log1p).  A model
    gene the data lacks contributes nothing.  Models below ``min_gene_overlap_pct`` are skipped.  With several models the
    highest raw confidence wins per cell (the first model on ties), decision scores are not stored and the raw confidence
    stands in for the transformed one.  ``tissue`` and ``ensemble_mode`` select downloadable presets in the reference and
    are only recorded here.

    Writes ``obs["cell_type"]`` (categorical; ``"Unassigned"`` below ``min_confidence``), ``obs["cell_type_confidence"]``,
    ``obs["cell_type_confidence_raw"]``, ``obs["cell_type_model"]``, ``obs["cell_type_predicted"]`` and, for one model with
    ``store_decision_scores``, ``obsm["cell_type_decision_scores"]`` (float32) and ``uns["cell_type_cell_types"]``.
    ``batch_size`` bounds the cells per device call and never changes a bit of the result."""
    if batch_size is not None:
        if isinstance(batch_size, bool) or not isinstance(batch_size, numbers.Integral) or batch_size <= 0:
            raise ValueError("batch_size must be a positive integer or None.")
        if majority_voting:
            raise ValueError("batch_size requires majority_voting=False because voting cannot be computed across batches.")
    if confidence_transform is not None:
        check_method(confidence_transform)
    for name, v in (("min_prop", min_prop), ("min_confidence", min_confidence), ("min_gene_overlap_pct", min_gene_overlap_pct)):
        if not isinstance(v, numbers.Real) or isinstance(v, bool) or not np.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    models = _load_models(custom_model_path, model)
    data_genes = set(adata.var_names)
    kept, used = [], set()
    for name, m in models:
        overlap = set(m.features.tolist()) & data_genes
        pct = 100 * len(overlap) / m.features.size
        if pct < min_gene_overlap_pct:
            logger.warning(f"Skipping {name}: only {pct:.1f}% gene overlap")
            continue
        logger.info(f"  {name}: {pct:.1f}% overlap ({len(overlap)}/{m.features.size} genes)")
        kept.append((name, m))
        used |= overlap
    if not kept:
        raise ValueError("No models passed gene overlap threshold. Consider training a custom model for your panel genes.")
    cluster_col = over_clustering or ("leiden" if "leiden" in adata.obs.columns else None)
    if majority_voting and (cluster_col is None or cluster_col not in adata.obs.columns):
        raise ValueError("majority_voting=True requires a valid cluster column. Provide over_clustering or add a cluster "
                         f"column (e.g., 'leiden') to adata.obs. Available columns: {list(adata.obs.columns)}")
    var_names = [str(g) for g in adata.var_names]
    cols = np.asarray([j for j, g in enumerate(var_names) if g in used], dtype=np.intp)
    Xc, mode = _input.prepare(adata.X, cols)
    n, G = Xc.shape
    genes = [var_names[j] for j in cols]
    logger.info(f"Predicting on {n:,} cells x {G:,} genes ({mode})")

    ctx = _lib.default_context(device)
    step = n if batch_size is None else int(batch_size)
    single = len(kept) == 1
    want_scores = single and store_decision_scores
    per_model = []
    for name, m in kept:
        # the model on the genes in use, in the data's order; a gene this model lacks gets weight 0 (and mean 0, scale 1)
        where = {g: k for k, g in enumerate(m.features.tolist())}
        src = np.asarray([where.get(g, -1) for g in genes], dtype=np.intp)
        has = src >= 0
        coef = np.zeros((m.cell_types.size, G))
        coef[:, has] = m.coef[:, src[has]]
        mean, scale = np.zeros(G), np.ones(G)
        mean[has], scale[has] = m.scaler_mean[src[has]], m.scaler_scale[src[has]]
        parts = []
        for a in range(0, n, step):
            b = min(a + step, n)
            p0, p1 = Xc.indptr[a], Xc.indptr[b]
            parts.append(ctx.annot_predict(Xc.indptr[a:b + 1] - p0, Xc.indices[p0:p1], Xc.data[p0:p1], mode, coef,
                                           m.intercept, mean, scale, scores=want_scores))
        res = {k: (np.concatenate([p[k] for p in parts]) if parts[0][k] is not None else None) for k in parts[0]}
        labels = m.cell_types[res["labels"]]
        if majority_voting:
            voted = majority_vote(res["labels"], adata.obs[cluster_col].to_numpy(), m.cell_types.size, float(min_prop))
            labels = np.where(voted < 0, "Heterogeneous", m.cell_types[np.maximum(voted, 0)])
        per_model.append((name, m, labels, res))

    if single:
        name, m, predicted, res = per_model[0]
        conf_raw = res["confidence_raw"]
        source = np.full(n, name, dtype=object)
    else:
        pick = ensemble([r["confidence_raw"] for _, _, _, r in per_model])
        rows = np.arange(n)
        predicted = np.stack([np.asarray(lab, dtype=object) for _, _, lab, _ in per_model])[pick, rows]
        conf_raw = np.stack([r["confidence_raw"] for _, _, _, r in per_model])[pick, rows]
        source = np.asarray([nm for nm, _, _, _ in per_model], dtype=object)[pick]

    adata = adata.copy() if copy else adata
    adata.obs["cell_type_predicted"] = np.asarray(predicted, dtype=object)
    adata.obs["cell_type_confidence_raw"] = conf_raw
    adata.obs["cell_type_model"] = source
    final = np.array(predicted, dtype=object)
    if min_confidence > 0.0:
        low = conf_raw < min_confidence
        if low.any():
            final[low] = "Unassigned"
            logger.info(f"Confidence filter: {int(low.sum()):,} cells ({100 * low.mean():.1f}%) below {min_confidence} "
                        "threshold -> 'Unassigned'")
    adata.obs["cell_type"] = pd.Categorical(final)
    outputs = {"obs": ["cell_type", "cell_type_confidence", "cell_type_confidence_raw", "cell_type_model", "cell_type_predicted"]}
    if single and store_decision_scores:
        adata.obsm["cell_type_decision_scores"] = res["scores"]
        adata.uns["cell_type_cell_types"] = [str(c) for c in m.cell_types]
        outputs.update(obsm="cell_type_decision_scores", uns="cell_type_cell_types")
    elif store_decision_scores:
        logger.warning("store_decision_scores=True requested, but decision scores are not stored in ensemble mode "
                       "(multiple models).")
    if confidence_transform is not None and single and store_decision_scores:   # the reference transforms what obsm holds
        adata.obs["cell_type_confidence"] = res[confidence_transform]
    else:
        if confidence_transform is not None:
            logger.warning("Confidence transform requested, but decision scores are missing. Using raw confidence values "
                           "instead.")
        adata.obs["cell_type_confidence"] = conf_raw
    update_metadata(adata, "annotate_celltypist",
                    {"tissue": tissue, "ensemble_mode": ensemble_mode, "models": [nm for nm, _ in kept],
                     "majority_voting": majority_voting, "over_clustering": cluster_col if majority_voting else None,
                     "min_prop": min_prop, "min_gene_overlap_pct": min_gene_overlap_pct, "min_confidence": min_confidence,
                     "store_decision_scores": store_decision_scores, "confidence_transform": confidence_transform,
                     "batch_size": batch_size, "n_genes_used": G, "input_state": mode},
                    outputs)
    logger.info(f"Annotation complete: {adata.obs['cell_type'].nunique()} cell types, mean confidence: "
                f"{float(np.mean(conf_raw)):.3f}")
    return adata
