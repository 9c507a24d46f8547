"""train_celltypist_model: the full-batch one-vs-rest L2 logistic regression behind a CellTypist model, on the device
(sc_annot_train_*).

Every pass over the cells -- normalisation, scaler statistics, the forward product, the residuals, the gradient, the line
search's derivatives -- runs in HIP, in fp64 and in one documented summation order.  The host keeps the T x (G + 1)
coefficients and runs the L-BFGS two-loop recursion on them in numpy.  There is no CPU fallback."""

from __future__ import annotations

import json
import numbers
import os
from typing import Any, Dict, Optional, Sequence, Union

import numpy as np

from spatialcore_amd import _lib
from spatialcore_amd._logging import get_logger
from spatialcore_amd.annotation import _input
from spatialcore_amd.annotation.model import G_MAX, T_MAX, CellTypeModel

logger = get_logger("annotation")

LBFGS_MEMORY = 10
LINE_EVALUATIONS = 25     # safeguarded Newton steps on one step length, at the most
LINE_TOL = 1e-3           # ... which stop at |phi'(alpha)| <= LINE_TOL |phi'(0)|


def _direction(g, S, Y, rho):
    """-H g by the two-loop recursion, every class (row) on its own; pairs with rho = 0 take no part."""
    q = g.copy()
    a = []
    for s, y, r in zip(reversed(S), reversed(Y), reversed(rho)):
        ak = r * np.einsum("tg,tg->t", s, q)
        q -= ak[:, None] * y
        a.append(ak)
    if S:
        yy = np.einsum("tg,tg->t", Y[-1], Y[-1])
        gamma = np.where(rho[-1] > 0, 1.0 / np.where(rho[-1] > 0, rho[-1] * yy, 1.0), 1.0)
        q *= gamma[:, None]
    for s, y, r, ak in zip(S, Y, rho, reversed(a)):
        b = r * np.einsum("tg,tg->t", y, q)
        q += s * (ak - b)[:, None]
    return -q


def _line_search(be, W, P, C, active):
    """Per class the minimiser of phi(alpha) = F(w + alpha p) by a safeguarded Newton iteration on alpha: phi is strictly
    convex, its derivatives are one pass over the n x T scores each."""
    T = W.shape[0]
    pen1 = np.einsum("tg,tg->t", W[:, :-1], P[:, :-1]) / C
    pen2 = np.einsum("tg,tg->t", P[:, :-1], P[:, :-1]) / C
    alpha, lo, hi = np.zeros(T), np.zeros(T), np.full(T, np.inf)
    done = ~active
    d10 = None
    for _ in range(LINE_EVALUATIONS):
        d1, d2 = be.annot_train_line(alpha)
        d1 = d1 + (pen1 + alpha * pen2)
        d2 = d2 + pen2
        if d10 is None:
            d10 = np.abs(d1)
        done = done | (np.abs(d1) <= LINE_TOL * d10)
        if done.all():
            break
        neg = d1 < 0
        lo = np.where(~done & neg, alpha, lo)
        hi = np.where(~done & ~neg, alpha, hi)
        with np.errstate(divide="ignore", invalid="ignore"):
            newton = alpha - d1 / d2
            mid = np.where(np.isfinite(hi), 0.5 * (lo + hi), 2.0 * alpha + 1.0)
        new = np.where(np.isfinite(newton) & (newton > lo) & (newton < hi), newton, mid)
        new = np.where(done, alpha, new)
        done = done | (np.abs(new - alpha) <= 1e-15 * np.abs(new))
        alpha = new
    return np.where(active, alpha, 0.0)


def fit(be, T: int, G: int, sum_s: float, C: float, tol: float, max_iter: int) -> Dict[str, Any]:
    """Minimise all T objectives in lockstep on the problem resident in ``be`` (a ``_lib.Context`` after
    ``annot_train_begin``, or the numpy restatement with the same methods).  Returns coefficients (T, G + 1, intercept
    last), per class ``n_iter``, ``converged`` and ``grad_norm`` = max|grad F_t| / sum_s, the last recomputed from the
    returned coefficients."""
    W = np.zeros((T, G + 1))

    def gradient():
        g, _ = be.annot_train_grad()
        g[:, :-1] += W[:, :-1] / C
        return g

    be.annot_train_forward(W[:, :-1], W[:, -1])
    g = gradient()
    fresh = True                      # the resident scores were computed from W itself, not updated step by step
    S, Y, rho = [], [], []
    n_iter = np.zeros(T, dtype=np.int64)
    it = 0
    while True:
        norm = np.abs(g).max(axis=1) / sum_s
        active = norm > tol
        if not active.any():
            if fresh:
                break
            be.annot_train_forward(W[:, :-1], W[:, -1])
            g = gradient()
            fresh = True
            continue
        if it >= max_iter:
            if not fresh:
                be.annot_train_forward(W[:, :-1], W[:, -1])
                g = gradient()
                norm = np.abs(g).max(axis=1) / sum_s
            break
        it += 1
        P = _direction(g, S, Y, rho)
        uphill = np.einsum("tg,tg->t", g, P) >= 0
        P[uphill] = -g[uphill]
        P[~active] = 0.0
        be.annot_train_forward(P[:, :-1], P[:, -1], True)
        alpha = _line_search(be, W, P, C, active)
        be.annot_train_step(alpha)
        step = alpha[:, None] * P
        W += step
        fresh = False
        g_new = gradient()
        y = g_new - g
        ys = np.einsum("tg,tg->t", step, y)
        S.append(step), Y.append(y), rho.append(np.where(ys > 0, 1.0 / np.where(ys > 0, ys, 1.0), 0.0))
        if len(S) > LBFGS_MEMORY:
            S.pop(0), Y.pop(0), rho.pop(0)
        g = g_new
        n_iter[active] = it
    return {"coef": W[:, :-1].copy(), "intercept": W[:, -1].copy(), "n_iter": n_iter, "grad_norm": norm,
            "converged": norm <= tol}


def _labels(adata, label_column: str):
    if label_column not in adata.obs.columns:
        raise ValueError(f"Label column '{label_column}' not found. Available: {list(adata.obs.columns)}")
    col = adata.obs[label_column]
    if col.isna().any():
        raise ValueError(f"Label column '{label_column}' has {int(col.isna().sum())} missing values")
    names, codes = np.unique(col.astype(str).to_numpy(), return_inverse=True)
    if names.size < 2:
        raise ValueError(f"training needs at least 2 cell types, '{label_column}' has {names.size}")
    if names.size > T_MAX:
        raise ValueError(f"at most {T_MAX} cell types are supported, '{label_column}' has {names.size}")
    return names, codes.astype(np.int32)


def train_celltypist_model(adata, label_column: str = "unified_cell_type", model_name: str = "custom_model",
                           output_path: Optional[Union[str, os.PathLike]] = None, use_SGD: bool = True,
                           mini_batch: bool = True, balance_cell_type: bool = True, feature_selection: bool = False,
                           n_jobs: int = -1, max_iter: int = 100, epochs: int = 10, batch_size: int = 1000,
                           batch_number: int = 200, *, C: float = 1.0, tol: float = 1e-4,
                           genes: Optional[Sequence[str]] = None, layer: Optional[str] = None,
                           device: int = 0) -> Dict[str, Any]:
    """Train a CellTypist-style model on ``adata`` (counts or log1p(10k) expression) with the labels of
    ``obs[label_column]``: a StandardScaler over the genes in use, a clip at 10, and for every cell type t the minimiser of
    ``sum_i s_i (softplus(w.z_i + b) - y_it (w.z_i + b)) + |w|^2 / (2 C)`` (celltypist's ``use_SGD=False`` objective).

    celltypist's SGD mini-batch path draws its batches from an unseeded generator, so ``use_SGD``, ``mini_batch``,
    ``epochs``, ``batch_size``, ``batch_number`` and ``n_jobs`` are accepted, recorded and ignored: the full-batch problem
    is always solved.  ``balance_cell_type=True`` is its deterministic counterpart, cell weights ``s_i = n / (T n_class(i))``;
    ``False`` gives weights of 1.  ``feature_selection=True`` raises ``NotImplementedError``.  The fit stops when
    ``max|grad F_t| / sum_i s_i <= tol`` for every class, or after ``max_iter`` iterations with a warning.

    Returns the reference's dict (``model_path``, ``metadata_path``, ``n_cells_trained``, ``n_genes``, ``n_cell_types``,
    ``cell_types``, ``model`` -- a ``CellTypeModel``) plus per-class ``n_iter``, ``converged`` and ``grad_norm`` and the
    recorded ``training_params``.  Genes that are zero in every cell are dropped from the model's features."""
    if feature_selection:
        raise NotImplementedError("feature_selection=True is not implemented: every gene in use becomes a feature")
    if not isinstance(max_iter, numbers.Integral) or isinstance(max_iter, bool) or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
    for name, v in (("C", C), ("tol", tol)):
        if not isinstance(v, numbers.Real) or isinstance(v, bool) or not np.isfinite(v) or v <= 0:
            raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    if output_path is not None and not os.fspath(output_path).endswith(".npz"):
        raise ValueError(f"the model is written as .npz (never as a pickle), got output_path={os.fspath(output_path)!r}")
    names, codes = _labels(adata, label_column)
    T, n = names.size, codes.size
    if genes is None:
        gene_names = list(adata.var_names)
    else:
        gene_names = [str(g) for g in ([genes] if isinstance(genes, str) else genes)]
        missing = set(gene_names) - set(adata.var_names)
        if missing:
            raise ValueError(f"Genes not found in adata.var_names: {sorted(missing)[:10]}")
        if len(set(gene_names)) != len(gene_names):
            raise ValueError("genes must not repeat a gene")
    wanted = set(gene_names)
    cols = np.asarray([j for j, g in enumerate(adata.var_names) if g in wanted], dtype=np.intp)
    if cols.size == 0:
        raise ValueError("genes must name at least one gene")
    Xc, mode = _input.prepare(adata.layers[layer] if layer is not None else adata.X, cols)
    if Xc.shape[0] != n:
        raise ValueError("the expression matrix and obs disagree on the number of cells")
    expressed = np.flatnonzero(np.bincount(Xc.indices, minlength=cols.size) > 0)
    if expressed.size == 0:
        raise ValueError("the expression matrix is all zero: there is nothing to train on")
    if expressed.size > G_MAX:
        raise ValueError(f"at most {G_MAX} genes are supported, got {expressed.size}")
    if expressed.size != cols.size:
        Xc = Xc[:, expressed]
        Xc.sort_indices()
    features = [str(adata.var_names[j]) for j in cols[expressed]]
    G = len(features)
    counts = np.bincount(codes, minlength=T)
    weights = (n / (T * counts[codes])).astype(np.float64) if balance_cell_type else np.ones(n)
    sum_s = float(np.sum(weights))
    logger.info("use_SGD, mini_batch, epochs, batch_size, batch_number and n_jobs are recorded and ignored: the "
                "full-batch problem (celltypist's use_SGD=False objective) is solved on the device")
    logger.info(f"Training CellTypist model: {n:,} cells x {G:,} genes, {T} cell types, balance_cell_type={balance_cell_type}")

    ctx = _lib.default_context(device)
    mean, scale = ctx.annot_train_begin(Xc.indptr, Xc.indices, Xc.data, G, mode, T, codes, weights)
    try:
        res = fit(ctx, T, G, sum_s, float(C), float(tol), int(max_iter))
    finally:
        ctx.annot_train_end()
    if not res["converged"].all():
        logger.warning(f"Maximum number of iterations {max_iter} reached with {int((~res['converged']).sum())} of {T} "
                       f"classes above tol={tol} (largest scaled gradient {res['grad_norm'].max():.3g}). Increase it to "
                       "improve convergence.")
    model = CellTypeModel(features, names, res["coef"], res["intercept"], mean, scale)
    params = {"use_SGD": use_SGD, "mini_batch": mini_batch, "balance_cell_type": balance_cell_type,
              "feature_selection": feature_selection, "n_jobs": n_jobs, "max_iter": int(max_iter), "epochs": epochs,
              "batch_size": batch_size, "batch_number": batch_number, "C": float(C), "tol": float(tol), "layer": layer,
              "solver": "full-batch L-BFGS", "input_state": mode}
    model_path = metadata_path = None
    if output_path is not None:
        model_path = model.write(output_path)
        logger.info(f"  Saved model to: {model_path}")
        # the reference's side file (training.py:698-718): <stem>_celltypist.json beside the model
        metadata_path = model_path[:-len(".npz")] + "_celltypist.json"
        with open(metadata_path, "w") as f:
            json.dump({"model_name": model_name, "label_column": label_column, "n_cells": int(n), "n_genes": G,
                       "n_cell_types": int(T), "cell_types": [str(c) for c in names], "features": features,
                       "training_params": params, "n_iter": [int(v) for v in res["n_iter"]],
                       "converged": [bool(v) for v in res["converged"]],
                       "grad_norm": [float(v) for v in res["grad_norm"]]}, f, indent=1)
        logger.info(f"  Saved metadata to: {metadata_path}")
    return {"model_path": model_path, "metadata_path": metadata_path, "model_name": model_name, "n_cells_trained": int(n),
            "n_genes": G, "n_cell_types": int(T), "cell_types": [str(c) for c in names], "model": model,
            "n_iter": res["n_iter"], "converged": res["converged"], "grad_norm": res["grad_norm"],
            "training_params": params}
