"""pca / project_pca: exact covariance PCA of a sparse expression matrix (sc_pca_*).

The algorithm is sklearn 1.7.2's ``PCA(svd_solver="covariance_eigh")``: ``C = (X^T X - N mu mu^T) / (N - 1)``, a symmetric
eigendecomposition, eigenvalues descending with negatives clipped to 0, and ``svd_flip(u_based_decision=False)``.  What
touches the N cells runs in HIP: the optional ``log1p`` normalisation, the Gram matrix ``X^T X`` with the column sums
(fp64 MFMA) and the projection ``X V^T - V mu``.  The G x G eigenproblem between the two is solved here on the host with
LAPACK (``scipy.linalg.eigh``), as ``diffusion/maps.py`` solves its tridiagonal problem: O(G^3), measured at 0.025 s for
G = 500 and 5.3 s for G = 4096 on 16 CPU threads of the MI355X host (profiles/pca_1m.json) -- hence the limit of 4096
genes.  There is no CPU fallback for the device part."""

from __future__ import annotations

import numbers
from typing import Optional, Sequence, Union

import numpy as np
from scipy import linalg

from spatialcore_amd import _lib
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd._sparse_input import canonical_csr, gene_columns

logger = get_logger("pca")

G_MAX = 4096      # the host solves a G x G eigenproblem and the device holds partial G x G sums
K_MAX = 64        # sc_knn_dense's D_MAX: every result feeds diffusion_map
DTYPES = ("float32", "float64")
_SUPPORTED = (f"2 <= cells <= 2^31 - 1, 1 <= genes <= {G_MAX}, 1 <= n_comps <= min({K_MAX}, cells - 1, genes), "
              'dtype "float32" or "float64"')


# ---- arguments -----------------------------------------------------------------------------------------------------------
def _check_flag(name: str, value) -> bool:
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, got {value!r}")
    return bool(value)


def _check_dtype(dtype) -> str:
    try:
        name = np.dtype(dtype).name
    except TypeError:
        name = None
    if name not in DTYPES:
        raise ValueError(f"dtype={dtype!r} is not supported; supported: {_SUPPORTED}")
    return name


def _check_key(key_added) -> None:
    if key_added is not None and (not isinstance(key_added, str) or not key_added):
        raise ValueError(f"key_added must be None or a non-empty string, got {key_added!r}")


def _keys(key_added):
    """(obsm, varm, uns) keys as scanpy >= 1.10 names them."""
    return ("X_pca", "PCs", "pca") if key_added is None else (key_added, key_added, key_added)


def _matrix(X, cols: np.ndarray, n_vars: int, nonneg: bool):
    """The matrix restricted to ``cols`` as sc_pca_begin takes it."""
    Xc, _ = canonical_csr(X, cols, n_vars, real=True, all_zero="the expression matrix is all zero: there is nothing to decompose",
                          negative="normalize=True needs non-negative values (counts); the expression matrix has negative entries"
                          if nonneg else None)
    if Xc.nnz > 2**32 - 1:
        raise ValueError("at most 2^32 - 1 stored entries are supported")
    return Xc


def _check_shape(n: int, G: int, n_comps: Optional[int]) -> None:
    if not 2 <= n <= 2**31 - 1:
        raise ValueError(f"PCA needs 2 <= cells <= 2^31 - 1, got {n}; supported: {_SUPPORTED}")
    if not 1 <= G <= G_MAX:
        raise ValueError(f"PCA is limited to {G_MAX} genes (the host solves a genes x genes eigenproblem), got {G}: "
                         f"select genes first; supported: {_SUPPORTED}")
    if n_comps is not None and n_comps > min(K_MAX, n - 1, G):
        raise ValueError(f"n_comps={n_comps} exceeds min({K_MAX}, cells - 1, genes) = {min(K_MAX, n - 1, G)}; "
                         f"supported: {_SUPPORTED}")


# ---- the host part ---------------------------------------------------------------------------------------------------------
def covariance_from_gram(gram, colsum, n: int):
    """``mu = colsum / N`` and ``C = (gram - N mu mu^T) / (N - 1)`` in numpy fp64, sklearn's order of operations."""
    gram = np.asarray(gram, dtype=np.float64)
    mean = np.asarray(colsum, dtype=np.float64) / n
    C = gram - n * mean.reshape(-1, 1) * mean.reshape(1, -1)
    C /= n - 1
    return mean, C


def correlation_scaling(C, mean, n: int):
    """``C <- D^-1 C D^-1`` with ``D = sqrt(diag C)``, the sample standard deviation (ddof = 1).  A gene that
    StandardScaler would call constant (variance <= N eps variance + (N mean eps)^2, which covers 0) gets scale 1 and a
    zero row and column.  Returns (scale, the scaled matrix)."""
    var = np.clip(np.diag(C), 0.0, None)
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.where(constant, 1.0, np.sqrt(var))
    Cs = C / scale.reshape(-1, 1) / scale.reshape(1, -1)
    Cs[constant, :] = 0.0
    Cs[:, constant] = 0.0
    return scale, Cs


def eigen_decompose(C, n_comps: int):
    """``scipy.linalg.eigh`` of the symmetric ``C``, flipped to descending order, negatives clipped to 0, each component's
    sign chosen so that its entry of largest magnitude (the first such) is positive.  Returns (variance, variance_ratio,
    components), the first ``n_comps`` of each; the ratio is relative to the sum of all (clipped) eigenvalues, the trace.

    A gene whose row of ``C`` is exactly zero (an all-zero gene) is decoupled from the others: the solve runs on the other
    genes, every component's loading of that gene is exactly 0, and the gene's own unit vector closes the spectrum with
    eigenvalue 0 (LAPACK on the full matrix leaves loadings of 1e-20 there)."""
    G = C.shape[0]
    live = np.flatnonzero(np.any(C != 0.0, axis=0))
    dead = np.setdiff1d(np.arange(G), live)
    lam, vec = np.zeros(G), np.zeros((G, G))
    if live.size:
        w, v = linalg.eigh(C[np.ix_(live, live)])
        lam[:live.size] = w[::-1]
        vec[np.ix_(live, np.arange(live.size))] = v[:, ::-1]
    vec[dead, live.size + np.arange(dead.size)] = 1.0
    lam[lam < 0.0] = 0.0
    Vt = vec.T
    top = np.argmax(np.abs(Vt), axis=1)
    signs = np.sign(Vt[np.arange(Vt.shape[0]), top])
    signs[signs == 0] = 1.0
    Vt = Vt * signs[:, None]
    total = lam.sum()
    ratio = lam / total if total > 0 else np.zeros_like(lam)
    return lam[:n_comps].copy(), ratio[:n_comps].copy(), np.ascontiguousarray(Vt[:n_comps])


def projection_operands(components, mean, scale):
    """What sc_pca_project takes: ``V / sigma`` (K x G) and ``offset = (V / sigma) mu``, added over the genes in index
    order from 0 with multiply and add rounded separately."""
    Vs = np.ascontiguousarray(np.asarray(components, dtype=np.float64) / np.asarray(scale, dtype=np.float64)[None, :])
    offset = np.zeros(Vs.shape[0])
    for g in range(Vs.shape[1]):
        offset = offset + Vs[:, g] * mean[g]
    return Vs, offset


def host_decompose(gram, colsum, n: int, n_comps: int, scale: bool = False) -> dict:
    """Everything between sc_pca_gram and sc_pca_project."""
    mean, C = covariance_from_gram(gram, colsum, n)
    if scale:
        sigma, C = correlation_scaling(C, mean, n)
    else:
        sigma = np.ones_like(mean)
    variance, ratio, components = eigen_decompose(C, n_comps)
    return {"mean": mean, "scale": sigma, "variance": variance, "variance_ratio": ratio, "components": components}


# ---- public functions --------------------------------------------------------------------------------------------------------
def _store(adata, function: str, key_added, scores, components, cols, info: dict, meta: dict) -> None:
    k_obsm, k_varm, k_uns = _keys(key_added)
    adata.obsm[k_obsm] = scores
    loadings = np.zeros((len(adata.var_names), components.shape[0]), dtype=np.float64)
    loadings[cols] = components.T
    adata.varm[k_varm] = loadings
    adata.uns[k_uns] = info
    update_metadata(adata, function, meta, {"obsm": k_obsm, "varm": k_varm, "uns": k_uns})


def pca(adata, n_comps: int = 50, *, genes: Optional[Union[str, Sequence[str]]] = None, layer: Optional[str] = None,
        normalize: bool = False, target_sum: float = 1e4, scale: bool = False, key_added: Optional[str] = None,
        dtype="float32", copy: bool = False, device: int = 0):
    """Principal component analysis of ``adata.X`` (or ``layers[layer]``) restricted to ``genes`` in the order given, as
    sklearn's ``PCA(n_comps, svd_solver="covariance_eigh")`` computes it, on the GPU.

    The matrix may be scipy sparse of any format or dense, of any real type, and must be finite; negative values are legal
    unless ``normalize=True``, which applies ``log1p(x / rowsum * target_sum)`` on the device first (an all-zero cell
    stays zero).  ``scale=True`` is PCA of the correlation matrix: scanpy's ``pp.scale`` without a clip, then PCA; a gene
    of zero variance gets scale 1 and zero loadings.  Limits: 2 <= cells <= 2^31 - 1, 1 <= genes <= 4096,
    1 <= ``n_comps`` <= min(64, cells - 1, genes).

    Writes ``obsm["X_pca"]`` (cells x n_comps in ``dtype``, "float32" -- the fp64 result rounded once -- or "float64"),
    ``varm["PCs"]`` (n_vars x n_comps, always float64 so that ``project_pca`` reproduces the scores bit for bit; rows of
    genes not in use are zero) and ``uns["pca"]`` = {``variance``, ``variance_ratio`` (of the total variance),
    ``mean`` and ``scale`` (per gene in use, after the normalisation; all ones without ``scale``), ``genes``,
    ``params``}; with ``key_added`` all three keys are ``key_added``.  Appends the usual entry to
    ``uns["spatialcore_metadata"]``.  The result is a function of the arguments alone, bit for bit."""
    if not isinstance(n_comps, numbers.Integral) or isinstance(n_comps, bool) or not 1 <= n_comps <= K_MAX:
        raise ValueError(f"n_comps must be an integer in 1..{K_MAX}, got {n_comps!r}; supported: {_SUPPORTED}")
    K = int(n_comps)
    normalize, scale = _check_flag("normalize", normalize), _check_flag("scale", scale)
    if not isinstance(target_sum, numbers.Real) or isinstance(target_sum, bool) or not np.isfinite(target_sum) or target_sum <= 0:
        raise ValueError(f"target_sum must be a finite number > 0, got {target_sum!r}")
    dtype = _check_dtype(dtype)
    _check_key(key_added)
    names, cols = gene_columns(adata, genes)
    X = adata.layers[layer] if layer is not None else adata.X
    _check_shape(int(X.shape[0]), len(names), K)
    Xc = _matrix(X, cols, len(adata.var_names), normalize)
    n, G = Xc.shape
    logger.info(f"PCA (covariance, exact): {n:,} cells x {G} genes, {K} components"
                + (", log1p-normalised" if normalize else "") + (", scaled" if scale else ""))
    ctx = _lib.default_context(device)
    ctx.pca_begin(Xc.indptr, Xc.indices, Xc.data, G, normalize, float(target_sum))
    try:
        colsum, gram = ctx.pca_gram()
        host = host_decompose(gram, colsum, n, K, scale)
        Vs, offset = projection_operands(host["components"], host["mean"], host["scale"])
        scores = ctx.pca_project(Vs, offset, dtype)
    finally:
        ctx.pca_end()
    adata = adata.copy() if copy else adata
    params = {"n_comps": K, "normalize": normalize, "target_sum": float(target_sum), "scale": scale, "dtype": dtype,
              "layer": layer, "solver": "covariance_eigh"}
    info = {"variance": host["variance"], "variance_ratio": host["variance_ratio"], "mean": host["mean"],
            "scale": host["scale"], "genes": list(names), "params": params}
    _store(adata, "pca", key_added, scores, host["components"], cols, info,
           {**params, "genes": list(names[:10]) if len(names) > 10 else list(names), "n_genes": len(names),
            "key_added": key_added})
    return adata


def _stored_result(source, key_added):
    """(uns entry, loadings K x genes in the entry's gene order) of a ``pca`` result."""
    _, k_varm, k_uns = _keys(key_added)
    if isinstance(source, tuple) and len(source) == 2 and isinstance(source[0], dict):
        info, L = source
        L = np.asarray(L, dtype=np.float64)
    elif hasattr(source, "uns") and hasattr(source, "varm"):
        if k_uns not in source.uns or k_varm not in source.varm:
            raise ValueError(f"source holds no PCA result under uns[{k_uns!r}] / varm[{k_varm!r}]: run pca first "
                             "(key_added names the result in source and in adata)")
        info = source.uns[k_uns]
        L = None
    else:
        raise ValueError("source must be an AnnData-like with a pca result, or (that result's uns dict, loadings genes x n_comps)")
    missing = [k for k in ("mean", "scale", "genes", "params") if k not in info]
    if missing:
        raise ValueError(f"the stored PCA result lacks {missing}")
    genes = [str(g) for g in info["genes"]]
    if L is None:
        absent = sorted(set(genes) - set(source.var_names))
        if absent:
            raise ValueError(f"source.var_names lacks genes of its own PCA result: {absent[:10]}")
        L = np.asarray(source.varm[k_varm], dtype=np.float64)[[source.var_names.get_loc(g) for g in genes]]
    if L.ndim != 2 or L.shape[0] != len(genes) or not 1 <= L.shape[1] <= K_MAX:
        raise ValueError(f"loadings must be (genes, n_comps) = ({len(genes)}, 1..{K_MAX}), got {L.shape}")
    mean, sigma = np.asarray(info["mean"], dtype=np.float64), np.asarray(info["scale"], dtype=np.float64)
    if mean.shape != (len(genes),) or sigma.shape != (len(genes),):
        raise ValueError("the stored mean and scale must have one entry per gene of the result")
    if not (np.all(np.isfinite(L)) and np.all(np.isfinite(mean)) and np.all(np.isfinite(sigma)) and np.all(sigma > 0)):
        raise ValueError("the stored loadings, mean and scale must be finite, the scale positive")
    return info, genes, np.ascontiguousarray(L.T), mean, sigma


def project_pca(adata, source, *, layer: Optional[str] = None, key_added: Optional[str] = None, copy: bool = False,
                device: int = 0):
    """Applies a stored decomposition to the cells of ``adata``: the same normalisation, centring, scaling and loadings.

    ``source`` is an AnnData-like that ``pca`` wrote to (its ``uns`` / ``varm`` entries under ``key_added``'s names), or
    the pair (that ``uns`` entry, loadings genes x n_comps in the entry's gene order).  Genes are matched by name; a gene
    of the decomposition that ``adata`` lacks is an error.  Writes the keys of ``pca`` into ``adata``;
    ``project_pca(adata, adata)`` reproduces ``obsm["X_pca"]`` byte for byte."""
    _check_key(key_added)
    info, genes, components, mean, sigma = _stored_result(source, key_added)
    p = dict(info["params"])
    dtype = _check_dtype(p.get("dtype", "float32"))
    normalize = bool(p.get("normalize", False))
    target_sum = float(p.get("target_sum", 1e4))
    missing = sorted(set(genes) - set(adata.var_names))
    if missing:
        raise ValueError(f"Genes of the decomposition not found in adata.var_names: {missing[:10]}")
    names, cols = gene_columns(adata, genes)
    X = adata.layers[layer] if layer is not None else adata.X
    _check_shape(int(X.shape[0]), len(names), None)
    Xc = _matrix(X, cols, len(adata.var_names), normalize)
    n, G = Xc.shape
    K = components.shape[0]
    logger.info(f"PCA projection: {n:,} cells x {G} genes onto {K} stored components")
    Vs, offset = projection_operands(components, mean, sigma)
    ctx = _lib.default_context(device)
    ctx.pca_begin(Xc.indptr, Xc.indices, Xc.data, G, normalize, target_sum)
    try:
        scores = ctx.pca_project(Vs, offset, dtype)
    finally:
        ctx.pca_end()
    adata = adata.copy() if copy else adata
    out = {**{k: info[k] for k in ("variance", "variance_ratio") if k in info}, "mean": mean, "scale": sigma,
           "genes": list(names), "params": {**p, "layer": layer}}
    _store(adata, "project_pca", key_added, scores, components, cols, out,
           {"n_comps": K, "n_genes": G, "layer": layer, "key_added": key_added})
    return adata
