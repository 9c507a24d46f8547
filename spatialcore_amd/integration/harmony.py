"""harmony_integrate: Harmony batch correction of an embedding (sc_harmony_*).

Korsunsky et al. 2019 ("Fast, sensitive and accurate integration of single-cell data with Harmony"), the step scanpy
exposes as ``external.pp.harmony_integrate`` on top of harmonypy, restated from the published algorithm.  harmonypy is not a
dependency of this package and is not installed where the package is tested: parity with it is NOT pinned by any test.  The
arithmetic is checked against a plain numpy restatement of the algorithm (tests/harmony_restated.py).

Differences from harmonypy, on purpose:
 - strided blocks: cell i is updated in block ``i mod n_blocks``, not in a freshly drawn random order.  A strided block mixes
   the batches even when the cells are sorted by batch, and the result is a function of the arguments alone;
 - no subtraction: the device keeps one cluster x batch table per block and adds the other blocks' tables in a fixed order
   where harmonypy subtracts a block's mass and adds it back, which accumulates cancellation error;
 - the row-minimum shift: the distances of a cell are shifted by their minimum before ``exp``, which cancels in the
   normalisation and keeps a small ``sigma`` from underflowing a whole row to 0 / 0;
 - the start is the package's own k-means (sc_kmeans_fit, which replays sklearn's ``KMeans``), not harmonypy's;
 - a single ``key``.

Everything that touches the n cells runs in HIP; this module holds the loop over the outer rounds.  There is no CPU
fallback."""

from __future__ import annotations

import math
import numbers

import numpy as np
from scipy import sparse

from spatialcore_amd import _lib
from spatialcore_amd._batches import batch_groups
from spatialcore_amd._kmeans_draws import kmeans_draws
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata

logger = get_logger("harmony")

D_MAX, K_MAX, B_MAX, BLOCKS_MAX = 64, 128, 64, 1024
KMEANS_MAX_ITER = 25          # harmonypy's start
_SUPPORTED = (f"2 <= cells <= 2^31 - 1, 1 <= features <= {D_MAX}, 2 <= batches <= {B_MAX}, 2 <= nclust <= min({K_MAX}, cells), "
              f"at most {BLOCKS_MAX} blocks")


def default_nclust(n: int) -> int:
    """harmonypy's ``min(round(n / 30), 100)``, but at least 2."""
    return max(2, min(int(round(n / 30.0)), 100))


def n_blocks(n: int, block_size: float) -> int:
    """``ceil(1 / block_size)`` blocks, capped at n."""
    return min(int(math.ceil(1.0 / block_size)), int(n))


def _number(name: str, value, low: float, strict: bool) -> float:
    ok = isinstance(value, numbers.Real) and not isinstance(value, bool) and math.isfinite(value) \
        and (value > low if strict else value >= low)
    if not ok:
        raise ValueError(f"{name} must be a finite number {'>' if strict else '>='} {low:g}, got {value!r}")
    return float(value)


def _count(name: str, value, low: int) -> int:
    if not isinstance(value, numbers.Integral) or isinstance(value, bool) or value < low:
        raise ValueError(f"{name} must be an integer >= {low}, got {value!r}")
    return int(value)


def _epsilon(name: str, value) -> float:
    if not isinstance(value, numbers.Real) or isinstance(value, bool) or math.isnan(value):
        raise ValueError(f"{name} must be a number (negative: never stop early), got {value!r}")
    return float(value)


def _basis(adata, basis) -> np.ndarray:
    if not isinstance(basis, str) or basis not in adata.obsm:
        raise ValueError(f"basis={basis!r} is not an entry of adata.obsm (available: {sorted(adata.obsm)})")
    Z = adata.obsm[basis]
    Z = Z.toarray() if sparse.issparse(Z) else np.asarray(getattr(Z, "values", Z))
    if Z.ndim != 2 or Z.dtype not in (np.float32, np.float64):
        raise ValueError(f"obsm[{basis!r}] must be a 2-D float32 or float64 array, got shape {Z.shape} of {Z.dtype}")
    if not 1 <= Z.shape[1] <= D_MAX:
        raise ValueError(f"obsm[{basis!r}] has {Z.shape[1]} features; supported: {_SUPPORTED}")
    if not 2 <= Z.shape[0] <= 2**31 - 1:
        raise ValueError(f"obsm[{basis!r}] has {Z.shape[0]} cells; supported: {_SUPPORTED}")
    Z = np.ascontiguousarray(Z)
    if not np.all(np.isfinite(Z)):
        raise ValueError(f"obsm[{basis!r}] contains NaN or infinite values")
    zero = int(np.count_nonzero(~Z.any(axis=1)))
    if zero:
        raise ValueError(f"obsm[{basis!r}] has {zero} row(s) that are all zero; a cell without a direction cannot be "
                         "placed on the unit sphere")
    return Z


def unit_rows(Z) -> np.ndarray:
    """Every row scaled to unit L2 norm, in float64, the sum of squares added in feature order (the device's Zc)."""
    Z = np.asarray(Z, dtype=np.float64)
    q = np.zeros(Z.shape[0])
    for j in range(Z.shape[1]):
        q = q + Z[:, j] * Z[:, j]
    return Z / np.sqrt(q)[:, None]


def kmeans_start(ctx, Zc, nclust: int, n_init: int, random_state) -> np.ndarray:
    """The starting centres: sc_kmeans_fit on the unit rows with the draws of ``RandomState(random_state)``, as
    identify_niches supplies them."""
    tol = float(np.mean(np.var(Zc, axis=0)) * 1e-4)
    fit = ctx.kmeans(Zc, nclust, n_init, KMEANS_MAX_ITER, tol, Zc.mean(axis=0), kmeans_draws(random_state, n_init, nclust))
    centres = np.asarray(fit["centers"], dtype=np.float64)
    if not np.all(np.isfinite(centres)) or not centres.any(axis=1).all():
        raise ValueError("the k-means start produced a centre at the origin; choose another nclust or random_state")
    return centres


def harmony_integrate(adata, key, *, basis: str = "X_pca", adjusted_basis: str = "X_pca_harmony", theta: float = 2.0,
                      lamb: float = 1.0, sigma: float = 0.1, nclust=None, max_iter_harmony: int = 10,
                      max_iter_kmeans: int = 20, epsilon_cluster: float = 1e-5, epsilon_harmony: float = 1e-4,
                      block_size: float = 0.05, n_init: int = 10, random_state=0, device: int = 0):
    """Removes the effect of the batches in ``obs[key]`` from the embedding ``obsm[basis]`` (Harmony, Korsunsky et al. 2019),
    on the GPU, and writes the corrected embedding to ``obsm[adjusted_basis]``.  It sits between ``pca`` and ``neighbors``:
    ``neighbors(adata, use_rep="X_pca_harmony")`` takes the result as it is.

    ``key`` is one column of ``obs``; its categories are taken in sorted order, without missing values, at least 2 cells
    each and at least 2 of them (as ``highly_variable_genes(batch_key=...)``).  ``basis`` is float32 or float64 with at most
    64 features, finite, without an all-zero row; the device works in float64.  The names and defaults are scanpy's and
    harmonypy's: ``theta`` the diversity penalty (0: none), ``lamb`` the ridge penalty, ``sigma`` the softness of the
    assignment, ``nclust`` the clusters (default ``min(round(cells / 30), 100)``, at least 2; at most 128),
    ``max_iter_harmony`` outer rounds of at most ``max_iter_kmeans`` clustering rounds, ``block_size`` the share of the cells
    updated at once (``ceil(1 / block_size)`` blocks, at most 1024).  A clustering stops when the objective's windows of 3
    rounds differ by less than ``epsilon_cluster`` relatively, the outer loop when the last objectives of two consecutive
    rounds differ by less than ``epsilon_harmony`` relatively; a negative epsilon never stops early.  The start is the
    package's k-means with ``n_init`` runs of ``RandomState(random_state)``.

    The rule restates the published one.  harmonypy is not installed where this package is tested, so parity with
    ``scanpy.external.pp.harmony_integrate`` is NOT pinned.  On purpose it differs from harmonypy in: strided blocks (cell i
    is in block ``i mod n_blocks``) in place of a random order; per-block tables that are added, never subtracted; the
    row-minimum shift of the distances before ``exp``; the sklearn-replayed k-means start; a single ``key``.  Out of scope:
    several keys at once, per-batch ``theta`` / ``tau`` scaling, automatic ``lamb``, ``reference_values``.

    Writes ``obsm[adjusted_basis]`` (float64) and ``uns["harmony"] = {"params", "nclust", "n_blocks", "batches"
    (category -> cells), "objectives" (per outer round: the objective after every clustering round), "objective_start",
    "n_rounds", "converged"}`` and the usual ``uns["spatialcore_metadata"]`` entry.  Returns ``adata``.  The result is a
    function of the arguments alone, bit for bit."""
    theta = _number("theta", theta, 0.0, strict=False)
    lamb = _number("lamb", lamb, 0.0, strict=True)
    sigma = _number("sigma", sigma, 0.0, strict=True)
    block_size = _number("block_size", block_size, 0.0, strict=True)
    if block_size > 1.0 or math.ceil(1.0 / block_size) > BLOCKS_MAX:
        raise ValueError(f"block_size must lie in [1 / {BLOCKS_MAX}, 1], got {block_size!r}")
    max_outer, max_inner = _count("max_iter_harmony", max_iter_harmony, 1), _count("max_iter_kmeans", max_iter_kmeans, 1)
    if max_inner > 4096:
        raise ValueError(f"max_iter_kmeans must be at most 4096, got {max_inner}")
    n_init = _count("n_init", n_init, 1)
    eps_c, eps_h = _epsilon("epsilon_cluster", epsilon_cluster), _epsilon("epsilon_harmony", epsilon_harmony)
    if not isinstance(adjusted_basis, str) or not adjusted_basis:
        raise ValueError(f"adjusted_basis must be a non-empty string, got {adjusted_basis!r}")
    if not isinstance(key, str):
        raise ValueError(f"key={key!r}: one column of adata.obs (several keys at once are not supported)")
    groups = batch_groups(adata, key, "key")
    B = len(groups)
    if not 2 <= B <= B_MAX:
        raise ValueError(f"adata.obs[{key!r}] has {B} batch(es); supported: {_SUPPORTED}")
    Z = _basis(adata, basis)
    n, d = Z.shape
    K = default_nclust(n) if nclust is None else _count("nclust", nclust, 2)
    if K > min(K_MAX, n):
        raise ValueError(f"nclust={K} is outside the supported range; supported: {_SUPPORTED}")
    codes = np.empty(n, dtype=np.int32)
    for b, (_, rows) in enumerate(groups):
        codes[rows] = b
    nb = n_blocks(n, block_size)
    logger.info(f"Harmony: {n:,} cells x {d} features of obsm[{basis!r}], {B} batches of {key!r}, {K} clusters, {nb} blocks, "
                f"theta={theta:g}, lamb={lamb:g}, sigma={sigma:g}")

    ctx = _lib.default_context(device)
    Y = kmeans_start(ctx, unit_rows(Z), K, n_init, random_state)
    objectives, converged = [], False
    try:
        start = ctx.harmony_begin(Z, codes, B, Y, nb, sigma, theta, lamb)
        for _ in range(max_outer):
            objectives.append(ctx.harmony_cluster(max_inner, eps_c))
            ctx.harmony_correct()
            if len(objectives) > 1:
                old, new = objectives[-2][-1], objectives[-1][-1]
                if abs(old - new) / abs(old) < eps_h:
                    converged = True
                    break
        Zcorr = ctx.harmony_get("Zcorr")
    finally:
        ctx.harmony_end()
    if not np.all(np.isfinite(Zcorr)):
        raise _lib.SpatialCoreHipError("harmony_integrate: the corrected embedding is not finite")
    adata.obsm[adjusted_basis] = Zcorr
    params = {"key": key, "basis": basis, "adjusted_basis": adjusted_basis, "theta": theta, "lamb": lamb, "sigma": sigma,
              "nclust": nclust, "max_iter_harmony": max_outer, "max_iter_kmeans": max_inner, "epsilon_cluster": eps_c,
              "epsilon_harmony": eps_h, "block_size": block_size, "n_init": n_init, "random_state": random_state}
    adata.uns["harmony"] = {"params": params, "nclust": K, "n_blocks": nb,
                            "batches": {cat: int(rows.size) for cat, rows in groups},
                            "objective_start": float(start), "objectives": [o.copy() for o in objectives],
                            "n_rounds": len(objectives), "converged": converged}
    logger.info(f"Harmony: {len(objectives)} outer round(s), {'converged' if converged else 'not converged'}; "
                f"stored obsm[{adjusted_basis!r}]")
    update_metadata(adata, "harmony_integrate", {**params, "n_clusters": K, "n_blocks": nb, "n_batches": B},
                    {"obsm": adjusted_basis, "uns": "harmony", "n_rounds": len(objectives), "converged": converged})
    return adata
