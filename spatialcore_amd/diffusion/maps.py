"""diffusion_map / diffusion_pseudotime.

The neighbour search, the kernel matrix, its normalisation, the connected components and every Lanczos step run in HIP,
in fp64 and in one documented summation order (sc_knn_dense_gram and sc_diffmap_graph through _rep_graph.py, the path
``neighbors`` takes; sc_lanczos_*); the host checks the arguments, solves the small tridiagonal eigenproblem between
batches of steps and applies the sign rule.  There is no CPU fallback.  Pseudotime is O(cells x components) on a stored
map and runs in numpy."""

from __future__ import annotations

import numbers
from typing import Optional

import numpy as np
from scipy import sparse
from scipy.linalg import eigh_tridiagonal

from spatialcore_amd import _lib
from spatialcore_amd._cell_graph import kernel_matrix
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd._rep_graph import (COMPS_MAX, COMPS_MIN, _SUPPORTED, _check_key, _is_int, check_n_neighbors, representation,
                                        resident_graph)

logger = get_logger("diffusion")

BASIS_DEFAULT = 1024
CHECK_EVERY = 16          # Lanczos steps between two solutions of the tridiagonal problem


def _sign(vecs: np.ndarray) -> np.ndarray:
    """Every column signed so that its entry of largest magnitude (lowest index among equals) is positive."""
    lead = np.argmax(np.abs(vecs), axis=0)
    flip = vecs[lead, np.arange(vecs.shape[1])] < 0
    vecs[:, flip] = -vecs[:, flip]
    return vecs


def _eigenpairs(ctx, n: int, n_comps: int, tol: float, max_basis: int, random_state):
    """The n_comps largest eigenpairs of the resident transition matrix: Lanczos steps on the device, the tridiagonal
    problem here every CHECK_EVERY steps.  Returns (values descending, vectors (n, n_comps), residuals, steps)."""
    start = np.random.RandomState(random_state).standard_normal(n)
    ctx.lanczos_begin(start, max_basis)
    try:
        m, worst = 0, np.inf
        while m < max_basis:
            alpha, beta = ctx.lanczos_run(min(CHECK_EVERY, max_basis - m))
            m = alpha.size
            if m < n_comps:
                continue
            theta, S = eigh_tridiagonal(alpha, beta[1:m])
            top = np.arange(m - 1, m - 1 - n_comps, -1)
            estimate = np.abs(beta[m] * S[m - 1, top])
            worst = float(estimate.max())
            if worst <= tol / 4 or m == max_basis:
                vecs, res = ctx.lanczos_ritz(S[:, top], theta[top])
                worst = float(res.max())
                if worst <= tol:
                    return theta[top].copy(), _sign(vecs), res, m
        raise RuntimeError(f"diffusion_map: the {n_comps} leading eigenpairs did not converge to tol={tol:g} within "
                           f"max_basis={max_basis} Lanczos steps (worst residual {worst:.3e}); raise max_basis or tol")
    finally:
        ctx.lanczos_end()


def diffusion_map(adata, use_rep: str = "X_nmf", n_neighbors: int = 15, n_comps: int = 15, *, graph=None,
                  tol: float = 1e-10, max_basis: Optional[int] = None, random_state: int = 0, key_added: str = "diffmap",
                  store_graph: bool = False, copy: bool = False, device: int = 0):
    """Diffusion map (Haghverdi et al. 2016) of the cells in the representation ``adata.obsm[use_rep]``, on the GPU.

    Exact ``n_neighbors`` nearest neighbours in feature space by (squared distance, index); local scale = median squared
    neighbour distance; Gaussian kernel with the geometric-mean prefactor on the symmetric union of the lists; density
    normalisation (alpha = 1) and the symmetric transition matrix T; the ``n_comps`` algebraically largest eigenpairs of
    T by Lanczos with full reorthogonalisation, accepted at a true residual ``||T psi - lambda psi|| <= tol``.

    ``use_rep`` names a float32 / float64 (anything else is converted to float64) finite ``obsm`` entry with 1..64
    columns (``"spatial"`` works); 2 <= ``n_neighbors`` <= 32 and 2 <= ``n_comps`` <= 64, both below the number of
    cells.  ``graph`` (an ``obsp`` name or a scipy sparse matrix: cells x cells, symmetric, non-negative, no empty row)
    replaces the search and the kernel; ``use_rep`` and ``n_neighbors`` are then ignored.  ``max_basis`` caps the Lanczos
    steps (default min(cells, 1024), lowered to what fits in free device memory).  A disconnected graph, a cell whose
    local scale is zero and anything else unsupported raise ``ValueError``; running out of ``max_basis`` or a Krylov
    breakdown raise ``RuntimeError``.

    Writes ``obsm["X_" + key_added]`` (cells x n_comps float64, unit columns, each signed so that its largest entry is
    positive; column 0 is the stationary vector), ``uns[key_added + "_evals"]`` (descending), ``uns[key_added]``
    (``params``, ``n_steps``, ``residuals``, ``n_edges``, ``use_rep``, ``n_features``), with ``store_graph`` also
    ``obsp[key_added + "_connectivities"]`` (the kernel matrix, float64 CSR), and the usual entry in
    ``uns["spatialcore_metadata"]``.  The result is a function of the arguments alone, bit for bit."""
    _check_key("key_added", key_added)
    n = int(adata.n_obs)
    if not _is_int(n_comps) or not COMPS_MIN <= n_comps <= COMPS_MAX or n_comps >= n:
        raise ValueError(f"n_comps must be an integer in {COMPS_MIN}..{COMPS_MAX} and below the {n} cells, got {n_comps!r}; "
                         f"supported: {_SUPPORTED}")
    if not isinstance(tol, numbers.Real) or isinstance(tol, bool) or not np.isfinite(tol) or tol <= 0:
        raise ValueError(f"tol must be a finite number > 0, got {tol!r}")
    if max_basis is not None and (not _is_int(max_basis) or max_basis < n_comps):
        raise ValueError(f"max_basis must be an integer >= n_comps = {n_comps}, got {max_basis!r}")
    if not _is_int(random_state) or not 0 <= random_state < 2 ** 32:
        raise ValueError(f"random_state must be an integer in [0, 2^32), got {random_state!r}")
    A = R = None
    if graph is not None:
        A = kernel_matrix(adata, graph, n)
    else:
        check_n_neighbors(n_neighbors, n)
        R = representation(adata, use_rep)

    ctx = _lib.default_context(device)
    if A is not None:
        logger.info(f"diffusion map: {n:,} cells, caller's graph with {A.nnz:,} stored entries, {n_comps} components")
        n_components, n_edges = ctx.diffmap_graph_csr(A.indptr, A.indices, A.data), int(A.nnz)
    else:
        logger.info(f"diffusion map: {n:,} cells x {R.shape[1]} features, {n_neighbors} neighbours, {n_comps} components")
        info = resident_graph(ctx, R, int(n_neighbors))
        n_components, n_edges = info["n_components"], info["n_edges"]
    if n_components != 1:
        raise ValueError(f"the neighbour graph has {n_components} connected components; a diffusion map needs one "
                         "(disconnected graphs are not supported): use a larger n_neighbors")
    if store_graph:
        indptr, indices, w = ctx.diffmap_graph_get()
    cap = min(n, BASIS_DEFAULT) if max_basis is None else min(int(max_basis), n)
    # vectors of n doubles that fit in 80 % of the free device memory, less the basis' extra one and the Ritz vectors
    fit = int(0.8 * ctx.device_mem_free() // (8 * n)) - 1 - n_comps
    if max_basis is None and fit < cap:
        cap = max(fit, n_comps)
        logger.warning(f"max_basis lowered to {cap}: the Lanczos basis has to fit in free device memory")
    evals, vecs, res, steps = _eigenpairs(ctx, n, int(n_comps), float(tol), cap, int(random_state))
    logger.info(f"diffusion map: {steps} Lanczos steps, worst residual {res.max():.2e}")

    adata = adata.copy() if copy else adata
    params = {"n_neighbors": None if A is not None else int(n_neighbors), "n_comps": int(n_comps), "tol": float(tol),
              "max_basis": cap, "random_state": int(random_state), "graph": None if A is None else
              (graph if isinstance(graph, str) else "matrix")}
    adata.obsm["X_" + key_added] = vecs
    adata.uns[key_added + "_evals"] = evals
    adata.uns[key_added] = {"params": params, "n_steps": int(steps), "residuals": res, "n_edges": int(n_edges),
                            "use_rep": None if A is not None else use_rep,
                            "n_features": None if A is not None else int(R.shape[1])}
    outputs = {"obsm": "X_" + key_added, "uns": [key_added, key_added + "_evals"]}
    if store_graph:
        adata.obsp[key_added + "_connectivities"] = sparse.csr_matrix((w, indices, indptr), shape=(n, n))
        outputs["obsp"] = key_added + "_connectivities"
    update_metadata(adata, "diffusion_map", {**params, "use_rep": use_rep if A is None else None, "key_added": key_added,
                                             "store_graph": bool(store_graph)}, outputs)
    return adata


def diffusion_pseudotime(adata, root, n_dcs: int = 10, *, key: str = "diffmap", key_added: str = "dpt_pseudotime",
                         copy: bool = False):
    """Diffusion pseudotime (Haghverdi et al. 2016) from the cell ``root`` on the map stored under ``key``.

    With ``c_l = lambda_l / (1 - lambda_l)`` for l = 1 .. n_dcs - 1 (component 0, the stationary one, is left out):
    ``dpt_i = sqrt(sum_l (c_l (psi_il - psi_root,l))^2)``, divided by its maximum.  ``root`` is a row number or an entry
    of ``adata.obs_names``; 2 <= ``n_dcs`` <= the stored number of components.  Runs on the host (numpy).  Writes
    ``obs[key_added]`` (float64, 0 at the root, 1 at the farthest cell) and ``uns[key_added]`` = {``root``, ``n_dcs``,
    ``key``}."""
    _check_key("key", key)
    _check_key("key_added", key_added)
    if "X_" + key not in adata.obsm or key + "_evals" not in adata.uns:
        raise ValueError(f"no diffusion map is stored under key={key!r}: run diffusion_map(adata, key_added={key!r}) first")
    psi = np.asarray(adata.obsm["X_" + key], dtype=np.float64)
    lam = np.asarray(adata.uns[key + "_evals"], dtype=np.float64)
    n = int(adata.n_obs)
    if psi.ndim != 2 or psi.shape != (n, lam.size):
        raise ValueError(f"the stored map has shape {psi.shape} and {lam.size} eigenvalues for {n} cells")
    if not _is_int(n_dcs) or not 2 <= n_dcs <= lam.size:
        raise ValueError(f"n_dcs must be an integer in 2..{lam.size} (the stored components), got {n_dcs!r}")
    if _is_int(root):
        if not 0 <= root < n:
            raise ValueError(f"root={root} is not a row number in [0, {n})")
        row = int(root)
    elif isinstance(root, str):
        names = adata.obs_names
        if root not in names:
            raise ValueError(f"root={root!r} is neither a row number nor an entry of adata.obs_names")
        row = int(np.flatnonzero(np.asarray(names) == root)[0])
    else:
        raise ValueError(f"root must be a row number or an entry of adata.obs_names, got {root!r}")
    if not np.all(lam[1:n_dcs] < 1.0):
        raise ValueError("an eigenvalue beyond the first equals 1: the stored map is that of a disconnected graph")
    acc = np.zeros(n, dtype=np.float64)
    for l in range(1, int(n_dcs)):
        term = (lam[l] / (1.0 - lam[l])) * (psi[:, l] - psi[row, l])
        acc = acc + term * term
    dpt = np.sqrt(acc)
    top = dpt.max()
    if not top > 0:
        raise ValueError("every cell is at diffusion distance 0 from the root: the stored components are constant")
    adata = adata.copy() if copy else adata
    adata.obs[key_added] = dpt / top
    adata.uns[key_added] = {"root": row, "n_dcs": int(n_dcs), "key": key}
    update_metadata(adata, "diffusion_pseudotime", {"root": row, "n_dcs": int(n_dcs), "key": key, "key_added": key_added},
                    {"obs": key_added, "uns": key_added})
    return adata
