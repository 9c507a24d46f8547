"""fit_nmf / project_nmf: sklearn 1.7.2 ``NMF(solver="mu")`` on the device (sc_nmf_fit).

The host resolves the genes, hands the library a canonical CSR and replays what sklearn draws or fills before its
loop (``init="random"``: two ``RandomState.standard_normal`` blocks; ``transform``: a constant W); every iteration and
every error evaluation runs in HIP, in fp64 and in one documented summation order.  There is no CPU fallback."""

from __future__ import annotations

import numbers
from typing import Optional, Sequence, Union

import numpy as np

from spatialcore_amd import _lib
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata
from spatialcore_amd._sparse_input import canonical_csr, gene_columns

logger = get_logger("nmf")

LOSSES = ("frobenius", "kullback-leibler")
INITS = ("random", "custom")
K_MAX = 64
_SUPPORTED = ('beta_loss "frobenius" or "kullback-leibler", init "random" or "custom", the multiplicative-update solver, '
              "no regularisation")


def _check_common(beta_loss, max_iter, tol) -> None:
    if not isinstance(beta_loss, str) or beta_loss not in LOSSES:
        raise ValueError(f"beta_loss={beta_loss!r} is not supported; supported: {_SUPPORTED}")
    if not isinstance(max_iter, numbers.Integral) or isinstance(max_iter, bool) or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
    if not isinstance(tol, numbers.Real) or isinstance(tol, bool) or not np.isfinite(tol) or tol < 0:
        raise ValueError(f"tol must be a finite number >= 0, got {tol!r}")


def _check_sklearn_kwargs(kw: dict) -> None:
    """sklearn arguments this function does not take: their no-op values pass, anything else names what is supported."""
    noop = {"solver": ("mu",), "alpha_W": (0, 0.0), "alpha_H": (0, 0.0, "same"), "l1_ratio": None, "shuffle": None,
            "verbose": None}
    for name, value in kw.items():
        if name not in noop:
            raise TypeError(f"unexpected keyword argument {name!r}")
        if noop[name] is not None and not any(value is v or (type(value) is type(v) and value == v) for v in noop[name]):
            raise ValueError(f"{name}={value!r} is not supported; supported: {_SUPPORTED}")


def _check_components(n_components) -> int:
    if not isinstance(n_components, numbers.Integral) or isinstance(n_components, bool) or not 1 <= n_components <= K_MAX:
        raise ValueError(f"n_components must be an integer in 1..{K_MAX}, got {n_components!r}")
    return int(n_components)


def _matrix(adata, layer, cols: np.ndarray):
    """The layer (or ``adata.X``) restricted to ``cols`` as sc_nmf_fit takes it, and the dtype of the result."""
    X = adata.layers[layer] if layer is not None else adata.X
    Xc, dtype = canonical_csr(X, cols, len(adata.var_names), negative="Negative values in data passed to NMF (input X)",
                              all_zero="the expression matrix is all zero: there is nothing to factorise")
    if Xc.shape[0] > 2**31 - 1 or Xc.nnz > 2**32 - 1:
        raise ValueError("at most 2^31 - 1 cells and 2^32 - 1 stored entries are supported")
    return Xc, dtype


def _scale(Xc, K: int) -> float:
    """sklearn's ``sqrt(X.mean() / n_components)`` on the float64 CSR."""
    X64 = Xc if Xc.dtype == np.float64 else Xc.astype(np.float64)
    return float(np.sqrt(X64.mean() / K))


def _random_state(random_state) -> np.random.RandomState:
    if random_state is None:
        return np.random.mtrand._rand
    if isinstance(random_state, np.random.RandomState):
        return random_state
    if isinstance(random_state, numbers.Integral) and not isinstance(random_state, bool):
        return np.random.RandomState(int(random_state))
    raise ValueError(f"random_state must be None, an integer or a numpy RandomState, got {random_state!r}")


def random_init(avg: float, n: int, n_genes: int, K: int, random_state):
    """sklearn's ``init="random"`` (_initialize_nmf): H0 is drawn first, then W0, both ``|avg * standard_normal|``."""
    rs = _random_state(random_state)
    H0 = avg * rs.standard_normal(size=(K, n_genes))
    W0 = avg * rs.standard_normal(size=(n, K))
    np.abs(H0, out=H0)
    np.abs(W0, out=W0)
    return W0, H0


def _check_factor(A, shape, whom: str) -> np.ndarray:
    """sklearn's _check_init: shape, finite, non-negative, not all zero."""
    A = np.asarray(A)
    if A.dtype == object or not (np.issubdtype(A.dtype, np.number) or A.dtype == bool):
        raise ValueError(f"{whom} must be numeric")
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.shape != shape:
        raise ValueError(f"Array with wrong shape passed to NMF (input {whom}): expected {shape}, but got {A.shape}")
    if not np.all(np.isfinite(A)):
        raise ValueError(f"{whom} contains NaN or infinite values")
    if A.min() < 0:
        raise ValueError(f"Negative values in data passed to NMF (input {whom})")
    if A.max() == 0:
        raise ValueError(f"Array passed to NMF (input {whom}) is full of zeros")
    return A


def _store(adata, function: str, key_added: str, res: dict, H: np.ndarray, names, dtype, params: dict) -> None:
    max_iter, tol = params["max_iter"], params["tol"]
    converged = not (res["n_iter"] == max_iter and tol > 0)
    if not converged:
        logger.warning(f"Maximum number of iterations {max_iter} reached. Increase it to improve convergence.")
    adata.obsm["X_" + key_added] = res["W"].astype(dtype, copy=False)
    adata.uns[key_added] = {
        "components": H.astype(dtype, copy=False),
        "genes": list(names),
        "reconstruction_err": float(res["reconstruction_err"]),
        "n_iter": int(res["n_iter"]),
        "converged": bool(converged),
        "error_trace": res["error_trace"],
        "params": dict(params),
    }
    update_metadata(adata, function,
                    {**params, "genes": list(names[:10]) if len(names) > 10 else list(names), "n_genes": len(names),
                     "key_added": key_added},
                    {"obsm": "X_" + key_added, "uns": key_added})


def fit_nmf(adata, n_components: int, genes: Optional[Union[str, Sequence[str]]] = None, layer: Optional[str] = None,
            beta_loss: str = "frobenius", init: str = "random", max_iter: int = 200, tol: float = 1e-4, random_state=0,
            W=None, H=None, key_added: str = "nmf", copy: bool = False, device: int = 0, **sklearn_kwargs):
    """``sklearn.decomposition.NMF(n_components, init, solver="mu", beta_loss, max_iter, tol, random_state)
    .fit_transform`` of ``adata.X`` (or ``layers[layer]``) restricted to ``genes`` in the order given, on the GPU.

    The matrix may be scipy sparse of any format or dense, float32, float64 or an integer type; it must be finite,
    non-negative and not all zero.  ``beta_loss`` is ``"frobenius"`` or ``"kullback-leibler"``; the solver is always the
    multiplicative update; there is no regularisation.  **The default ``init`` differs from sklearn's**: sklearn's
    ``init=None`` means NNDSVDA, which is not implemented here -- the default is ``"random"`` (sklearn's
    ``init="random"`` with the same ``random_state``, draw for draw); ``"custom"`` starts from ``W`` (cells x K) and
    ``H`` (K x genes).  1 <= ``n_components`` <= 64.  Anything else sklearn accepts raises a ``ValueError``.

    Writes ``adata.obsm["X_" + key_added]`` (usages, cells x K; float32 for a float32 matrix -- the fp64 result rounded
    once -- else float64) and ``adata.uns[key_added]`` = {``components`` (K x genes), ``genes``, ``reconstruction_err``,
    ``n_iter``, ``converged`` (False where sklearn raises its ConvergenceWarning), ``error_trace``, ``params``}, and
    appends the usual entry to ``uns["spatialcore_metadata"]``.  The result is a function of the arguments alone, bit
    for bit."""
    K = _check_components(n_components)
    _check_common(beta_loss, max_iter, tol)
    _check_sklearn_kwargs(sklearn_kwargs)
    if not isinstance(init, str) or init not in INITS:
        raise ValueError(f"init={init!r} is not supported (sklearn's default init=None means NNDSVDA); supported: {_SUPPORTED}")
    if init == "custom" and (W is None or H is None):
        raise ValueError('init="custom" needs both W (cells x n_components) and H (n_components x genes)')
    if init != "custom" and (W is not None or H is not None):
        raise ValueError('W and H are only used with init="custom"')
    names, cols = gene_columns(adata, genes)
    Xc, dtype = _matrix(adata, layer, cols)
    n, G = Xc.shape
    if init == "custom":
        W0, H0 = _check_factor(W, (n, K), "W"), _check_factor(H, (K, G), "H")
    else:
        _random_state(random_state)   # its type, before anything is drawn
    logger.info(f"NMF ({beta_loss}, multiplicative update): {n:,} cells x {G} genes, {K} components")
    ctx = _lib.default_context(device)
    if init == "random":
        W0, H0 = random_init(_scale(Xc, K), n, G, K, random_state)
    res = ctx.nmf_fit(Xc.indptr, Xc.indices, Xc.data, G, W0, H0, beta_loss, True, int(max_iter), float(tol))
    adata = adata.copy() if copy else adata
    params = {"n_components": K, "beta_loss": beta_loss, "init": init, "solver": "mu", "max_iter": int(max_iter),
              "tol": float(tol), "random_state": random_state if isinstance(random_state, numbers.Integral) else None,
              "layer": layer}
    _store(adata, "fit_nmf", key_added, res, res["H"], names, dtype, params)
    return adata


def project_nmf(adata, components, genes: Sequence[str], layer: Optional[str] = None, beta_loss: str = "frobenius",
                max_iter: int = 200, tol: float = 1e-4, key_added: str = "nmf", copy: bool = False, device: int = 0):
    """``NMF.transform``: the usages of these cells under the fixed programs ``components`` (K x ``genes``), from
    sklearn's constant start ``sqrt(mean(X) / K)``.  Writes the keys of ``fit_nmf``; ``components`` are the ones given."""
    _check_common(beta_loss, max_iter, tol)
    C = np.asarray(components)
    if C.ndim != 2:
        raise ValueError(f"components must be 2-D (n_components x genes), got shape {C.shape}")
    K = _check_components(C.shape[0])
    if genes is None or isinstance(genes, str) and C.shape[1] != 1:
        raise ValueError("genes must name the columns of components")
    names, cols = gene_columns(adata, genes)
    H0 = _check_factor(C, (K, len(names)), "H")
    Xc, dtype = _matrix(adata, layer, cols)
    n, G = Xc.shape
    logger.info(f"NMF projection ({beta_loss}): {n:,} cells x {G} genes onto {K} components")
    ctx = _lib.default_context(device)
    W0 = np.full((n, K), _scale(Xc, K), dtype=np.float64)
    res = ctx.nmf_fit(Xc.indptr, Xc.indices, Xc.data, G, W0, H0, beta_loss, False, int(max_iter), float(tol))
    adata = adata.copy() if copy else adata
    params = {"n_components": K, "beta_loss": beta_loss, "init": "transform", "solver": "mu", "max_iter": int(max_iter),
              "tol": float(tol), "layer": layer}
    _store(adata, "project_nmf", key_added, res, H0, names, dtype, params)
    return adata
