"""umap: a deterministic two- or three-dimensional layout of the cells' neighbour graph.

The optimisation runs in HIP (sc_umap_layout), in fp64 and in one documented order; the host checks the arguments, fits the
curve parameters ``a`` and ``b`` and prepares the start positions.  There is no CPU fallback.

Two differences from umap-learn's ``optimize_layout_euclidean``, on purpose, so that the bytes of the result are a function
of the arguments alone: every epoch reads the positions of the PREVIOUS epoch (umap-learn's threads read positions other
threads are writing), and every firing entry gives its row's vertex one attraction and exactly ``negative_sample_rate``
repulsions -- the move umap-learn gives an edge's other end comes from the mirrored entry -- so the ratio per vertex is
1 : rate against umap-learn's 2 : rate.  Parity with umap-learn or scanpy is not claimed."""

from __future__ import annotations

import numbers
from typing import Optional

import numpy as np
from scipy import sparse

from spatialcore_amd import _lib
from spatialcore_amd._cell_graph import symmetric_graph
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata

logger = get_logger("embedding")

NEG_MAX = 16
EXTENT = 10.0            # the start positions are scaled to max |.| = 10, as umap-learn scales its spectral start
EPOCHS_SMALL, EPOCHS_LARGE, SMALL_BELOW = 500, 200, 10000


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _is_real(v) -> bool:
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and np.isfinite(v)


def find_ab_params(spread: float, min_dist: float):
    """umap-learn's ``find_ab_params``: least squares of ``1 / (1 + a x^(2b))`` to the curve that is 1 up to ``min_dist`` and
    ``exp(-(x - min_dist) / spread)`` beyond it, on ``linspace(0, 3 spread, 300)``."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def default_epochs(n: int) -> int:
    return EPOCHS_SMALL if n <= SMALL_BELOW else EPOCHS_LARGE


def _check_arguments(min_dist, spread, n_components, n_epochs, alpha, gamma, negative_sample_rate, seed, a, b, neighbors_key,
                     key_added, copy):
    if not _is_real(spread) or spread <= 0:
        raise ValueError(f"spread must be a finite number > 0, got {spread!r}")
    if not _is_real(min_dist) or not 0 <= min_dist < 3 * spread:
        raise ValueError(f"min_dist must be a finite number in [0, 3 spread), got {min_dist!r}")
    if not _is_int(n_components) or n_components not in (2, 3):
        raise ValueError(f"n_components must be 2 or 3, got {n_components!r}")
    if n_epochs is not None and (not _is_int(n_epochs) or not 1 <= n_epochs <= 2**31 - 1):
        raise ValueError(f"n_epochs must be None or an integer in 1..2^31 - 1, got {n_epochs!r}")
    if not _is_real(alpha) or alpha <= 0:
        raise ValueError(f"alpha must be a finite number > 0, got {alpha!r}")
    if not _is_real(gamma) or gamma < 0:
        raise ValueError(f"gamma must be a finite number >= 0, got {gamma!r}")
    if not _is_int(negative_sample_rate) or not 0 <= negative_sample_rate <= NEG_MAX:
        raise ValueError(f"negative_sample_rate must be an integer in 0..{NEG_MAX}, got {negative_sample_rate!r}")
    if not _is_int(seed) or not 0 <= seed < 2**64:
        raise ValueError(f"seed must be an integer in 0..2^64 - 1, got {seed!r}")
    if (a is None) != (b is None):
        raise ValueError("a and b must be given together or not at all")
    if a is not None and (not _is_real(a) or a <= 0 or not _is_real(b) or b <= 0):
        raise ValueError(f"a and b must be finite numbers > 0, got a={a!r}, b={b!r}")
    for name, value in (("neighbors_key", neighbors_key), ("key_added", key_added)):
        if value is not None and (not isinstance(value, str) or not value):
            raise ValueError(f"{name} must be None or a non-empty string, got {value!r}")
    if not isinstance(copy, (bool, np.bool_)):
        raise ValueError(f"copy must be True or False, got {copy!r}")


def _graph(adata, graph, neighbors_key, n: int) -> sparse.csr_matrix:
    if graph is None:
        key = neighbors_key or "neighbors"
        if key not in adata.uns or "connectivities_key" not in adata.uns[key]:
            raise KeyError(f"no neighbour graph in adata.uns[{key!r}]: run spatialcore_amd.neighbors.neighbors first "
                           f"(or pass graph=)")
        graph = adata.uns[key]["connectivities_key"]
        if graph not in adata.obsp:
            raise KeyError(f"adata.uns[{key!r}] names obsp[{graph!r}], which does not exist: run neighbors again")
    return symmetric_graph(adata, graph, n)


def _start(adata, init_pos, n: int, C: int, seed: int):
    """(positions (n, C) float64, what to record as ``init_pos``)."""
    if isinstance(init_pos, str) and init_pos == "random":
        return np.random.default_rng(seed).uniform(-EXTENT, EXTENT, size=(n, C)), "random"
    if isinstance(init_pos, str):
        if init_pos not in adata.obsm:
            raise ValueError(f"init_pos={init_pos!r} is neither \"random\" nor an entry of adata.obsm (available: {sorted(adata.obsm)})")
        Y, name, scale = adata.obsm[init_pos], init_pos, True
    else:
        Y, name, scale = init_pos, "<array>", False
    Y = Y.toarray() if sparse.issparse(Y) else np.asarray(getattr(Y, "values", Y))
    if Y.ndim != 2 or Y.shape[0] != n or Y.dtype == object or not (np.issubdtype(Y.dtype, np.number) or Y.dtype == bool) \
            or np.issubdtype(Y.dtype, np.complexfloating):
        raise ValueError(f"init_pos must be \"random\", an obsm key or a real array of shape ({n}, n_components), got shape "
                         f"{getattr(Y, 'shape', None)}")
    if Y.shape[1] < C or (not scale and Y.shape[1] != C):
        raise ValueError(f"init_pos has {Y.shape[1]} columns, n_components={C} needs "
                         f"{'at least ' if scale else ''}{C}")
    Y = np.array(Y[:, :C], dtype=np.float64, order="C", copy=True)
    if not np.all(np.isfinite(Y)):
        raise ValueError("init_pos contains NaN or infinite values")
    if scale:
        top = float(np.abs(Y).max()) if Y.size else 0.0
        if top > 0:
            Y = Y * (EXTENT / top)
    return Y, name


def umap(adata, *, min_dist: float = 0.5, spread: float = 1.0, n_components: int = 2, n_epochs: Optional[int] = None,
         alpha: float = 1.0, gamma: float = 1.0, negative_sample_rate: int = 5, init_pos="X_pca", seed: int = 0,
         a: Optional[float] = None, b: Optional[float] = None, neighbors_key: Optional[str] = None, graph=None,
         key_added: Optional[str] = None, copy: bool = False, device: int = 0):
    """Embed the cells' neighbour graph in ``n_components`` (2 or 3) dimensions on the GPU (scanpy's ``tl.umap``).

    The graph is ``obsp[uns[neighbors_key or "neighbors"]["connectivities_key"]]`` as ``neighbors`` writes it (either
    ``method``), or ``graph=``: an ``obsp`` key or a scipy sparse matrix, cells x cells, finite, positive, symmetric in
    structure and value.  A missing graph is a ``KeyError``.  ``a`` and ``b`` come from umap-learn's ``find_ab_params`` for
    (``spread``, ``min_dist``) unless both are given.  ``n_epochs=None`` is 500 up to 10,000 cells, else 200.  ``init_pos``
    is an ``obsm`` key (its first ``n_components`` columns scaled to ``max |.| = 10``, no noise added), ``"random"``
    (``default_rng(seed).uniform(-10, 10)``) or an ``(n, n_components)`` array taken as it is.  ``alpha`` is the initial
    learning rate, ``gamma`` the repulsion strength, ``negative_sample_rate`` (0..16) the negatives per firing entry, drawn
    by Philox4x32-10 from ``seed``.

    Stored entry t with weight ``w_t`` fires in epoch e iff ``floor((e + 1) w_t / w_max) > floor(e w_t / w_max)`` (umap's
    ``epochs_per_sample`` schedule; weights below ``w_max / n_epochs`` never fire).  Every vertex computes its new position
    from the previous epoch's positions: its firing entries in stored order, each one attraction and
    ``negative_sample_rate`` repulsions (include/spatialcore_hip.h has the exact expressions).  Unlike umap-learn, reads
    come from the previous epoch only and the ratio of attractions to repulsions per vertex is 1 : rate, not 2 : rate;
    parity with umap-learn is not claimed.  The result is a function of the arguments alone, bit for bit.

    Writes ``obsm["X_umap"]`` (float64) and ``uns["umap"]`` = {``params``: ``a``, ``b``, ``min_dist``, ``spread``,
    ``n_epochs``, ``alpha``, ``gamma``, ``negative_sample_rate``, ``seed``, ``init_pos``, ``n_components``,
    ``neighbors_key``}; with ``key_added="x"`` the keys are ``obsm["x"]`` and ``uns["x"]``.  Appends the usual entry to
    ``uns["spatialcore_metadata"]``."""
    _check_arguments(min_dist, spread, n_components, n_epochs, alpha, gamma, negative_sample_rate, seed, a, b, neighbors_key,
                     key_added, copy)
    n = int(adata.n_obs)
    if not 1 <= n <= 2**31 - 1:
        raise ValueError(f"umap needs 1 <= cells <= 2^31 - 1, got {n}")
    C = int(n_components)
    A = _graph(adata, graph, neighbors_key, n)
    Y0, init_name = _start(adata, init_pos, n, C, int(seed))
    if a is None:
        a, b = find_ab_params(float(spread), float(min_dist))
    epochs = default_epochs(n) if n_epochs is None else int(n_epochs)

    ctx = _lib.default_context(device)
    logger.info(f"umap: {n:,} cells, {A.nnz:,} stored entries, {epochs} epochs, a={a:.5f}, b={b:.5f}")
    Y = ctx.umap_layout((A.indptr, A.indices, A.data), Y0, a, b, gamma, alpha, int(negative_sample_rate), epochs, int(seed))

    adata = adata.copy() if copy else adata
    obsm_key = "X_umap" if key_added is None else key_added
    uns_key = "umap" if key_added is None else key_added
    params = {"a": float(a), "b": float(b), "min_dist": float(min_dist), "spread": float(spread), "n_epochs": epochs,
              "alpha": float(alpha), "gamma": float(gamma), "negative_sample_rate": int(negative_sample_rate), "seed": int(seed),
              "init_pos": init_name, "n_components": C, "neighbors_key": neighbors_key}
    adata.obsm[obsm_key] = Y
    adata.uns[uns_key] = {"params": params}
    source = graph if isinstance(graph, str) else ("<matrix>" if graph is not None else None)
    update_metadata(adata, "umap", {**params, "graph": source, "key_added": key_added}, {"obsm": obsm_key, "uns": uns_key})
    return adata
