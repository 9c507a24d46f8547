"""Neighbourhood composition profiles on MI355X.

Drop-in mirror of the reference's ``compute_neighborhood_profile``
(reference src/spatialcore/spatial/neighborhoods.py:48-296, ``NB`` below): same keywords, defaults,
outputs (``adata.obsm[key_added]`` float32, ``adata.uns[key_added + '_celltypes']``), and errors.
Neighbour search (exact kNN or closed-ball radius) and the per-cell label counting run in HIP
kernels.  ``identify_niches`` (NB:299-522) clusters the profiles with sklearn's k-means (k-means++ seeding, Lloyd
iterations, best of ``n_init`` runs) replayed step for step in HIP (``sc_kmeans_fit``).
``neighborhood_enrichment``, ``ripley_k`` and ``co_occurrence`` are extensions: the three cell-type pattern statistics
squidpy users run on an annotated section, as exact integer pair counts; ``ripley_g`` is the
nearest-neighbour counterpart of ``ripley_k``, a minimum per cell where those are sums over pairs.  ``ligrec`` is the
fourth extension under squidpy's name: the ligand-receptor permutation test over cluster pairs, expression summed by
permuted label as exact integers.
"""

from __future__ import annotations

import warnings
from typing import Optional

import numpy as np
import pandas as pd

from spatialcore_amd import _lib
from spatialcore_amd._kmeans_draws import kmeans_draws      # its name stays importable from here
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata

logger = get_logger("spatial.neighborhoods")


class ConvergenceWarning(UserWarning):
    """Raised as sklearn's ``ConvergenceWarning`` (same text) when k-means finds fewer distinct clusters than asked."""


def _request_problem(adata, celltype_column, method, k, radius, spatial_key) -> Optional[str]:
    """The first thing wrong with a request, as the reference words it (NB:146-179), else None."""
    if spatial_key not in adata.obsm:
        return (f"adata.obsm['{spatial_key}'] not found. "
                "Spatial coordinates are required for neighborhood computation.")
    if celltype_column not in adata.obs.columns:
        return (f"Column '{celltype_column}' not found in adata.obs. "
                f"Available columns: {list(adata.obs.columns)[:10]}...")
    per_method = {
        "knn": lambda: (f"k must be >= 1, got {k}" if k < 1 else
                        f"k must be < number of cells ({adata.n_obs}), got {k}" if k >= adata.n_obs else None),
        "radius": lambda: ("'radius' must be provided when method='radius'." if radius is None else
                           f"radius must be > 0, got {radius}" if radius <= 0 else None),
    }
    if method not in per_method:
        return f"Invalid method: '{method}'. Must be 'knn' or 'radius'."
    return per_method[method]()


def _label_codes(adata, celltype_column: str):
    """Sorted unique labels (NB:196) and the int32 code of every cell; missing labels are an error (NB:186-192)."""
    labels = adata.obs[celltype_column]
    n_missing = int(labels.isna().sum())
    if n_missing:
        raise ValueError(f"{n_missing} cells have missing labels in '{celltype_column}'. "
                         "Fill or remove missing labels before computing neighborhoods.")
    codes, kinds = pd.factorize(np.asarray(labels.values, dtype=object), sort=True)
    return list(kinds), codes.astype(np.int32)


def _category_codes(adata, column: str):
    """The categories of a categorical column (unused ones kept), else ``_label_codes``' sorted unique labels, and the
    int32 code of every cell."""
    labels = adata.obs[column]
    if isinstance(labels.dtype, pd.CategoricalDtype):
        return list(labels.cat.categories), np.asarray(labels.cat.codes, dtype=np.int32)
    return _label_codes(adata, column)


def _point_pattern_request_problem(adata, column, spatial_key, what) -> Optional[str]:
    """What ``ripley_k`` and ``co_occurrence`` (``what``) check first: the spatial key, the column, 2-D coordinates."""
    if spatial_key not in adata.obsm:
        return (f"adata.obsm['{spatial_key}'] not found. "
                f"Spatial coordinates are required for {what}.")
    if column not in adata.obs.columns:
        return (f"Column '{column}' not found in adata.obs. "
                f"Available columns: {list(adata.obs.columns)[:10]}...")
    shape = np.shape(adata.obsm[spatial_key])
    if len(shape) != 2 or shape[1] != 2:
        return ("only 2-D coordinates are supported by the MI355X path "
                f"(adata.obsm['{spatial_key}'] has shape {tuple(shape)})")
    return None


def _rng_problem(rng) -> Optional[str]:
    return None if rng in ("numpy", "philox") else f"rng must be 'numpy' or 'philox', got '{rng}'"


def _coordinates(adata, spatial_key: str) -> np.ndarray:
    xy = np.asarray(adata.obsm[spatial_key])
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("only 2-D coordinates are supported by the MI355X path "
                         f"(adata.obsm['{spatial_key}'] has shape {xy.shape})")
    return np.ascontiguousarray(xy, dtype=np.float64)


def _activate_neighbour_graph(ctx, coords: np.ndarray, method: str, k: int, radius) -> None:
    """Exact kNN (NB:213-228) or closed-ball radius lists (NB:241-251) as the context's unweighted graph."""
    if method == "knn":
        logger.debug(f"Querying {k} nearest neighbors per cell")
        ctx.knn(coords, k, fetch=False)
        ctx.graph_from_knn(1.0)
    else:
        logger.debug(f"Querying neighbors within radius={radius}")
        indptr, indices = ctx.radius_graph(coords, float(radius))
        ctx.set_graph_csr(indptr, indices, np.ones(indices.size), coords.shape[0])


def _label_permutation_null(ctx, n_cells: int, n_permutations: int, seed: int, perm_batch: int, rng: str, comm,
                            resident, counter):
    """The null of a label-permutation test over this rank's share of the ``n_permutations`` permutations:
    ``(observed, sums)``.  ``resident(rows)`` -> ``(observed, sums)`` over the first ``rows`` rows of the resident
    permutation table (``rng="numpy"``: the stream ``default_rng(seed).permutation(n_cells)``, generated ``perm_batch``
    rows at a time and continued batch after batch; one pass with ``rows = 0`` still runs when there is nothing to
    permute, for the observed tables).  ``counter(lo, n)`` -> the same over the counter-based permutations
    lo .. lo + n - 1 (``rng="philox"``), one call for the whole range.  ``sums`` is an int64 array, exact and order-free:
    batches add theirs, and the permutation shards of the ranks of ``comm`` merge with one integer all-reduce;
    ``observed`` is whatever the last call gave."""
    lo, hi = 0, n_permutations
    if comm is not None and comm.world > 1:
        from spatialcore_amd.parallel import shard_bounds

        lo, hi = shard_bounds(n_permutations, comm.world, comm.rank)
    if rng == "philox":
        observed, sums = counter(lo, hi - lo)
    else:
        words = _lib.rng_state_words(np.random.default_rng(seed))
        sums, done = 0, lo
        while True:
            batch = min(perm_batch, hi - done)
            if batch > 0:
                ctx.generate_permutations(words, n_cells, batch)   # one stream, continued batch after batch
            observed, part = resident(batch)
            sums = sums + part
            done += batch
            if done >= hi:
                break
    if comm is not None and comm.world > 1:
        sums = comm.sum_over_ranks_i64(sums)     # the one collective of this path
    return observed, sums


def _pair_count_null(ctx, counts, counter, codes, n_types: int, n_sums: int, n_permutations: int, seed: int,
                     perm_batch: int, rng: str, comm):
    """``_label_permutation_null`` of ``neighborhood_enrichment``, ``ripley_k`` and ``ripley_g``: the observed table and the integer
    sums of the null: sum of (null - observed), sum of (null - observed)^2, #{null >= observed} and, with
    ``n_sums = 4``, #{null <= observed}.  ``counts(codes, T, rows)``: the tables of the resident permutation rows, then
    the observed one; ``counter(codes, T, seed, lo, n, batch)``: the observed table and the sums, from one device call
    (generation of batch b + 1 beside the counting of batch b, integer sums accumulated on the device)."""
    def resident(rows):
        cnt = counts(codes, n_types, rows)
        observed = cnt[rows]
        dev = cnt[:rows] - observed
        sums = [dev.sum(axis=0), (dev * dev).sum(axis=0), (dev >= 0).sum(axis=0)]
        if n_sums > 3:
            sums.append((dev <= 0).sum(axis=0))
        return observed, np.stack(sums)

    return _label_permutation_null(ctx, codes.size, n_permutations, seed, perm_batch, rng, comm, resident,
                                   lambda lo, n: counter(codes, n_types, seed, lo, n, perm_batch))


def _permgen_form(ctx, n_cells: int, rng: str, n_permutations: int) -> Optional[str]:
    """The ``permgen_form`` provenance entry of a call that draws label permutations."""
    if n_permutations <= 0:
        return None
    return ctx.permgen_form(n_cells) if rng == "numpy" else "counter-based (philox)"


def _null_statistics(count, sums, n_permutations: int) -> dict:
    """``mean``, ``std`` (population), ``zscore = (count - mean) / std`` and ``p_value = (#{>=} + 1) / (P + 1)`` from the
    integer sums of ``_pair_count_null`` over P = ``n_permutations`` > 0 null tables, and
    ``p_value_less = (#{<=} + 1) / (P + 1)`` when the sums have that fourth row."""
    s1, s2, ge, *le = (np.asarray(x, dtype=np.int64) for x in sums)
    mean_dev = s1 / n_permutations
    std = np.sqrt(np.maximum(s2 / n_permutations - mean_dev * mean_dev, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = -mean_dev / std
    out = {"mean": count + mean_dev, "std": std, "zscore": z, "p_value": (ge + 1) / (n_permutations + 1)}
    if le:
        out["p_value_less"] = (le[0] + 1) / (n_permutations + 1)
    return out


def compute_neighborhood_profile(
    adata,
    celltype_column: str,
    method: str = "knn",
    k: int = 15,
    radius: Optional[float] = None,
    normalize: bool = True,
    spatial_key: str = "spatial",
    key_added: str = "neighborhood_profile",
    copy: bool = False,
    *,
    device: int = 0,
):
    """Cell-type composition of every cell's spatial neighbourhood (NB:48-296)."""
    problem = _request_problem(adata, celltype_column, method, k, radius, spatial_key)
    if problem:
        raise ValueError(problem)
    if copy:
        adata = adata.copy()
    n_cells = adata.n_obs
    unique_celltypes, codes = _label_codes(adata, celltype_column)
    n_celltypes = len(unique_celltypes)
    if n_celltypes < 2:
        raise ValueError(f"At least 2 unique cell types required, found {n_celltypes}. "
                         f"Check column '{celltype_column}'.")
    coords = _coordinates(adata, spatial_key)
    logger.info(f"Computing neighborhood profiles: {n_cells:,} cells, {n_celltypes} cell types, method={method}")

    ctx = _lib.default_context(device)
    _activate_neighbour_graph(ctx, coords, method, k, radius)
    try:
        neighborhood_profile = ctx.profile_counts(codes, n_celltypes)
    except ValueError as e:
        if "empty neighborhood profiles" not in str(e):
            raise
        n_empty = int(str(e).split()[0])
        raise ValueError(f"{n_empty} cells have empty neighborhood profiles. "
                         "Increase radius, switch to knn, or pre-filter isolated cells before profiling.") from None

    if normalize:
        row_sums = neighborhood_profile.sum(axis=1)
        neighborhood_profile = neighborhood_profile / row_sums[:, None]
        logger.debug("Normalized profiles to proportions")

    adata.obsm[key_added] = neighborhood_profile
    adata.uns[f"{key_added}_celltypes"] = list(unique_celltypes)
    logger.info(f"Stored neighborhood profiles in adata.obsm['{key_added}'] (shape: {neighborhood_profile.shape})")

    update_metadata(
        adata,
        function_name="compute_neighborhood_profile",
        parameters={
            "celltype_column": celltype_column,
            "method": method,
            "k": k if method == "knn" else None,
            "radius": radius if method == "radius" else None,
            "normalize": normalize,
            "spatial_key": spatial_key,
        },
        outputs={"obsm": key_added, "uns": f"{key_added}_celltypes",
                 "n_celltypes": n_celltypes, "n_cells": n_cells},
    )
    return adata


def neighborhood_enrichment(
    adata,
    celltype_column: str,
    method: str = "knn",
    k: int = 15,
    radius: Optional[float] = None,
    n_permutations: int = 1000,
    seed: int = 0,
    spatial_key: str = "spatial",
    key_added: str = "neighborhood_enrichment",
    copy: bool = False,
    *,
    device: int = 0,
    perm_batch: int = 512,
    rng: str = "numpy",
    comm=None,
):
    """Cell-type pair enrichment of the neighbourhood graph under label permutations.

    EXTENSION -- the reference has no such function (its ``neighborhoods.py`` stops at
    composition profiles and k-means niches); BASELINE.json's config 5 asks for it.  Semantics
    defined here: on the same neighbour graph ``compute_neighborhood_profile`` uses,
    ``count[a, b]`` = number of edges cell -> neighbour with types (a, b); the null is drawn by
    permuting the label vector (``labels[perm]``) ``n_permutations`` times.  Stored in
    ``adata.uns[key_added]``: ``count``, ``mean``, ``std`` (population), ``zscore = (count - mean) / std``,
    ``p_value = (#{perm count >= count} + 1) / (P + 1)`` as (T, T) arrays and ``celltypes``.

    ``rng``: ``"numpy"`` (default) -- the numpy-exact stream ``default_rng(seed).permutation(n_cells)``, sequential by
    nature: one GPU, generator-bound.  ``"philox"`` -- counter-based permutations (permutation p is a pure function of
    ``(seed, p)``: Fisher-Yates with Philox4x32-10 + Lemire draws, ``sc_perm_generate_counter``); there is no reference
    result to be seed-exact to here, and this source has no sequential stage.  With ``rng="philox"`` and ``comm`` (a
    communicator from ``spatialcore_amd.parallel.connect``) the permutations are SHARDED over the ranks of the launch
    (rank r takes ``shard_bounds(P, world, r)``) and the integer sums are merged with one all-reduce: every rank ends
    with the same table, identical to a one-rank run.
    """
    problem = _request_problem(adata, celltype_column, method, k, radius, spatial_key)
    if problem:
        raise ValueError(problem)
    if n_permutations < 0:
        raise ValueError(f"n_permutations must be >= 0, got {n_permutations}")
    if _rng_problem(rng):
        raise ValueError(_rng_problem(rng))
    if comm is not None and comm.world > 1 and rng != "philox":
        raise ValueError("permutations can only be sharded over ranks with rng='philox': the numpy stream is sequential")
    if copy:
        adata = adata.copy()
    n_cells = adata.n_obs
    celltypes, codes = _label_codes(adata, celltype_column)
    coords = _coordinates(adata, spatial_key)
    T = len(celltypes)
    logger.info(f"Computing neighborhood enrichment: {n_cells:,} cells, {T} cell types, method={method}, "
                f"permutations={n_permutations}")

    ctx = _lib.default_context(device)
    _activate_neighbour_graph(ctx, coords, method, k, radius)

    observed, sums = _pair_count_null(ctx, ctx.enrichment_counts, ctx.enrichment_counter, codes, T, 3, n_permutations, seed,
                                      perm_batch, rng, comm)
    result = {"count": observed, "celltypes": list(celltypes), "n_permutations": n_permutations, "seed": seed, "rng": rng}
    if n_permutations > 0:
        result.update(_null_statistics(observed, sums, n_permutations))
    adata.uns[key_added] = result
    update_metadata(
        adata,
        function_name="neighborhood_enrichment",
        parameters={"celltype_column": celltype_column, "method": method, "k": k if method == "knn" else None,
                    "radius": radius if method == "radius" else None, "n_permutations": n_permutations,
                    "seed": seed, "spatial_key": spatial_key, "rng": rng,
                    "permgen_form": _permgen_form(ctx, n_cells, rng, n_permutations)},
        outputs={"uns": key_added, "n_celltypes": T, "n_cells": n_cells},
    )
    return adata


def _ripley_request_problem(adata, celltype_column, radii, n_permutations, area, spatial_key, rng, comm,
                            what: str = "Ripley's K") -> Optional[str]:
    """The first thing wrong with a ``ripley_k`` or ``ripley_g`` (``what``) request (checked before any device work),
    else None."""
    problem = _point_pattern_request_problem(adata, celltype_column, spatial_key, what)
    if problem:
        return problem
    try:
        r = np.asarray(radii, dtype=np.float64)
    except (TypeError, ValueError):
        return f"radii must be a 1-D sequence of numbers, got {radii!r}"
    if r.ndim != 1:
        return f"radii must be 1-D, got shape {r.shape}"
    if r.size == 0:
        return "radii must not be empty"
    if r.size > 32:
        return f"at most 32 radii are supported, got {r.size}"
    if not np.all(np.isfinite(r)):
        return f"radii must be finite, got {r[~np.isfinite(r)][0]}"
    if np.any(r <= 0):
        return f"radii must be > 0, got {r[r <= 0][0]}"
    if np.any(np.diff(r) <= 0):
        j = int(np.argmax(np.diff(r) <= 0))
        return f"radii must be strictly increasing, got {r[j + 1]} after {r[j]}"
    if not np.all(np.isfinite(r * r)):
        return f"radii must have a finite square, got {r[-1]}"
    if n_permutations < 0:
        return f"n_permutations must be >= 0, got {n_permutations}"
    if _rng_problem(rng):
        return _rng_problem(rng)
    if comm is not None and rng != "philox":
        return "permutations can only be sharded over ranks (comm=) with rng='philox': the numpy stream is sequential"
    if area is not None and not (np.isfinite(area) and area > 0):
        return f"area must be > 0, got {area}"
    return None


def ripley_statistics(count, n_per_type, area: float, sums=None, n_permutations: int = 0) -> dict:
    """K, L and the permutation statistics from the integer tables alone (pure host arithmetic, no device).

    ``count``: (T, T, R) cumulative ordered pair counts; ``n_per_type``: (T,) cells per type.
    ``K[a, b, j] = area * count[a, b, j] / (n_a n_b)`` for a != b and ``/ (n_a (n_a - 1))`` for a = b, NaN where that
    denominator is 0; ``L = sqrt(K / pi)``.  ``sums``: (4, T, T, R) integers over the ``n_permutations`` null tables --
    sum of (null - count), sum of (null - count)^2, #{null >= count}, #{null <= count} -- giving ``mean``, ``std``
    (population), ``zscore = (count - mean) / std``, ``p_value = (#{>=} + 1) / (P + 1)`` and
    ``p_value_less = (#{<=} + 1) / (P + 1)``.
    """
    count = np.asarray(count, dtype=np.int64)
    n_t = np.asarray(n_per_type, dtype=np.int64)
    denom = (n_t[:, None] * n_t[None, :]).astype(np.float64)
    denom[np.diag_indices(n_t.size)] = (n_t * (n_t - 1)).astype(np.float64)
    denom = np.where(denom > 0, denom, np.nan)
    K = float(area) * count / denom[:, :, None]
    out = {"K": K, "L": np.sqrt(K / np.pi)}
    if n_permutations > 0:
        out.update(_null_statistics(count, sums, n_permutations))
    return out


def ripley_k(
    adata,
    celltype_column: str,
    radii,
    n_permutations: int = 0,
    seed: int = 0,
    area: Optional[float] = None,
    spatial_key: str = "spatial",
    key_added: str = "ripley_k",
    copy: bool = False,
    *,
    device: int = 0,
    perm_batch: int = 512,
    rng: str = "numpy",
    comm=None,
):
    """Cross-type Ripley's K function at several radii, with a label-permutation null.

    EXTENSION -- the reference has no point-pattern statistic; its documentation sends users to Ripley's K where
    Moran's I breaks down (sparse markers: pass a boolean column, two types).  Semantics defined here
    (include/spatialcore_hip.h, N6): for radii ``r_1 < ... < r_R`` (at most 32),
    ``count[a, b, j]`` = number of ORDERED pairs of distinct cells (i, i') of types (a, b) with squared distance
    ``fl(fl(dx dx) + fl(dy dy)) <= fl(r_j r_j)`` (fp64, the closed ball of the radius graph), cumulative in j.  So
    ``count[:, :, j].sum()`` is the nnz of the radius graph at ``r_j``, ``count[:, :, j]`` equals
    ``neighborhood_enrichment(method="radius", radius=r_j)["count"]`` and the table is symmetric in (a, b).
    ``K[a, b, j] = area * count / (n_a n_b)`` (``n_a (n_a - 1)`` on the diagonal; NaN where that is 0),
    ``L = sqrt(K / pi)``; ``area`` defaults to the bounding box of all cells.  NO EDGE CORRECTION is applied: it
    cancels in the permutation null, which is the inference this function offers.

    Null: the label vector permuted ``n_permutations`` times exactly as ``neighborhood_enrichment`` does it
    (``rng="numpy"``: ``default_rng(seed).permutation(n)`` continued across batches; ``rng="philox"``: counter-based,
    and with ``comm`` sharded over the ranks and merged by one integer all-reduce).  Stored in ``adata.uns[key_added]``:
    ``radii``, ``celltypes``, ``n_per_type``, ``area``, ``count`` (T, T, R int64), ``K``, ``L`` and, with permutations,
    ``mean``, ``std`` (population), ``zscore``, ``p_value = (#{null >= count} + 1) / (P + 1)``,
    ``p_value_less = (#{null <= count} + 1) / (P + 1)``, plus ``n_permutations``, ``seed``, ``rng``.

    All R radii come from ONE pass over the pairs within ``r_R`` (each tagged with the smallest radius containing it)
    per batch of permutations; the pair list is built on the device and never visits the host.
    """
    problem = _ripley_request_problem(adata, celltype_column, radii, n_permutations, area, spatial_key, rng, comm)
    if problem:
        raise ValueError(problem)
    if copy:
        adata = adata.copy()
    n_cells = adata.n_obs
    celltypes, codes = _label_codes(adata, celltype_column)
    coords = _coordinates(adata, spatial_key)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    T, R = len(celltypes), radii.size
    if area is None:
        ext = coords.max(axis=0) - coords.min(axis=0) if n_cells else np.zeros(2)
        area = float(ext[0] * ext[1])
        if not area > 0:
            raise ValueError(f"the bounding box of the cells has area {area}; pass area= explicitly")
    logger.info(f"Computing Ripley's K: {n_cells:,} cells, {T} cell types, {R} radii up to {radii[-1]:g}, "
                f"permutations={n_permutations}")

    ctx = _lib.default_context(device)
    n_pairs = ctx.ripley_build(coords, radii)
    logger.debug(f"{n_pairs:,} ordered pairs within r={radii[-1]:g}")

    observed, sums = _pair_count_null(ctx, ctx.ripley_counts, ctx.ripley_counter, codes, T, 4, n_permutations, seed,
                                      perm_batch, rng, comm)
    n_per_type = np.bincount(codes, minlength=T).astype(np.int64)
    result = {"radii": radii, "celltypes": list(celltypes), "n_per_type": n_per_type, "area": float(area), "count": observed}
    result.update(ripley_statistics(observed, n_per_type, area, sums, n_permutations))
    result.update({"n_permutations": n_permutations, "seed": seed, "rng": rng})
    adata.uns[key_added] = result
    update_metadata(
        adata,
        function_name="ripley_k",
        parameters={"celltype_column": celltype_column, "radii": [float(r) for r in radii], "n_permutations": n_permutations,
                    "seed": seed, "area": float(area), "spatial_key": spatial_key, "rng": rng,
                    "permgen_form": _permgen_form(ctx, n_cells, rng, n_permutations)},
        outputs={"uns": key_added, "n_celltypes": T, "n_cells": n_cells, "n_radii": R, "n_pairs": n_pairs},
    )
    return adata


def ripley_g_statistics(count, n_per_type, area: float, sums=None, n_permutations: int = 0, *, radii=None) -> dict:
    """G, its Poisson curve and the permutation statistics from the integer tables alone (pure host arithmetic, no device).

    ``count``: (T, T, R) cumulative counts of the cells of type a with at least one other cell of type b within ``r_j``;
    ``n_per_type``: (T,) cells per type.  ``G[a, b, j] = count[a, b, j] / n_a``, NaN where ``n_a = 0``.  With ``radii``
    (the R radii), ``G_poisson[a, b, j] = 1 - exp(-lambda pi r_j^2)`` with ``lambda = n_b / area``, and
    ``(n_a - 1) / area`` on the diagonal (a cell is not its own neighbour): the curve of complete spatial randomness at
    the types' densities, for plotting only -- the inference is the permutation null.  ``sums``: (4, T, T, R) integers
    over the ``n_permutations`` null tables -- sum of (null - count), sum of (null - count)^2, #{null >= count},
    #{null <= count} -- giving ``mean``, ``std`` (population), ``zscore = (count - mean) / std``,
    ``p_value = (#{>=} + 1) / (P + 1)`` (attraction: b nearer to a than under random labelling) and
    ``p_value_less = (#{<=} + 1) / (P + 1)``.
    """
    count = np.asarray(count, dtype=np.int64)
    n_t = np.asarray(n_per_type, dtype=np.int64)
    n_a = np.where(n_t > 0, n_t, 1).astype(np.float64)
    out = {"G": np.where((n_t > 0)[:, None, None], count / n_a[:, None, None], np.nan)}
    if radii is not None:
        r = np.asarray(radii, dtype=np.float64)
        others = np.broadcast_to(n_t[None, :], (n_t.size, n_t.size)).astype(np.float64)   # [a, b] = n_b ...
        others[np.diag_indices(n_t.size)] = np.maximum(n_t - 1, 0)                          # ... and n_a - 1 for b = a
        out["G_poisson"] = 1.0 - np.exp(-(others / float(area))[:, :, None] * (np.pi * r * r)[None, None, :])
    if n_permutations > 0:
        out.update(_null_statistics(count, sums, n_permutations))
    return out


def ripley_g(
    adata,
    celltype_column: str,
    radii,
    n_permutations: int = 0,
    seed: int = 0,
    area: Optional[float] = None,
    spatial_key: str = "spatial",
    key_added: str = "ripley_g",
    copy: bool = False,
    *,
    device: int = 0,
    perm_batch: int = 512,
    rng: str = "numpy",
    comm=None,
):
    """Cross-type nearest-neighbour distance distribution G at several radii, with a label-permutation null.

    EXTENSION -- spatstat's ``Gcross``, squidpy's ``ripley(mode="G")``: how far is a cell of type a from its nearest
    cell of type b, and is that nearer or farther than random labelling would give?  ``ripley_k`` and this function are
    read together: K is a sum over pairs and is dominated by dense clumps, G is a minimum per cell and speaks for the
    typical cell.  Semantics defined here (include/spatialcore_hip.h, N11): for radii ``r_1 < ... < r_R`` (at most 32),
    ``count[a, b, j]`` = number of cells i of type a with at least one OTHER cell i' of type b at squared distance
    ``fl(fl(dx dx) + fl(dy dy)) <= fl(r_j r_j)`` (fp64, the closed ball of the radius graph and of ``ripley_k``; "other"
    is decided by index, so a coincident cell counts).  The table is cumulative in j, ``count[a, b, j] <= n_a`` and NOT
    symmetric in (a, b).  ``G[a, b, j] = count / n_a`` (NaN where ``n_a = 0``); ``G_poisson`` is the curve of complete
    spatial randomness at the types' densities (``ripley_g_statistics``), for plotting; ``area`` defaults to the
    bounding box of all cells and enters ``G_poisson`` only.  NO EDGE CORRECTION is applied: it cancels in the
    permutation null, which is the inference this function offers.

    Null: the label vector permuted ``n_permutations`` times exactly as ``ripley_k`` does it (``rng="numpy"``:
    ``default_rng(seed).permutation(n)`` continued across batches; ``rng="philox"``: counter-based, and with ``comm``
    sharded over the ranks and merged by one integer all-reduce).  Stored in ``adata.uns[key_added]``: ``radii``,
    ``celltypes``, ``n_per_type``, ``area``, ``count`` (T, T, R int64), ``G``, ``G_poisson`` and, with permutations,
    ``mean``, ``std`` (population), ``zscore``, ``p_value = (#{null >= count} + 1) / (P + 1)`` (attraction),
    ``p_value_less = (#{null <= count} + 1) / (P + 1)``, plus ``n_permutations``, ``seed``, ``rng``.

    The ordered neighbour lists within ``r_R`` are built on the device once and never visit the host; every batch of
    permutations is one pass over them.  Envelope: at most 64 cell types and ``T * T * R <= 16384``.
    """
    problem = _ripley_request_problem(adata, celltype_column, radii, n_permutations, area, spatial_key, rng, comm,
                                      "Ripley's G")
    if problem:
        raise ValueError(problem)
    if copy:
        adata = adata.copy()
    n_cells = adata.n_obs
    celltypes, codes = _label_codes(adata, celltype_column)
    coords = _coordinates(adata, spatial_key)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    T, R = len(celltypes), radii.size
    if area is None:
        ext = coords.max(axis=0) - coords.min(axis=0) if n_cells else np.zeros(2)
        area = float(ext[0] * ext[1])
        if not area > 0:
            raise ValueError(f"the bounding box of the cells has area {area}; pass area= explicitly")
    logger.info(f"Computing Ripley's G: {n_cells:,} cells, {T} cell types, {R} radii up to {radii[-1]:g}, "
                f"permutations={n_permutations}")

    ctx = _lib.default_context(device)
    n_entries = ctx.ripley_g_build(coords, radii)
    logger.debug(f"{n_entries:,} list entries (ordered pairs) within r={radii[-1]:g}")

    observed, sums = _pair_count_null(ctx, ctx.ripley_g_counts, ctx.ripley_g_counter, codes, T, 4, n_permutations, seed,
                                      perm_batch, rng, comm)
    n_per_type = np.bincount(codes, minlength=T).astype(np.int64)
    result = {"radii": radii, "celltypes": list(celltypes), "n_per_type": n_per_type, "area": float(area), "count": observed}
    result.update(ripley_g_statistics(observed, n_per_type, area, sums, n_permutations, radii=radii))
    result.update({"n_permutations": n_permutations, "seed": seed, "rng": rng})
    adata.uns[key_added] = result
    update_metadata(
        adata,
        function_name="ripley_g",
        parameters={"celltype_column": celltype_column, "radii": [float(r) for r in radii], "n_permutations": n_permutations,
                    "seed": seed, "area": float(area), "spatial_key": spatial_key, "rng": rng,
                    "permgen_form": _permgen_form(ctx, n_cells, rng, n_permutations)},
        outputs={"uns": key_added, "n_celltypes": T, "n_cells": n_cells, "n_radii": R, "n_entries": n_entries},
    )
    return adata


CO_OCCURRENCE_MAX_THRESHOLDS = 128     # sc_cooccurrence_2d's envelope


def _interval_problem(interval) -> Optional[str]:
    """What is wrong with ``co_occurrence``'s ``interval`` as given (an integer number of thresholds, or the thresholds
    themselves), else None."""
    if isinstance(interval, (bool, np.bool_)):
        return f"interval must be an integer or a 1-D sequence of thresholds, got {interval!r}"
    if isinstance(interval, (int, np.integer)):
        if not 2 <= interval <= CO_OCCURRENCE_MAX_THRESHOLDS:
            return f"interval must give 2 to {CO_OCCURRENCE_MAX_THRESHOLDS} thresholds, got {interval}"
        return None
    try:
        t = np.asarray(interval, dtype=np.float64)
    except (TypeError, ValueError):
        return f"interval must be an integer or a 1-D sequence of thresholds, got {interval!r}"
    if t.ndim != 1:
        return f"interval must be an integer or a 1-D sequence of thresholds, got shape {t.shape}"
    t = np.sort(t)
    if not 2 <= t.size <= CO_OCCURRENCE_MAX_THRESHOLDS:
        return f"interval must give 2 to {CO_OCCURRENCE_MAX_THRESHOLDS} thresholds, got {t.size}"
    if not np.all(np.isfinite(t)):
        return f"interval must be finite, got {t[~np.isfinite(t)][0]}"
    if t[0] < 0:
        return f"interval must be non-negative, got {t[0]}"
    if np.any(np.diff(t) <= 0):
        j = int(np.argmax(np.diff(t) <= 0))
        return f"interval must be strictly increasing, got {t[j + 1]} after {t[j]}"
    with np.errstate(over="ignore"):
        if not np.isfinite(t[-1] * t[-1]):
            return f"interval must have a finite square, got {t[-1]}"
    return None


def _co_occurrence_request_problem(adata, cluster_key, spatial_key, interval) -> Optional[str]:
    """The first thing wrong with a ``co_occurrence`` request (checked before any device work), else None."""
    problem = _point_pattern_request_problem(adata, cluster_key, spatial_key, "co-occurrence")
    if problem:
        return problem
    n_missing = int(adata.obs[cluster_key].isna().sum())
    if n_missing:
        return (f"{n_missing} cells have missing labels in '{cluster_key}'. "
                "Fill or remove missing labels before computing co-occurrence.")
    return _interval_problem(interval)


def co_occurrence_thresholds(coords, interval) -> np.ndarray:
    """The float64 thresholds of ``co_occurrence``.  An array ``interval`` is sorted and returned.  An integer
    ``interval = m`` is squidpy's ``_find_min_max`` rule (restated from memory, not read): with ``s = x + y``, ``a`` and
    ``b`` the two cells of smallest ``s`` (stable order: ties go to the lowest index) and ``c`` the first cell of largest
    ``s``, ``t_min = dist(a, b)``, ``t_max = dist(a, c) / 2`` and the thresholds are ``np.linspace(t_min, t_max, m)`` --
    in float64, where squidpy works in float32.  ``ValueError`` when they do not come out strictly increasing."""
    if not isinstance(interval, (int, np.integer)):
        return np.sort(np.asarray(interval, dtype=np.float64))
    xy = np.asarray(coords, dtype=np.float64)
    if xy.shape[0] < 2:
        raise ValueError(f"interval={interval} derives the thresholds from the cells: at least 2 cells are needed, got {xy.shape[0]}")
    s = xy[:, 0] + xy[:, 1]
    a, b = np.argsort(s, kind="stable")[:2]
    c = int(np.argmax(s))

    def dist(p, q):
        dx, dy = xy[p, 0] - xy[q, 0], xy[p, 1] - xy[q, 1]
        return float(np.sqrt(dx * dx + dy * dy))

    t_min, t_max = dist(a, b), dist(a, c) / 2
    t = np.linspace(t_min, t_max, int(interval))
    if not (np.all(np.isfinite(t)) and np.all(np.diff(t) > 0)):
        raise ValueError(f"the thresholds derived from the cells are not strictly increasing: t_min = {t_min}, "
                         f"t_max = {t_max}; pass interval= as an array")
    return t


def co_occurrence_ratio(count) -> np.ndarray:
    """``occ`` (T, T, R) float32 from the (T, T, R + 1) integer table (pure host arithmetic, no device): for annulus
    ``r = 1 .. R`` with ``co = count[:, :, r]``, ``occ[a, b, r - 1] = co[a, b] * co.sum() / (co[a, :].sum() *
    co[:, b].sum())`` in float64, ``0 / 0`` giving NaN.  Bin 0, the pairs within the first threshold, has no ratio."""
    co = np.asarray(count, dtype=np.int64)[:, :, 1:]
    total = co.sum(axis=(0, 1)).astype(np.float64)
    rows = co.sum(axis=1).astype(np.float64)          # [a, r] = co[a, :].sum()
    cols = co.sum(axis=0).astype(np.float64)          # [b, r] = co[:, b].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        occ = co.astype(np.float64) * total[None, None, :] / (rows[:, None, :] * cols[None, :, :])
    return occ.astype(np.float32)


def co_occurrence(
    adata,
    cluster_key: str,
    spatial_key: str = "spatial",
    interval=50,
    copy: bool = False,
    n_splits: Optional[int] = None,
    n_jobs: Optional[int] = None,
    backend: str = "loky",
    show_progress_bar: bool = True,
    *,
    device: int = 0,
):
    """Cell-type co-occurrence by distance: squidpy's ``gr.co_occurrence``, every pair of cells in one pass on the GPU.

    EXTENSION -- the reference has no such function; the name, the keywords and the stored key are squidpy's.
    ``n_splits``, ``n_jobs``, ``backend`` and ``show_progress_bar`` are accepted and IGNORED: squidpy uses them to
    split its O(N^2) CPU loop, and there is nothing to split here.

    Semantics (include/spatialcore_hip.h, N9).  Thresholds ``t_0 < ... < t_R``: ``interval`` itself when it is an array
    (sorted; finite, non-negative, strictly increasing, 2 to 128 entries), else ``co_occurrence_thresholds``' rule for
    an integer ``interval`` (default 50 thresholds).  For an ordered pair of distinct cells
    ``d2 = fl(fl(dx dx) + fl(dy dy))`` in fp64, its bin is the smallest ``j`` with ``d2 <= fl(t_j t_j)`` (the closed
    ball of the radius graph and of ``ripley_k``), and a pair beyond ``t_R`` is dropped.  ``count[a, b, j]`` is the
    number of ordered pairs of types (a, b) in bin j: bin 0 the pairs within ``t_0``, bins 1 .. R the annuli
    ``(t_{j-1}, t_j]``.  ``occ[a, b, r - 1] = co[a, b] * co.sum() / (co[a, :].sum() * co[:, b].sum())`` with
    ``co = count[:, :, r]``, float64 arithmetic on the integers stored as float32, NaN for ``0 / 0``: squidpy's
    conditional-over-marginal ratio.  Two stated differences from squidpy, whose code was restated from memory and not
    read: the coordinates and thresholds stay in float64 (squidpy casts them to float32), and the formula is the one
    above.  The types are the categories of a categorical column, unused ones kept as all-zero rows (NaN in ``occ``),
    else the sorted unique labels.

    Stored in ``adata.uns[f"{cluster_key}_co_occurrence"]``: ``occ`` (T, T, R) float32, ``interval`` (R + 1,) float64,
    ``count`` (T, T, R + 1) int64, ``celltypes``, ``n_per_type``.  ``copy=True`` returns ``(occ, interval)`` and writes
    nothing to ``adata`` -- squidpy's convention, unlike this package's own functions, whose ``copy`` returns a copied
    AnnData.  With ``copy=False`` the function returns ``adata``, as its siblings here do.
    """
    problem = _co_occurrence_request_problem(adata, cluster_key, spatial_key, interval)
    if problem:
        raise ValueError(problem)
    celltypes, codes = _category_codes(adata, cluster_key)
    coords = _coordinates(adata, spatial_key)
    thresholds = co_occurrence_thresholds(coords, interval)
    n_cells, T, R = adata.n_obs, len(celltypes), thresholds.size - 1
    if n_cells < 1 or T < 1:
        raise ValueError("co_occurrence needs at least one cell")
    logger.info(f"Computing co-occurrence: {n_cells:,} cells, {T} cell types, {R} intervals from {thresholds[0]:g} "
                f"to {thresholds[-1]:g}")

    order = np.argsort(codes, kind="stable")
    n_per_type = np.bincount(codes, minlength=T).astype(np.int64)
    type_off = np.concatenate([[0], np.cumsum(n_per_type)]).astype(np.int64)
    ctx = _lib.default_context(device)
    count = ctx.cooccurrence_counts(coords[order], type_off, thresholds)
    occ = co_occurrence_ratio(count)
    logger.debug(f"{int(count.sum()):,} of {n_cells * (n_cells - 1):,} ordered pairs lie within {thresholds[-1]:g}")
    if copy:
        return occ, thresholds
    key_added = f"{cluster_key}_co_occurrence"
    adata.uns[key_added] = {"occ": occ, "interval": thresholds, "count": count, "celltypes": celltypes,
                            "n_per_type": n_per_type}
    logger.info(f"Stored co-occurrence in adata.uns['{key_added}'] (occ shape: {occ.shape})")
    update_metadata(
        adata,
        function_name="co_occurrence",
        parameters={"cluster_key": cluster_key, "spatial_key": spatial_key,
                    "interval": int(interval) if isinstance(interval, (int, np.integer)) else [float(t) for t in thresholds]},
        outputs={"uns": key_added, "n_celltypes": T, "n_cells": n_cells, "n_intervals": R,
                 "n_pairs": int(count.sum())},
    )
    return adata


LIGREC_MAX_CLUSTERS = 96        # sc_ligrec_*'s envelope
LIGREC_MAX_SHIFT_SPREAD = 30    # |s_L - s_R| of an interaction at most: the comparison stays inside 128 bits


def ligrec_shifts(X) -> np.ndarray:
    """The shift ``s_g`` of every column of the host matrix ``X`` (cells x genes, dense or scipy sparse), int32: 0 for a
    gene whose values are all integers in [0, 2^32) -- raw counts are summed as they are -- else ``32 - e_g`` with ``e_g``
    the smallest integer such that ``max |x| < 2^e_g`` (``np.frexp``'s exponent).  A value enters the test as the integer
    ``rint(x * 2**s_g)``.  ``ValueError`` naming the columns that hold a non-finite value."""
    from scipy import sparse

    if sparse.issparse(X):
        Xc = X.tocsc()
        columns = (Xc.data[Xc.indptr[g]:Xc.indptr[g + 1]] for g in range(Xc.shape[1]))
    else:
        A = np.asarray(X)
        columns = (A[:, g] for g in range(A.shape[1]))
    shifts, bad = [], []
    for g, col in enumerate(columns):
        col = np.asarray(col, dtype=np.float64)
        if not np.all(np.isfinite(col)):
            bad.append(g)
            shifts.append(0)
            continue
        top = float(np.abs(col).max()) if col.size else 0.0
        counts = col.size == 0 or (col.min() >= 0 and top < 4294967296.0 and bool(np.all(col == np.floor(col))))
        shifts.append(0 if counts else 32 - int(np.frexp(top)[1]))
    if bad:
        raise ValueError(f"non-finite expression values in columns {bad[:10]}{'...' if len(bad) > 10 else ''}")
    return np.asarray(shifts, dtype=np.int32)


def _ligrec_interactions(interactions, var_names):
    """``(pairs, metadata, n_unknown)``: the distinct (source, target) name pairs whose two genes are in ``var_names``, in
    the order given; the other columns of an interactions frame for those pairs (None when there are none); how many
    distinct pairs were dropped for an unknown name.  A string means the request is malformed."""
    if isinstance(interactions, pd.DataFrame):
        if "source" not in interactions.columns or "target" not in interactions.columns:
            return "interactions must have the columns 'source' and 'target'"
        frame = interactions.reset_index(drop=True)
    else:
        try:
            rows = [tuple(p) for p in interactions]
        except TypeError:
            return "interactions must be a DataFrame with 'source' and 'target' columns or a sequence of (source, target) pairs"
        if any(len(p) != 2 for p in rows):
            return "interactions must be a DataFrame with 'source' and 'target' columns or a sequence of (source, target) pairs"
        frame = pd.DataFrame(rows, columns=["source", "target"])
    frame = frame.assign(source=frame["source"].astype(str), target=frame["target"].astype(str))
    frame = frame.drop_duplicates(subset=["source", "target"], keep="first")
    known = frame["source"].isin(var_names) & frame["target"].isin(var_names)
    n_unknown = int((~known).sum())
    frame = frame[known].reset_index(drop=True)
    pairs = list(zip(frame["source"], frame["target"]))
    extra = frame.drop(columns=["source", "target"])
    metadata = None
    if extra.shape[1]:
        extra.index = pd.MultiIndex.from_tuples(pairs, names=["source", "target"])
        metadata = extra
    return pairs, metadata, n_unknown


def _ligrec_cluster_pairs(clusters, categories):
    """The ordered cluster pairs (as positions in ``categories``) that ``clusters`` asks for: all K^2 for None, every
    ordered pair of a subset of categories, or the listed pairs themselves.  A string names what is wrong."""
    where = {c: k for k, c in enumerate(categories)}
    K = len(categories)
    if clusters is None:
        return [(a, b) for a in range(K) for b in range(K)]
    items = list(clusters)
    if not items:
        return "clusters must not be empty"
    if all(isinstance(it, (tuple, list)) and len(it) == 2 for it in items):
        flat = [c for it in items for c in it]
        pairs = [tuple(it) for it in items]
    else:
        flat = items
        pairs = [(a, b) for a in items for b in items]
    unknown = [c for c in flat if not isinstance(c, (str, int, float, np.generic)) or c not in where]
    if unknown:
        return f"clusters {unknown[:5]} are not categories of the cluster column (categories: {list(categories)[:10]}...)"
    return list(dict.fromkeys((where[a], where[b]) for a, b in pairs))


def _ligrec_request_problem(adata, cluster_key, interactions, clusters, n_perms, threshold, corr_method, corr_axis, rng,
                            comm, perm_batch, gene_batch) -> Optional[str]:
    """The first thing wrong with a ``ligrec`` request (checked before any device work), else None."""
    if cluster_key not in adata.obs.columns:
        return (f"Column '{cluster_key}' not found in adata.obs. "
                f"Available columns: {list(adata.obs.columns)[:10]}...")
    n_missing = int(adata.obs[cluster_key].isna().sum())
    if n_missing:
        return (f"{n_missing} cells have missing labels in '{cluster_key}'. "
                "Fill or remove missing labels before running ligrec.")
    if interactions is None:
        return "interactions is required: no database is fetched (pass a DataFrame with 'source' and 'target' columns)"
    parsed = _ligrec_interactions(interactions, adata.var_names)
    if isinstance(parsed, str):
        return parsed
    if not parsed[0]:
        return (f"no interaction is left: none of the given (source, target) pairs has both genes in adata.var_names "
                f"({parsed[2]} dropped)")
    if n_perms < 0:
        return f"n_perms must be >= 0, got {n_perms}"
    if not 0 <= threshold <= 1:
        return f"threshold must lie in [0, 1], got {threshold}"
    if corr_method not in (None, "fdr_bh", "bonferroni"):
        return f"corr_method must be None, 'fdr_bh' or 'bonferroni', got '{corr_method}'"
    if corr_axis not in ("clusters", "interactions"):
        return f"corr_axis must be 'clusters' or 'interactions', got '{corr_axis}'"
    if _rng_problem(rng):
        return _rng_problem(rng)
    if comm is not None and comm.world > 1 and rng != "philox":
        return "permutations can only be sharded over ranks (comm=) with rng='philox': the numpy stream is sequential"
    if perm_batch < 1:
        return f"perm_batch must be >= 1, got {perm_batch}"
    if gene_batch is not None and gene_batch < 2:
        return f"gene_batch must be >= 2 (an interaction needs its two genes in one batch), got {gene_batch}"
    labels = adata.obs[cluster_key]
    categories = list(labels.cat.categories) if isinstance(labels.dtype, pd.CategoricalDtype) else sorted(set(labels.values))
    if not 1 <= len(categories) <= LIGREC_MAX_CLUSTERS:
        return f"ligrec supports 1 to {LIGREC_MAX_CLUSTERS} clusters, '{cluster_key}' has {len(categories)}"
    picked = _ligrec_cluster_pairs(clusters, categories)
    if isinstance(picked, str):
        return picked
    return None


def _ligrec_gene_batch(n_cells: int, requested: Optional[int]) -> int:
    """Genes per device batch of ``ligrec``, sized like ``morans_i``'s: the fp64 tiles are 8 bytes per (cell, gene), and
    half of a 128 GB budget is left to the permutation table, the label words and the null tables."""
    if requested is not None:
        return int(requested)
    fit = int((64 << 30) // (8 * max(n_cells, 1)))
    return max(64, fit // 64 * 64)


def _ligrec_batches(pairs_idx, gene_batch: int):
    """The interactions (pairs of gene positions) cut, in order, into batches whose distinct genes number at most
    ``gene_batch``: ``[(genes, rows)]`` with ``genes`` sorted and ``rows`` the batch's interaction numbers.  A gene may be
    loaded with several batches; its integers do not depend on its company."""
    batches, genes, rows = [], set(), []
    for i, (l, r) in enumerate(pairs_idx):
        if rows and len(genes | {l, r}) > gene_batch:
            batches.append((sorted(genes), rows))
            genes, rows = set(), []
        genes |= {l, r}
        rows.append(i)
    batches.append((sorted(genes), rows))
    return batches


def ligrec_adjust(pvalues: np.ndarray, method: Optional[str], axis: str) -> np.ndarray:
    """``pvalues`` (interactions x cluster pairs, NaN = not tested) corrected over the non-NaN entries of every cluster-pair
    COLUMN (``axis="clusters"``: one family per cluster pair, its interactions) or of every interaction ROW
    (``axis="interactions"``), in float64.  ``"bonferroni"``: ``min(p m, 1)`` with m the family's size; ``"fdr_bh"``:
    Benjamini-Hochberg, ``min over ranks j >= k of p_(j) m / j``, clipped at 1 (the step-up form of the tables in
    ``autocorrelation._padj_tables``, on values instead of permutation-count levels).  NaN stays NaN."""
    p = np.array(pvalues, dtype=np.float64)
    if method is None:
        return p
    fam = p if axis == "interactions" else p.T      # (a view: families are rows)
    for row in fam:
        ok = ~np.isnan(row)
        m = int(ok.sum())
        if m == 0:
            continue
        v = row[ok]
        if method == "bonferroni":
            row[ok] = np.minimum(v * m, 1.0)
            continue
        order = np.argsort(v, kind="stable")
        adj = v[order] * m / np.arange(1, m + 1)
        adj = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
        out = np.empty(m, dtype=np.float64)
        out[order] = adj
        row[ok] = out
    return p


def ligrec_statistics(sums, nnz, group_n, shifts, pairs_idx, cluster_pairs, count_ge, n_perms: int, threshold: float):
    """``(means, pvalues)`` (interactions x cluster pairs, float64) from the integer tables alone (pure host arithmetic):
    ``m[c, g] = float(S[c, g]) * 2**-s_g / n_c`` (0 for an empty cluster), ``means = (m[a, L] + m[b, R]) / 2`` and 0 where
    either mean is <= 0; ``pvalues = count_ge / n_perms``, NaN where ``N[a, L] / n_a < threshold`` or
    ``N[b, R] / n_b < threshold`` (float64 division; an empty cluster is never kept); None for ``n_perms = 0``."""
    S, N = np.asarray(sums, dtype=np.int64), np.asarray(nnz, dtype=np.int64)
    n_c = np.asarray(group_n, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.ldexp(S.astype(np.float64), -np.asarray(shifts, dtype=np.int64)[None, :]) / n_c[:, None].astype(np.float64)
        frac = N.astype(np.float64) / n_c[:, None].astype(np.float64)
    m[n_c == 0, :] = 0.0
    L = np.asarray([l for l, _ in pairs_idx], dtype=np.intp)
    R = np.asarray([r for _, r in pairs_idx], dtype=np.intp)
    A = np.asarray([a for a, _ in cluster_pairs], dtype=np.intp)
    B = np.asarray([b for _, b in cluster_pairs], dtype=np.intp)
    mL, mR = m[A[None, :], L[:, None]], m[B[None, :], R[:, None]]
    means = np.where((mL > 0) & (mR > 0), (mL + mR) / 2, 0.0)
    if n_perms <= 0:
        return means, None
    keep = (frac[A[None, :], L[:, None]] >= threshold) & (frac[B[None, :], R[:, None]] >= threshold)
    pvalues = np.where(keep, np.asarray(count_ge, dtype=np.int64) / n_perms, np.nan)
    return means, pvalues


def ligrec(
    adata,
    cluster_key: str,
    interactions=None,
    clusters=None,
    n_perms: int = 1000,
    threshold: float = 0.01,
    corr_method: Optional[str] = None,
    corr_axis: str = "clusters",
    alpha: float = 0.05,
    seed: int = 0,
    key_added: Optional[str] = None,
    copy: bool = False,
    *,
    device: int = 0,
    perm_batch: int = 512,
    gene_batch: Optional[int] = None,
    rng: str = "numpy",
    comm=None,
):
    """Ligand-receptor permutation test over ordered cluster pairs: squidpy's ``gr.ligrec`` (the CellPhoneDB test) on the GPU.

    EXTENSION -- the reference has no such function; the name and the keywords are squidpy's, the semantics are defined
    here (include/spatialcore_hip.h, N10).  For every interaction (L, R) and every ordered pair of
    clusters (a, b): is the mean of L in a plus the mean of R in b higher than under shuffled cluster labels?

    Inputs.  ``adata.X`` (cells x genes, CSR or dense, float32 or float64); ``cluster_key``, a column with K <= 96
    categories (those of a categorical column, unused ones kept; else the sorted unique labels); ``interactions``, a
    DataFrame with ``source`` and ``target`` columns or a sequence of ``(source, target)`` names.  NO DATABASE IS FETCHED:
    ``interactions`` is required.  Duplicate pairs are dropped, a pair with a name that is not in ``var_names`` is dropped
    (one log line gives the count), and nothing left is a ``ValueError``.  Complexes (``A_B``) and ``use_raw`` are out of
    scope: ``SimpleAnnData`` has no ``.raw``, and a name is looked up as it stands.

    Arithmetic: exact integers, order-free.  Gene g carries a shift ``s_g`` (``ligrec_shifts``: 0 for integer counts in
    [0, 2^32), else ``32 - e_g`` with ``max |x| < 2^e_g``) and every value enters as ``q = rint(x * 2**s_g)``, |q| < 2^32.
    ``S[c, g]`` = sum of q over cluster c (int64), ``N[c, g]`` = cells of c with x > 0, ``n_c`` = cells of c.  A label
    permutation keeps every ``n_c``, so "permuted ``(mean_L,a + mean_R,b) / 2`` >= observed" is decided as
    ``2^s_R n_b (S_p[a, L] - S[a, L]) + 2^s_L n_a (S_p[b, R] - S[b, R]) >= 0`` in 128-bit integers on the device; an
    interaction whose two shifts differ by more than 30 is a ``ValueError`` naming the genes.  The result is a function of
    the inputs alone: it does not depend on ``perm_batch``, ``gene_batch``, the rank count or the run.

    Stored in ``adata.uns[key_added or f"{cluster_key}_ligrec"]``, rows a MultiIndex ``(source, target)``, columns a
    MultiIndex ``(cluster_1, cluster_2)``: ``means`` = ``(m_L,a + m_R,b) / 2`` with ``m = float(S) * 2**-s / n_c`` in
    float64, 0 where either mean is <= 0; ``count_ge`` (int64); ``pvalues = count_ge / n_perms`` -- squidpy's and
    CellPhoneDB's form, WITHOUT the +1 in numerator and denominator that this package's other permutation tests use --
    NaN where ``N[a, L] / n_a < threshold`` or ``N[b, R] / n_b < threshold`` (``>=`` keeps), absent for ``n_perms = 0``;
    ``metadata``, the interactions frame's other columns, if any; and ``n_perms``, ``seed``, ``rng``, ``clusters`` (the
    categories), ``threshold``, ``alpha`` (recorded only), ``corr_method``, ``corr_axis``.  ``corr_method`` (None,
    ``"fdr_bh"``, ``"bonferroni"``) corrects the non-NaN p-values along ``corr_axis`` (``ligrec_adjust``:
    ``"clusters"`` = every cluster-pair column over its interactions, ``"interactions"`` = every interaction row over its
    cluster pairs).  ``clusters``: a subset of categories (all their ordered pairs) or a list of ordered pairs; default
    all K^2.  It selects columns only: the null always permutes the labels of ALL cells.

    Null: ``labels[perm_p]``, the sources and rules of ``neighborhood_enrichment``.  ``rng="numpy"`` (default):
    ``default_rng(seed).permutation(n)`` continued batch after batch on one GPU; every gene batch sees the same
    permutations (a permutation batch is generated once and all gene batches run against it).  ``rng="philox"``:
    counter-based, and with ``comm`` sharded by ``shard_bounds`` and merged with one ``sum_over_ranks_i64`` of
    ``count_ge``.  Sharding with ``rng="numpy"`` is a ``ValueError``.  ``copy=True`` works on, and returns, a copy.
    """
    problem = _ligrec_request_problem(adata, cluster_key, interactions, clusters, n_perms, threshold, corr_method, corr_axis,
                                      rng, comm, perm_batch, gene_batch)
    if problem:
        raise ValueError(problem)
    if copy:
        adata = adata.copy()
    n_cells = adata.n_obs
    categories, codes = _category_codes(adata, cluster_key)
    K = len(categories)
    cluster_pairs = _ligrec_cluster_pairs(clusters, categories)
    pairs, metadata, n_unknown = _ligrec_interactions(interactions, adata.var_names)
    if n_unknown:
        logger.info(f"Dropped {n_unknown} interactions with a gene that is not in adata.var_names")
    names = list(dict.fromkeys(g for pair in pairs for g in pair))            # the G distinct genes, first-seen order
    var_pos = np.asarray([adata.var_names.get_loc(g) for g in names], dtype=np.int64)
    at = {g: j for j, g in enumerate(names)}
    pairs_idx = [(at[l], at[r]) for l, r in pairs]
    X = adata.X
    shifts = ligrec_shifts(X[:, var_pos])
    for l, r in pairs_idx:
        if abs(int(shifts[l]) - int(shifts[r])) > LIGREC_MAX_SHIFT_SPREAD:
            raise ValueError(f"interaction ({names[l]}, {names[r]}): the value ranges of the two genes are too far apart for "
                             f"the exact comparison (shifts {int(shifts[l])} and {int(shifts[r])} differ by more than "
                             f"{LIGREC_MAX_SHIFT_SPREAD}); rescale one of them")
    G, I = len(names), len(pairs)
    logger.info(f"Computing ligrec: {n_cells:,} cells, {K} clusters, {I} interactions of {G} genes, permutations={n_perms}")

    ctx = _lib.default_context(device)
    batches = _ligrec_batches(pairs_idx, _ligrec_gene_batch(n_cells, gene_batch))
    group_n = np.bincount(codes, minlength=K).astype(np.int64)
    resident = [None]

    def all_gene_batches(call):
        """One device call per gene batch (loaded unless it is the resident one), all against the same permutations:
        the observed integers ``(S, N)``, and ``count_ge`` of those permutations."""
        S, N = np.zeros((K, G), dtype=np.int64), np.zeros((K, G), dtype=np.int64)
        count_ge = np.zeros((I, K, K), dtype=np.int64)
        for batch in batches:
            genes, rows = batch
            if resident[0] is not batch:
                ctx.set_expression(X, var_pos[genes])
                resident[0] = batch
            local = {g: j for j, g in enumerate(genes)}
            r = call(codes, K, shifts[genes], [local[pairs_idx[i][0]] for i in rows], [local[pairs_idx[i][1]] for i in rows])
            S[:, genes], N[:, genes] = r["sum"], r["nnz"]
            count_ge[rows] += r["count_ge"]
        return (S, N), count_ge

    # a batch of the numpy stream is generated once and every gene batch runs against those rows; counter-based
    # permutation p is a function of (seed, p), so there too every gene batch sees the same ones
    (S, N), count_ge = _label_permutation_null(
        ctx, n_cells, n_perms, seed, perm_batch, rng, comm,
        lambda rows: all_gene_batches(lambda *a: ctx.ligrec_counts(*a, rows)),
        lambda lo, n: all_gene_batches(lambda *a: ctx.ligrec_counter(*a, seed, lo, n, perm_batch)))

    A = [a for a, _ in cluster_pairs]
    B = [b for _, b in cluster_pairs]
    picked_ge = count_ge[:, A, B]
    means, pvalues = ligrec_statistics(S, N, group_n, shifts, pairs_idx, cluster_pairs, picked_ge, n_perms, threshold)
    index = pd.MultiIndex.from_tuples(pairs, names=["source", "target"])
    columns = pd.MultiIndex.from_tuples([(categories[a], categories[b]) for a, b in cluster_pairs],
                                        names=["cluster_1", "cluster_2"])
    result = {"means": pd.DataFrame(means, index=index, columns=columns),
              "count_ge": pd.DataFrame(picked_ge, index=index, columns=columns)}
    if pvalues is not None:
        result["pvalues"] = pd.DataFrame(ligrec_adjust(pvalues, corr_method, corr_axis), index=index, columns=columns)
    if metadata is not None:
        result["metadata"] = metadata
    result.update({"n_perms": n_perms, "seed": seed, "rng": rng, "clusters": list(categories), "threshold": threshold,
                   "alpha": alpha, "corr_method": corr_method, "corr_axis": corr_axis})
    key_added = key_added or f"{cluster_key}_ligrec"
    adata.uns[key_added] = result
    logger.info(f"Stored ligrec results in adata.uns['{key_added}'] ({I} interactions x {len(cluster_pairs)} cluster pairs)")
    update_metadata(
        adata,
        function_name="ligrec",
        parameters={"cluster_key": cluster_key, "n_perms": n_perms, "threshold": threshold, "corr_method": corr_method,
                    "corr_axis": corr_axis, "alpha": alpha, "seed": seed, "rng": rng,
                    "permgen_form": _permgen_form(ctx, n_cells, rng, n_perms)},
        outputs={"uns": key_added, "n_clusters": K, "n_cells": n_cells, "n_interactions": I, "n_genes": G,
                 "n_cluster_pairs": len(cluster_pairs), "n_dropped_interactions": n_unknown},
    )
    return adata


def _niche_request_problem(adata, n_niches, method, neighborhood_key) -> Optional[str]:
    """The first thing wrong with an identify_niches request, as the reference words it (NB:416-436), else None."""
    if neighborhood_key not in adata.obsm:
        return (f"adata.obsm['{neighborhood_key}'] not found. "
                "Run compute_neighborhood_profile() first.")
    if method not in ["kmeans", "minibatch_kmeans"]:
        return f"Invalid method: '{method}'. Must be 'kmeans' or 'minibatch_kmeans'."
    if n_niches < 2:
        return f"n_niches must be >= 2, got {n_niches}"
    if n_niches > adata.n_obs:
        return f"n_niches ({n_niches}) cannot exceed number of cells ({adata.n_obs})"
    return None


def identify_niches(
    adata,
    n_niches: int,
    method: str = "kmeans",
    neighborhood_key: str = "neighborhood_profile",
    key_added: str = "niche",
    random_state: int = 0,
    n_init: int = 10,
    max_iter: int = 300,
    copy: bool = False,
    *,
    device: int = 0,
):
    """Cluster neighbourhood profiles into niches (NB:299-522): sklearn's ``KMeans(init="k-means++")`` on the GPU.

    Same outputs as the reference: ``adata.obs[key_added]`` (Categorical ``niche_1..niche_K``),
    ``adata.uns["niche_centroids"]`` (K, C) in the input's dtype and ``adata.uns["niche_params"]``.
    ``method="minibatch_kmeans"`` is answered with the same exact full-batch algorithm (sklearn's
    minibatch stream draws depend on the data); ``niche_params["method"]`` records what was asked.
    """
    problem = _niche_request_problem(adata, n_niches, method, neighborhood_key)
    if problem:
        raise ValueError(problem)
    n_cells = adata.n_obs
    adata = adata.copy() if copy else adata
    profiles = adata.obsm[neighborhood_key]
    logger.info(
        f"Identifying {n_niches} niches from {n_cells:,} cells "
        f"(method={method}, random_state={random_state})"
    )
    empty_mask = profiles.sum(axis=1) == 0
    n_empty = int(np.asarray(empty_mask).sum())
    if n_empty > 0:
        raise ValueError(f"{n_empty} cells have empty neighborhood profiles. "
                         "Increase radius, switch to knn, or pre-filter isolated cells before profiling.")

    X = profiles.toarray() if hasattr(profiles, "toarray") else np.asarray(profiles)
    if X.dtype not in (np.float32, np.float64):      # sklearn's validate_data: float64 unless float32
        X = X.astype(np.float64)
    X = np.ascontiguousarray(X)
    if method == "kmeans":
        logger.debug(f"Running KMeans (n_init={n_init}, max_iter={max_iter})")
    else:
        logger.info("method='minibatch_kmeans' is answered with full-batch Lloyd k-means on the GPU "
                    "(exact; the same result as method='kmeans')")
    tol = np.mean(np.var(X, axis=0)) * 1e-4           # sklearn's _tolerance, on the input
    x_mean = X.mean(axis=0)
    draws = kmeans_draws(random_state, n_init, n_niches)

    ctx = _lib.default_context(device)
    fit = ctx.kmeans(X, n_niches, n_init, max_iter, float(tol), x_mean, draws)
    labels, centroids, inertia = fit["labels"], fit["centers"], fit["inertia"]
    if fit["distinct"] < n_niches:
        warnings.warn(
            "Number of distinct clusters ({}) found smaller than "
            "n_clusters ({}). Possibly due to duplicate points "
            "in X.".format(fit["distinct"], n_niches),
            ConvergenceWarning,
            stacklevel=2,
        )

    niche_names = [f"niche_{i + 1}" for i in range(n_niches)]
    adata.obs[key_added] = pd.Categorical.from_codes(labels, categories=niche_names)
    adata.uns["niche_centroids"] = centroids
    adata.uns["niche_params"] = {
        "n_niches": n_niches,
        "method": method,
        "neighborhood_key": neighborhood_key,
        "random_state": random_state,
        "n_init": n_init,
        "max_iter": max_iter,
        "inertia": float(inertia),
    }
    cluster_sizes = np.bincount(labels, minlength=n_niches)
    cluster_sizes = cluster_sizes[cluster_sizes > 0]
    logger.info(f"Niche sizes: min={cluster_sizes.min()}, "
                f"max={cluster_sizes.max()}, mean={cluster_sizes.mean():.0f}")
    logger.info(f"Stored niche labels in adata.obs['{key_added}'] "
                f"and centroids in adata.uns['niche_centroids']")
    update_metadata(
        adata,
        function_name="identify_niches",
        parameters={
            "n_niches": n_niches,
            "method": method,
            "neighborhood_key": neighborhood_key,
            "random_state": random_state,
            "n_init": n_init,
            "max_iter": max_iter,
            "algorithm": "lloyd",
        },
        outputs={
            "obs": key_added,
            "uns_centroids": "niche_centroids",
            "uns_params": "niche_params",
            "inertia": float(inertia),
            "n_iter": fit["n_iter"],
            "strict_convergence": fit["strict"],
        },
    )
    return adata
