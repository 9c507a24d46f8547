"""Spatial domains on MI355X: buffer - union - shrink over discs, computed from the points alone.

Same public contract as the reference's ``make_spatial_domains`` / ``get_domain_summary`` (reference
src/spatialcore/spatial/domains.py:289-732 and 735-792, ``DM`` below): keywords, defaults, filter expressions,
platform defaults, ``adata.obs[output_column]``, error messages, log lines and the provenance entry.  The reference
runs the geometry as an R subprocess (``sf`` + ``concaveman``, DM:579-638); there is no R here.  The geometry is
restated in its continuous meaning (include/spatialcore_hip.h N7) and evaluated by ``sc_domains_2d``:

* buffer + union: the union U of the closed discs of radius ``cell_dist_um`` about the target cells; its pieces are
  the connected components of the targets under "within 2 * cell_dist_um";
* shrink: a cell is in a domain iff the closed disc of radius ``cell_dist_um - shrink_margin_um`` about it lies in U;
* the reduce (``<=`` thresholds) and number (largest first) steps are ``np.bincount`` on the two integer arrays that
  come back.

Deviations from the R pipeline, all three deliberate:

1. No concave hull: ``concaveman`` fills holes and bridges the pieces of an eroded polygon.  Cells in a hole of U, or
   of its erosion, stay unassigned here.
2. A small domain is dropped, never merged: under this definition the regions of different components are disjoint,
   so a small domain has no neighbour to merge into (the reference merges it into the first kept hull it intersects).
3. ``0 < shrink_margin_um <= cell_dist_um`` is required (the reference passes anything to ``sf``, where a margin
   larger than the buffer turns the shrink into a second growth).
"""

from __future__ import annotations

import re
from pathlib import Path
from typing import Dict, Optional, Tuple, Union

import numpy as np
import pandas as pd

from spatialcore_amd import _lib
from spatialcore_amd._logging import get_logger
from spatialcore_amd._metadata import update_metadata

logger = get_logger("spatial.domains")

# Platform-specific defaults for cell_dist_um: typical cell spacing in the platform's native units (DM:83-87)
PLATFORM_DEFAULTS: Dict[str, float] = {
    "cosmx": 400.0,   # pixels (coordinates typically 0-120000)
    "xenium": 50.0,   # microns (typically 0-10000)
    "visium": 200.0,  # spot array units (typically 0-50000)
}

# Coordinate range thresholds for platform auto-detection (DM:91-95)
PLATFORM_COORD_RANGES: Dict[str, Tuple[float, float]] = {
    "cosmx": (50000.0, float("inf")),
    "xenium": (0.0, 15000.0),
    "visium": (15000.0, 50000.0),
}


def _detect_platform(adata) -> Optional[str]:
    """Platform from the largest absolute coordinate (DM:98-141); None when there are no coordinates."""
    if "spatial" not in adata.obsm:
        return None
    spatial_coords = np.asarray(adata.obsm["spatial"])
    if spatial_coords.shape[0] == 0:
        return None
    max_coord = np.max(np.abs(spatial_coords))
    if max_coord > PLATFORM_COORD_RANGES["cosmx"][0]:
        return "cosmx"
    elif max_coord <= PLATFORM_COORD_RANGES["xenium"][1]:
        return "xenium"
    elif max_coord <= PLATFORM_COORD_RANGES["visium"][1]:
        return "visium"
    return None


def _get_platform_defaults(platform: str) -> float:
    """Default cell_dist_um of a platform (DM:144-170)."""
    platform_lower = platform.lower()
    if platform_lower not in PLATFORM_DEFAULTS:
        valid_platforms = list(PLATFORM_DEFAULTS.keys())
        raise ValueError(f"Unknown platform '{platform}'. Valid platforms are: {valid_platforms}")
    return PLATFORM_DEFAULTS[platform_lower]


def _evaluate_filter_expression(filter_expression: str, adata) -> pd.Series:
    """Boolean mask of the target cells (DM:173-252): column equality (``"cell_type == 'B cell'"``,
    ``"cluster == 1"``), a boolean column (``"is_tumor"``), or any expression ``adata.obs.eval`` understands.
    Ontology IDs (``"CL:0000236"``) need the reference's ontology package, which this project does not carry."""
    expr = filter_expression.strip()

    if re.search(r'[A-Z]+:[0-9]+', expr):
        raise NotImplementedError(
            f"Ontology IDs in filter expressions are not supported: '{filter_expression}'. "
            "Use column equality (\"cell_type == 'B cell'\") or a boolean column instead."
        )

    equality_match = re.match(r"^(\w+)\s*==\s*['\"]?(.+?)['\"]?$", expr)
    if equality_match:
        col_name = equality_match.group(1)
        col_value = equality_match.group(2)
        if col_name not in adata.obs.columns:
            raise ValueError(
                f"Column '{col_name}' not found in adata.obs. "
                f"Available columns: {list(adata.obs.columns)[:10]}..."
            )
        return adata.obs[col_name] == col_value

    if expr in adata.obs.columns:
        col = adata.obs[expr]
        if col.dtype == bool or set(col.dropna().unique()).issubset({True, False, "True", "False"}):
            if col.dtype == object:
                return col.map({"True": True, "False": False, True: True, False: False}).fillna(False)
            return col.fillna(False).astype(bool)
        else:
            raise ValueError(
                f"Column '{expr}' exists but is not boolean. "
                f"Use equality syntax like \"{expr} == 'value'\" instead."
            )

    try:
        result = adata.obs.eval(expr)
        return result.astype(bool)
    except Exception as e:
        raise ValueError(
            f"Could not evaluate filter expression: '{filter_expression}'. "
            f"Error: {e}\n"
            "Supported formats:\n"
            "  - Ontology ID: 'CL:0000236'\n"
            "  - Column equality: \"cell_type == 'B cell'\"\n"
            "  - Boolean column: 'is_tumor'\n"
            "  - Compound: 'CL:0000236 & is_tumor'"
        ) from e


def _generate_domain_prefix(filter_expression: str) -> str:
    """A sanitised prefix for the domain names (DM:255-286)."""
    ontology_match = re.search(r'([A-Z]+):([0-9]+)', filter_expression)
    if ontology_match:
        return f"{ontology_match.group(1)}_{ontology_match.group(2)}"
    equality_match = re.match(r"^(\w+)\s*==\s*['\"]?(.+?)['\"]?$", filter_expression)
    if equality_match:
        return re.sub(r'[^a-zA-Z0-9_]', '_', equality_match.group(2))
    prefix = re.sub(r'[^a-zA-Z0-9_]', '_', filter_expression[:20])
    return prefix if prefix else "domain"


def _number_domains(comp_t: np.ndarray, comp_q: np.ndarray, min_target: int, min_total: Optional[int]):
    """Reduce and number: rank (1 = largest, 0 = none) per target and per query.  A component with
    ``n_target <= min_target`` -- or ``n_total <= min_total`` -- is small (the ``<=`` of r_functions.R:181,189) and is
    dropped; the survivors are numbered by assigned-cell count, largest first, ties to the smaller component id."""
    n = comp_t.size
    n_target = np.bincount(comp_t, minlength=n)
    n_total = n_target + np.bincount(comp_q[comp_q >= 0], minlength=n)
    keep = n_target > min_target
    if min_total is not None:
        keep &= n_total > min_total
    ids = np.flatnonzero(keep)
    order = ids[np.lexsort((ids, -n_total[ids]))]
    rank = np.zeros(n + 1, dtype=np.int64)        # slot n takes the -1 of the cells outside every region
    rank[order] = np.arange(1, order.size + 1)
    return rank[comp_t], rank[comp_q]


def make_spatial_domains(
    adata,
    filter_expression: Optional[str] = None,
    cell_dist_um: Optional[float] = None,
    shrink_margin_um: float = 25.0,
    domain_prefix: Optional[str] = None,
    min_target_cells_domain: int = 10,
    min_total_cells_domain: Optional[int] = None,
    output_column: str = "spatial_domain",
    assign_all_cells: bool = True,
    domain_expansion_warn_ratio: float = 10.0,
    r_functions_path: Optional[Union[str, Path]] = None,
    copy: bool = False,
    platform: Optional[str] = None,
    *,
    device: int = 0,
):
    """Create spatial domains from the cells a filter selects, by buffer - union - shrink (DM:289-732).

    1. Buffer each target cell by ``cell_dist_um`` and union the discs.
    2. Shrink by ``cell_dist_um - shrink_margin_um``: a cell is inside iff the disc of that radius about it lies in
       the union.
    3. Drop small domains, number the rest by assigned-cell count (``{domain_prefix}_1`` is the largest; ties go to
       the domain that holds the earliest target cell).

    Parameters are the reference's (DM:319-380).  ``cell_dist_um=None`` takes the platform default (CosMx 400, Xenium
    50, Visium 200), the platform auto-detected from the coordinate range unless given.  ``min_target_cells_domain``
    / ``min_total_cells_domain``: a domain with that many target (total) cells OR FEWER is dropped.
    ``assign_all_cells=False`` assigns the target cells only.  ``r_functions_path`` is accepted and ignored: there is
    no R in this path, hence no ``RNotFoundError`` either.  ``device`` (keyword only): the GPU to run on.

    Deviations from the reference's R pipeline:

    * no concave hull -- cells in a hole of the union, or of its erosion, stay unassigned (``concaveman`` fills holes
      and bridges the pieces of an eroded polygon);
    * a small domain is dropped, not merged into a neighbour: the regions of different components are disjoint here;
    * ``0 < shrink_margin_um <= cell_dist_um`` is required (``ValueError``); ``sf`` accepts a larger margin and grows
      the polygon a second time;
    * only 2-D coordinates, as in ``calculate_domain_distances``; ontology IDs in ``filter_expression`` raise
      ``NotImplementedError``.

    Returns the AnnData with ``adata.obs[output_column]`` (object: domain names, NaN outside every domain).
    """
    if "spatial" not in adata.obsm:
        raise ValueError(
            "adata.obsm['spatial'] not found. "
            "Spatial coordinates are required for domain creation."
        )
    if filter_expression is None:
        raise ValueError(
            "'filter_expression' must be provided. Examples:\n"
            "  - Ontology ID: 'CL:0000236' (B cell)\n"
            "  - Boolean expression: 'CL:0000236 & NCIT:C4349'\n"
            "  - Column equality: \"cell_type == 'B cell'\"\n"
            "  - Boolean column: 'is_tumor'"
        )
    if platform is not None:
        _get_platform_defaults(platform)        # unknown platform: ValueError

    effective_platform = platform
    if cell_dist_um is not None:
        effective_cell_dist_um = cell_dist_um
        logger.debug(f"Using user-provided cell_dist_um={cell_dist_um}")
    elif platform is None:
        detected_platform = _detect_platform(adata)
        if detected_platform is None:
            raise ValueError(
                "Could not auto-detect platform from coordinate ranges. "
                "Provide 'platform' or 'cell_dist_um' explicitly."
            )
        effective_platform = detected_platform
        effective_cell_dist_um = _get_platform_defaults(detected_platform)
        max_coord = np.max(np.abs(np.asarray(adata.obsm["spatial"])))
        logger.info(
            f"Auto-detected platform '{detected_platform}' "
            f"(max coordinate: {max_coord:.1f}), "
            f"using cell_dist_um={effective_cell_dist_um}"
        )
    else:
        effective_cell_dist_um = _get_platform_defaults(platform)
        logger.info(f"Using platform '{platform}' defaults: cell_dist_um={effective_cell_dist_um}")

    d, m = float(effective_cell_dist_um), float(shrink_margin_um)
    if not (np.isfinite(d) and d > 0):
        raise ValueError(f"cell_dist_um must be finite and > 0, got {effective_cell_dist_um}")
    if not (np.isfinite(m) and 0 < m <= d):
        raise ValueError(
            f"shrink_margin_um must satisfy 0 < shrink_margin_um <= cell_dist_um, got {shrink_margin_um} "
            f"with cell_dist_um={effective_cell_dist_um}"
        )

    adata = adata.copy() if copy else adata

    logger.info("Creating spatial domains by buffer-union-shrink on the GPU")
    logger.info(f"Evaluating filter expression: {filter_expression}")
    mask = np.asarray(_evaluate_filter_expression(filter_expression, adata), dtype=bool)
    n_target_cells = int(mask.sum())
    if n_target_cells == 0:
        raise ValueError(
            f"No cells match filter expression: '{filter_expression}'. "
            "Check that column names and values are correct."
        )
    logger.info(f"Filter expression matched {n_target_cells:,} cells")

    if domain_prefix is None:
        domain_prefix = _generate_domain_prefix(filter_expression)

    spatial_coords = np.asarray(adata.obsm["spatial"])
    if spatial_coords.ndim != 2 or spatial_coords.shape[1] < 2:
        raise ValueError(
            f"Spatial coordinates must have at least 2 columns, "
            f"got shape {spatial_coords.shape}"
        )
    if spatial_coords.shape[1] != 2:
        raise ValueError("only 2-D coordinates are supported by the MI355X path "
                         f"(adata.obsm['spatial'] has shape {spatial_coords.shape})")
    no_cells_assigned = (
        "No cells were assigned to any domain. "
        "Try relaxing filters, adjusting cell_dist_um, or setting "
        "assign_all_cells=True."
    )
    # (every domain holds target cells only in this mode: none can have more than there are)
    if assign_all_cells is False and n_target_cells <= min_target_cells_domain:
        raise ValueError(no_cells_assigned)

    xy = np.ascontiguousarray(spatial_coords, dtype=np.float64)
    targets = np.flatnonzero(mask)
    others = np.flatnonzero(~mask) if assign_all_cells else np.zeros(0, dtype=np.intp)
    ctx = _lib.default_context(device)
    # every target lies in its own component's region (the margin is positive): only the other cells are queries
    comp_t, comp_q, _ = ctx.domains(xy[targets], xy[others], d, d - m, return_clearance=False)
    rank_t, rank_q = _number_domains(comp_t, comp_q, min_target_cells_domain, min_total_cells_domain)
    n_kept = int(max(rank_t.max(initial=0), rank_q.max(initial=0)))
    if assign_all_cells is False and not rank_t.any():
        raise ValueError(no_cells_assigned)

    rank = np.zeros(xy.shape[0], dtype=np.int64)
    rank[targets] = rank_t
    rank[others] = rank_q
    names = np.array([np.nan] + [f"{domain_prefix}_{k}" for k in range(1, n_kept + 1)], dtype=object)
    adata.obs[output_column] = names[rank]
    logger.debug(f"Numbered {n_kept} domains 1-{n_kept} by assigned-cell count")

    n_domains = adata.obs[output_column].nunique()
    n_assigned = adata.obs[output_column].notna().sum()
    domains_list = adata.obs[output_column].dropna().unique().tolist()
    logger.info(
        f"Created {n_domains} domains, assigned {n_assigned:,}/{adata.n_obs:,} cells "
        f"({100 * n_assigned / adata.n_obs:.1f}%)"
    )

    if n_target_cells > 0:
        expansion_ratio = n_assigned / n_target_cells
        if expansion_ratio > domain_expansion_warn_ratio:
            logger.warning(
                f"Domain expansion ratio {expansion_ratio:.1f}x exceeds threshold "
                f"({domain_expansion_warn_ratio}x). This means {n_assigned:,} cells were "
                f"assigned to domains defined by only {n_target_cells:,} target cells. "
                "Review assign_all_cells setting if this is unexpected."
            )

    update_metadata(
        adata,
        function_name="make_spatial_domains",
        parameters={
            "filter_expression": filter_expression,
            "cell_dist_um": effective_cell_dist_um,
            "cell_dist_um_user_provided": cell_dist_um is not None,
            "platform": effective_platform,
            "platform_user_provided": platform is not None,
            "shrink_margin_um": shrink_margin_um,
            "domain_prefix": domain_prefix,
            "min_target_cells_domain": min_target_cells_domain,
            "min_total_cells_domain": min_total_cells_domain,
            "output_column": output_column,
            "assign_all_cells": assign_all_cells,
            "domain_expansion_warn_ratio": domain_expansion_warn_ratio,
        },
        outputs={
            "obs": output_column,
            "n_domains": n_domains,
            "n_cells_assigned": int(n_assigned),
            "n_target_cells": int(n_target_cells),
            "domains": domains_list,
        },
    )
    return adata


def get_domain_summary(adata, domain_column: str = "spatial_domain") -> pd.DataFrame:
    """Per domain: ``domain, n_cells, percent`` (of all cells, unassigned included), ``centroid_x, centroid_y``;
    largest domain first (DM:735-792).  Host arithmetic."""
    if domain_column not in adata.obs.columns:
        raise ValueError(
            f"Column '{domain_column}' not found in adata.obs. "
            f"Available columns: {list(adata.obs.columns)}"
        )
    if "spatial" not in adata.obsm:
        raise ValueError(
            "adata.obsm['spatial'] not found. "
            f"Available keys: {list(adata.obsm.keys())}"
        )
    spatial = np.asarray(adata.obsm["spatial"])
    domains = adata.obs[domain_column]
    summaries = []
    for domain in domains.dropna().unique():
        mask = domains == domain
        n_cells = mask.sum()
        coords = spatial[mask.values]
        summaries.append({
            "domain": domain,
            "n_cells": n_cells,
            "percent": 100 * n_cells / len(domains),
            "centroid_x": coords[:, 0].mean(),
            "centroid_y": coords[:, 1].mean(),
        })
    return pd.DataFrame(summaries).sort_values("n_cells", ascending=False)
