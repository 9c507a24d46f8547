"""EXTENSION (not in the reference): the other two members of the LISA family on local Moran's pipeline.

``local_getis_ord`` -- Getis-Ord Gi / Gi* hot and cold spots -- and ``local_gearys_c`` -- local Geary's C -- share with
``local_morans_i`` the float32 z-scores, the row-sequential lag, the batches of genes, the ONE numpy-exact permutation
stream and the histogram -> lookup-table -> classify finalisation.  What differs is the per-cell statistic and the count:
both tails are counted, ``ge = #(sim >= obs)`` and ``le = #(sim <= obs)``, and the permutation level is
``m = min(ge, le)``, ``p = float32((m + 1) / (P + 1))``.  The textbook fold ``min(c, P - c)`` of a one-sided count calls a
cell whose null mostly EQUALS the observed value significant; on count data that is a fifth of all cells.
"""

from __future__ import annotations

from typing import List, Optional, Union

from spatialcore_amd._logging import get_logger
from spatialcore_amd.spatial.autocorrelation import _local_driver

logger = get_logger("spatial.local_stats")

MAX_PERMUTATIONS = 65535      # the two tails of a cell share one 32-bit word on the device
SPOT_CODES = {"NS": 0, "hot": 1, "cold": 2}          # name -> int8 code (string keys: uns must survive an h5ad round trip)
GEARY_CODES = {"NS": 0, "high-high": 1, "low-low": 2, "other-positive": 3, "negative": 4}


def local_getis_ord(
    adata,
    genes: Optional[Union[str, List[str]]] = None,
    layer: Optional[str] = None,
    spatial_key: str = "spatial",
    n_neighbors: int = 6,
    star: bool = True,
    n_permutations: int = 10,
    fdr_correction: str = "fdr_bh",
    alpha: float = 0.05,
    seed: int = 0,
    batch_size: int = 100,
    key_added: str = "local_getis",
    copy: bool = False,
    *,
    device: int = 0,
):
    """Getis-Ord hot and cold spots per cell and gene: Gi* (``star=True``, the cell is its own neighbour: k + 1 edges of
    weight float32(1 / (k + 1))) or Gi (Ord & Getis 1995) on the row-normalised kNN graph.

    Outputs: ``obsm[{key}_G|_z|_lag|_p|_p_adj]`` float32 ``(n_cells, n_genes)``, ``obsm[{key}_spot]`` int8 (1 hot: G > 0,
    2 cold: G < 0, 0 not significant), ``uns[{key}_params]``.  ``G`` is the standardised statistic.  The p-value is that
    of the neighbourhood sum ``lag_i`` under this package's FULL-permutation scheme -- every permutation relabels all
    cells, the cell itself included, as in ``local_morans_i`` -- not esda's conditional scheme, which holds the cell's own
    value fixed.  Both tails are counted, ``p = float32((min(ge, le) + 1) / (P + 1))``, so a permuted sum that ties the
    observed one never counts as evidence (see the module docstring).
    """
    return _local_driver(adata, "getis", "Getis-Ord Gi*" if star else "Getis-Ord Gi", "local_getis_ord", "G", "spot", "classes",
                         logger, genes, layer, spatial_key, n_neighbors, bool(star), n_permutations, fdr_correction, alpha,
                         seed, batch_size, key_added, copy, device, max_permutations=MAX_PERMUTATIONS,
                         extra_params={"class_codes": dict(SPOT_CODES), "star": bool(star)}, extra_recorded={"star": bool(star)})


def local_gearys_c(
    adata,
    genes: Optional[Union[str, List[str]]] = None,
    layer: Optional[str] = None,
    spatial_key: str = "spatial",
    n_neighbors: int = 6,
    n_permutations: int = 10,
    fdr_correction: str = "fdr_bh",
    alpha: float = 0.05,
    seed: int = 0,
    batch_size: int = 100,
    key_added: str = "local_geary",
    copy: bool = False,
    *,
    device: int = 0,
):
    """Local Geary's C per cell and gene on the row-normalised kNN graph: ``C_i = sum_e w_e (z_i - z_e)^2`` in float32.

    Outputs: ``obsm[{key}_C|_z|_lag|_p|_p_adj]`` float32 ``(n_cells, n_genes)``, ``obsm[{key}_cluster]`` int8 by GeoDa's
    convention against the null expectation ``E_i = 2n / (n - 1) * sum_e w_e`` of the full-permutation scheme: ``C < E``
    positive association (1 high-high, 2 low-low, 3 other positive), ``C > E`` 4 negative, 0 not significant;
    ``uns[{key}_params]``.  Both tails are counted, ``p = float32((min(ge, le) + 1) / (P + 1))``.
    """
    return _local_driver(adata, "geary", "Local Geary's C", "local_gearys_c", "C", "cluster", "classes", logger, genes, layer,
                         spatial_key, n_neighbors, False, n_permutations, fdr_correction, alpha, seed, batch_size, key_added,
                         copy, device, max_permutations=MAX_PERMUTATIONS, extra_params={"class_codes": dict(GEARY_CODES)})
