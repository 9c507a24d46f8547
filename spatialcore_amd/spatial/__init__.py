"""MI355X-native spatial statistics: the hot path of ``spatialcore.spatial``
(reference src/spatialcore/spatial/__init__.py:11-52) behind the same function names."""

from spatialcore_amd.spatial.autocorrelation import (
    build_spatial_weights,
    lees_l,
    lees_l_local,
    local_morans_i,
    morans_i,
)
from spatialcore_amd.spatial.distance import calculate_domain_distances, get_distance_matrix
from spatialcore_amd.spatial.local_stats import local_gearys_c, local_getis_ord
from spatialcore_amd.spatial.domains import get_domain_summary, make_spatial_domains
from spatialcore_amd.spatial.hops import aggregate_neighbors
from spatialcore_amd.spatial.markers import rank_genes_groups
from spatialcore_amd.spatial.neighborhoods import (
    co_occurrence,
    compute_neighborhood_profile,
    identify_niches,
    ligrec,
    neighborhood_enrichment,
    ripley_g,
    ripley_k,
)

__all__ = [
    "morans_i",
    "local_morans_i",
    "local_getis_ord",  # extension: not in the reference
    "local_gearys_c",  # extension: not in the reference
    "lees_l",
    "lees_l_local",
    "build_spatial_weights",
    "compute_neighborhood_profile",
    "identify_niches",
    "neighborhood_enrichment",  # extension: not in the reference
    "ripley_k",  # extension: not in the reference
    "co_occurrence",  # extension: squidpy's function, not in the reference
    "ligrec",  # extension: squidpy's function, not in the reference
    "ripley_g",  # extension: not in the reference
    "aggregate_neighbors",  # extension: cellcharter's function, not in the reference
    "make_spatial_domains",
    "get_domain_summary",
    "calculate_domain_distances",
    "get_distance_matrix",
    "rank_genes_groups",  # extension: scanpy's function, not in the reference
]
