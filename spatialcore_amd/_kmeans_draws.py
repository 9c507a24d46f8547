"""The random stream of sklearn's k-means++ seeding, drawn on the host for ``Context.kmeans``: shared by identify_niches,
gaussian_mixture, harmony_integrate and classify_by_threshold."""

from __future__ import annotations

import numpy as np


def kmeans_draws(random_state, n_init: int, n_clusters: int) -> np.ndarray:
    """Every draw of sklearn's k-means++ over ``n_init`` runs of ONE ``check_random_state(random_state)``: per run the
    ``random_sample()`` of the first centre's ``choice`` and ``uniform(size=L)`` for each later centre,
    L = 2 + int(log(K)).  The stream does not depend on the data, so it is drawn here up front."""
    if random_state is None:
        rs = np.random.mtrand._rand
    elif isinstance(random_state, np.random.RandomState):
        rs = random_state
    else:
        rs = np.random.RandomState(random_state)
    L = 2 + int(np.log(n_clusters))
    out = np.empty((n_init, 1 + (n_clusters - 1) * L), dtype=np.float64)
    for r in range(n_init):
        out[r, 0] = rs.random_sample()
        for c in range(n_clusters - 1):
            out[r, 1 + c * L:1 + (c + 1) * L] = rs.uniform(size=L)
    return out
