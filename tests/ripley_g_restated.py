"""Ripley's G first-contact counts restated twice, independently of the device code (test infrastructure).

``count[a, b, j]`` = number of cells i of type a with at least one OTHER cell i' != i of type b with
``fl(fl(dx dx) + fl(dy dy)) <= fl(r_j r_j)`` -- cumulative in j, not symmetric (include/spatialcore_hip.h, N11).

* ``brute_counts_g``: on ``ripley_restated.pair_list`` (all n^2 distances, the definition read literally): per
  (cell, type) the minimum radius index over the cell's pairs, a histogram of those minima, then the cumulative sum.
* ``scipy_counts_g``: one ``cKDTree`` per type b, ``query(k=2 if a == b else 1)`` for the cells of type a; the squared
  distance to the neighbour the tree returns is recomputed as ``dx * dx + dy * dy`` and compared with ``r * r``, so the
  predicate has the definition's bits whatever the tree's own arithmetic (an equidistant other neighbour under ties gives
  the same bits).  Shares nothing with the brute force but the input.
tests/test_cpu_ripley_g.py pins the two against each other before the GPU is asked anything.
"""
import numpy as np

from ripley_restated import pair_list


def counts_g_from_pairs(pairs, codes, n_types, n_radii):
    rows, cols, bins = pairs
    codes = np.asarray(codes, dtype=np.int64)
    first = np.full((codes.size, n_types), n_radii, dtype=np.int64)      # per (cell, type): index of the nearest one's radius
    np.minimum.at(first, (rows, codes[cols]), bins)
    hist = np.zeros((n_types, n_types, n_radii + 1), dtype=np.int64)
    np.add.at(hist, (np.repeat(codes, n_types), np.tile(np.arange(n_types), codes.size), first.ravel()), 1)
    return np.cumsum(hist[:, :, :n_radii], axis=2)


def brute_counts_g(coords, codes, n_types, radii, block=1024):
    """(T, T, R) int64: the definition read literally."""
    return counts_g_from_pairs(pair_list(coords, radii, block), codes, n_types, len(radii))


def scipy_counts_g(coords, codes, n_types, radii):
    """(T, T, R) int64 by scipy's nearest-neighbour queries, one tree per type."""
    from scipy.spatial import cKDTree

    xy = np.ascontiguousarray(coords, dtype=np.float64)
    codes = np.asarray(codes)
    radii = np.asarray(radii, dtype=np.float64)
    r2 = radii * radii
    out = np.zeros((n_types, n_types, radii.size), dtype=np.int64)
    members = [np.flatnonzero(codes == t) for t in range(n_types)]
    trees = [cKDTree(xy[m]) if m.size else None for m in members]
    for a in range(n_types):
        for b in range(n_types):
            k = 2 if a == b else 1
            if members[a].size == 0 or trees[b] is None or members[b].size < k:
                continue
            _, idx = trees[b].query(xy[members[a]], k=k)
            nb = xy[members[b]][idx[:, 1] if k == 2 else idx]
            dx = xy[members[a], 0] - nb[:, 0]
            dy = xy[members[a], 1] - nb[:, 1]
            d2 = dx * dx
            d2 += dy * dy
            out[a, b] = (d2[:, None] <= r2[None, :]).sum(axis=0)
    return out


def null_tables_g(coords, codes, n_types, radii, perms):
    """(P, T, T, R): the brute-force table of ``codes[perm_p]`` for every row of ``perms``."""
    codes = np.asarray(codes)
    pairs = pair_list(coords, radii)
    return np.stack([counts_g_from_pairs(pairs, codes[p], n_types, len(radii)) for p in perms])
