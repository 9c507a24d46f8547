"""Ripley's K pair counts restated twice, independently of the device code (test infrastructure).

``count[a, b, j]`` = number of ORDERED pairs (i, i'), i != i', type(i) = a, type(i') = b, with
``fl(fl(dx dx) + fl(dy dy)) <= fl(r_j r_j)`` -- cumulative in j (include/spatialcore_hip.h, N6).

* ``brute_counts``: blocked brute force in numpy, the definition read literally (numpy rounds ``dx * dx``, ``dy * dy``
  and their sum separately: there is no fused multiply-add in an elementwise expression of temporaries).
* ``scipy_counts``: per-type ``cKDTree`` + ``count_neighbors`` -- an exact cumulative pair count by a tree code that
  shares nothing with the brute force but the input.
tests/test_cpu_ripley.py pins the two against each other before the GPU is asked anything.
"""
import numpy as np


def pair_list(coords, radii, block=1024):
    """Every ordered pair (i, i'), i != i', within the largest radius, and the index of the smallest radius containing
    it: all n^2 squared distances in row blocks, ``searchsorted(side="left")`` in ``fl(r^2)``."""
    xy = np.ascontiguousarray(coords, dtype=np.float64)
    radii = np.asarray(radii, dtype=np.float64)
    r2 = radii * radii
    n = xy.shape[0]
    x, y = xy[:, 0], xy[:, 1]
    rows, cols, bins = [], [], []
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        dx = x[i0:i1, None] - x[None, :]
        dy = y[i0:i1, None] - y[None, :]
        d2 = dx * dx
        d2 += dy * dy
        d2[np.arange(i1 - i0), np.arange(i0, i1)] = np.inf          # i != i'
        ii, jj = np.nonzero(d2 <= r2[-1])
        rows.append(i0 + ii)
        cols.append(jj)
        bins.append(np.searchsorted(r2, d2[ii, jj], side="left"))   # the smallest j with d2 <= r2[j]
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(bins)


def counts_from_pairs(pairs, codes, n_types, n_radii):
    rows, cols, bins = pairs
    codes = np.asarray(codes, dtype=np.int64)
    hist = np.zeros((n_types, n_types, n_radii), dtype=np.int64)
    np.add.at(hist, (codes[rows], codes[cols], bins), 1)
    return np.cumsum(hist, axis=2)


def brute_counts(coords, codes, n_types, radii, block=1024):
    """(T, T, R) int64: the definition read literally."""
    return counts_from_pairs(pair_list(coords, radii, block), codes, n_types, len(radii))


def scipy_counts(coords, codes, n_types, radii, pairs=None):
    """(T, T, R) int64 by scipy's exact tree counts: ``count_neighbors`` of the type-a tree against the type-b tree
    (cumulative, closed balls), minus the n_a self pairs on the diagonal.  ``pairs``: only these (a, b) entries (and
    their mirror images) are filled, the rest stays -1."""
    from scipy.spatial import cKDTree

    xy = np.ascontiguousarray(coords, dtype=np.float64)
    codes = np.asarray(codes)
    radii = np.asarray(radii, dtype=np.float64)
    out = np.full((n_types, n_types, radii.size), -1, dtype=np.int64)
    members = [np.flatnonzero(codes == t) for t in range(n_types)]
    trees = {}

    def tree(t):
        if t not in trees:
            trees[t] = cKDTree(xy[members[t]]) if members[t].size else None
        return trees[t]

    todo = pairs if pairs is not None else [(a, b) for a in range(n_types) for b in range(a, n_types)]
    for a, b in todo:
        ta, tb = tree(a), tree(b)
        if ta is None or tb is None:
            c = np.zeros(radii.size, dtype=np.int64)
        else:
            c = np.asarray(ta.count_neighbors(tb, radii), dtype=np.int64)
            if a == b:
                c = c - members[a].size
        out[a, b] = c
        out[b, a] = c
    return out


def null_tables(coords, codes, n_types, radii, perms):
    """(P, T, T, R): the brute-force table of ``codes[perm_p]`` for every row of ``perms``."""
    codes = np.asarray(codes)
    pairs = pair_list(coords, radii)
    return np.stack([counts_from_pairs(pairs, codes[p], n_types, len(radii)) for p in perms])
