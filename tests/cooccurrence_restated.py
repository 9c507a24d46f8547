"""Co-occurrence by distance restated in plain numpy, independently of the device code (test infrastructure).

Three parts, each the definition of include/spatialcore_hip.h (N9) read literally:

* ``thresholds``: the rule for an integer ``interval`` -- ``s = x + y``, ``a`` and ``b`` the two cells of smallest ``s``
  (stable order), ``c`` the first cell of largest ``s``, ``linspace(dist(a, b), dist(a, c) / 2, m)`` in float64.
* ``brute_counts``: ``count[a, b, j]`` = ordered pairs (i, i'), i != i', of types (a, b) whose
  ``d2 = fl(fl(dx dx) + fl(dy dy))`` has ``j`` as the smallest index with ``d2 <= fl(t_j t_j)``; pairs beyond the last
  threshold are dropped.  All n^2 squared distances in row blocks (numpy rounds ``dx * dx``, ``dy * dy`` and their sum
  separately), ``searchsorted(T2, d2, side="left")``, the diagonal removed.  NOT cumulative.
* ``occ``: ``co[a, b] * co.sum() / (co[a, :].sum() * co[:, b].sum())`` per annulus ``co = count[:, :, r]``, r >= 1,
  float64 on the integers, stored as float32, ``0 / 0`` = NaN.
tests/test_cpu_cooccurrence.py pins the counts against scipy's tree counts before the GPU is asked anything.
"""
import numpy as np


def thresholds(coords, m):
    xy = np.asarray(coords, dtype=np.float64)
    s = xy[:, 0] + xy[:, 1]
    a, b = np.argsort(s, kind="stable")[:2]
    c = int(np.argmax(s))
    ab, ac = xy[a] - xy[b], xy[a] - xy[c]
    t_min = np.sqrt(ab[0] * ab[0] + ab[1] * ab[1])
    t_max = np.sqrt(ac[0] * ac[0] + ac[1] * ac[1]) / 2
    return np.linspace(t_min, t_max, m)


def brute_counts(coords, codes, n_types, thr, block=1024):
    """(T, T, len(thr)) int64, and the number of ordered pairs beyond the last threshold."""
    xy = np.ascontiguousarray(coords, dtype=np.float64)
    codes = np.asarray(codes, dtype=np.int64)
    thr = np.asarray(thr, dtype=np.float64)
    t2 = thr * thr
    n, nb = xy.shape[0], thr.size
    x, y = xy[:, 0], xy[:, 1]
    flat = np.zeros(n_types * n_types * (nb + 1), dtype=np.int64)     # one more bin: the dropped pairs
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        dx = x[i0:i1, None] - x[None, :]
        dy = y[i0:i1, None] - y[None, :]
        d2 = dx * dx
        d2 += dy * dy
        bins = np.searchsorted(t2, d2.ravel(), side="left").reshape(d2.shape)    # the smallest j with d2 <= t2[j]; nb: none
        key = (codes[i0:i1, None] * n_types + codes[None, :]) * (nb + 1) + bins
        key[np.arange(i1 - i0), np.arange(i0, i1)] = -1                            # i != i'
        key = key.ravel()
        flat += np.bincount(key[key >= 0], minlength=flat.size)
    table = flat.reshape(n_types, n_types, nb + 1)
    return table[:, :, :nb].copy(), int(table[:, :, nb].sum())


def occ(count):
    """(T, T, R) float32 from the (T, T, R + 1) table."""
    count = np.asarray(count, dtype=np.int64)
    T, _, nb = count.shape
    out = np.empty((T, T, nb - 1), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(1, nb):
            co = count[:, :, r].astype(np.float64)
            out[:, :, r - 1] = co * co.sum() / (co.sum(axis=1)[:, None] * co.sum(axis=0)[None, :])
    return out
