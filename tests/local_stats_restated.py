"""Getis-Ord Gi / Gi* and local Geary's C restated, independently of the device code (test infrastructure; numpy only).

Neither statistic is in the reference, so the package defines them and this file is the executable
form of that definition: float32 z and lag from ``local_restated`` (pinned to the reference there), the permuted sums
with the observed sum's own products and order so that a tie is a tie, both tails counted.

* ``getis_values``: the standardised G in float64 from float32 z / lag / weights, stored as float32.
* ``geary_values``: C_i = sum_e fl(w_e fl(d d)), d = fl(z_i - z_e), float32 in edge order.
* ``two_tail_counts``: (ge, le) per cell and gene over a table of permutations.
* ``geary_expectation``: the null expectation of C_i under the full-permutation scheme, float64.
* ``spot_classes`` / ``geary_classes``: the int8 classes.
tests/test_cpu_local_stats.py pins these to the textbook formulas before tests/test_gpu_local_stats.py asks the GPU.
"""
import numpy as np

from local_restated import (count_matrix, knn_csr, knn_weight, local_moran_arrays, lognorm_matrix, row_sequential,  # noqa: F401
                            thinned_csr, uniform_coords)

STATS = ("getis", "getis_star", "geary")


def star_lists(idx):
    """Neighbour lists with the cell itself in front: what a (k + 1)-neighbour search that includes self returns."""
    idx = np.asarray(idx, dtype=np.int32)
    return np.concatenate([np.arange(idx.shape[0], dtype=np.int32)[:, None], idx], axis=1)


def row_weight_sums(indptr, indices, w32):
    """(W, S1) float64 per row: sums of (double)w_e and of (double)w_e (double)w_e over the edges in stored order."""
    w = np.asarray(w32, dtype=np.float32).astype(np.float64)
    ones = np.ones(len(indptr) - 1, dtype=np.float64)
    return row_sequential(indptr, indices, w, ones), row_sequential(indptr, indices, w * w, ones)


def getis_values(indptr, indices, w32, z, lag, star):
    """float32 (n, G).  Gi*: lag / sqrt((n S1 - W^2) / (n - 1)).  Gi (Ord & Getis 1995 in z units): mi = -z / (n - 1),
    vi = (n - z^2) / (n - 1) - mi^2, (lag - W mi) / (sqrt(vi) sqrt(((n - 1) S1 - W^2) / (n - 2))).  float64, every
    operation rounded once, in the order written; 0 where the denominator is 0 or not finite."""
    z, lag = np.asarray(z, dtype=np.float32).astype(np.float64), np.asarray(lag, dtype=np.float32).astype(np.float64)
    n = float(z.shape[0])
    W, S1 = row_weight_sums(indptr, indices, w32)
    W, S1 = W[:, None], S1[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        if star:
            den = np.sqrt((n * S1 - W * W) / (n - 1.0)) * np.ones_like(z)
            num = lag
        else:
            mi = -z / (n - 1.0)
            vi = (n - z * z) / (n - 1.0) - mi * mi
            den = np.sqrt(vi) * np.sqrt(((n - 1.0) * S1 - W * W) / (n - 2.0))
            num = lag - W * mi
        ok = np.isfinite(den) & (den != 0)
        G = np.where(ok, num / np.where(ok, den, 1.0), 0.0)
    return G.astype(np.float32)


def geary_values(indptr, indices, w32, Y):
    """C[i] = (((0 + w_e0 d0 d0) + w_e1 d1 d1) + ...), d = Y[i] - Y[c_e], in float32: difference, square, product and sum
    rounded separately, edges in stored order.  Y is (n, G)."""
    Y = np.asarray(Y, dtype=np.float32)
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    w = np.asarray(w32, dtype=np.float32)
    deg = np.diff(indptr)
    s = np.zeros(Y.shape, dtype=np.float32)
    for j in range(int(deg.max(initial=0))):
        rows = np.flatnonzero(deg > j)
        e = indptr[rows] + j
        d = Y[rows] - Y[indices[e]]
        s[rows] = s[rows] + w[e][:, None] * (d * d)
    return s


def simulated(stat, indptr, indices, w32, Y):
    """The value the counts compare: the neighbourhood sum (both Getis-Ord forms) or C, on the (permuted) matrix Y."""
    if stat == "geary":
        return geary_values(indptr, indices, w32, Y)
    return row_sequential(indptr, indices, np.asarray(w32, dtype=np.float32), np.asarray(Y, dtype=np.float32))


def two_tail_counts(stat, indptr, indices, w32, Z32, obs, perms):
    """(ge, le) int32 (n, G): #{p : sim_p >= obs} and #{p : sim_p <= obs}, sim_p = simulated(Z32[perm_p]); signed."""
    Z32 = np.asarray(Z32, dtype=np.float32)
    obs = np.asarray(obs, dtype=np.float32)
    ge, le = np.zeros(Z32.shape, dtype=np.int32), np.zeros(Z32.shape, dtype=np.int32)
    for perm in np.asarray(perms):
        sim = simulated(stat, indptr, indices, w32, Z32[perm])
        ge += sim >= obs
        le += sim <= obs
    return ge, le


def geary_expectation(indptr, indices, w32):
    """E[i] = (2 n / (n - 1)) * sum_{e : c_e != i} w_e, float64, the sum in stored order."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    w = np.asarray(w32, dtype=np.float32).astype(np.float64) * (np.asarray(indices) != rows)
    return (2.0 * n / (n - 1.0)) * row_sequential(indptr, indices, w, np.ones(n, dtype=np.float64))


def _not_significant(q, padj, alpha, zero):
    if padj is not None:
        q[np.asarray(padj, dtype=np.float32) >= np.float32(alpha)] = 0
    q[:, np.asarray(zero, dtype=bool)] = 0
    return q


def spot_classes(G, padj, alpha, zero):
    """int8: 1 hot (G > 0), 2 cold (G < 0); 0 where padj >= alpha (float32; None: no filter), flagged, or G == 0."""
    G = np.asarray(G)
    q = np.zeros(G.shape, dtype=np.int8)
    q[G > 0] = 1
    q[G < 0] = 2
    return _not_significant(q, padj, alpha, zero)


def geary_classes(C, E, z, lag, padj, alpha, zero):
    """int8, GeoDa's convention: C < E 1 high-high (z > 0, lag > 0), 2 low-low (z < 0, lag < 0), 3 other positive;
    C > E 4 negative; 0 where padj >= alpha, flagged, or C == E.  C float32 compared with E float64 in float64."""
    C, z, lag = np.asarray(C, dtype=np.float64), np.asarray(z), np.asarray(lag)
    E = np.asarray(E, dtype=np.float64)[:, None]
    q = np.zeros(C.shape, dtype=np.int8)
    pos = C < E
    q[pos] = 3
    q[pos & (z > 0) & (lag > 0)] = 1
    q[pos & (z < 0) & (lag < 0)] = 2
    q[C > E] = 4
    return _not_significant(q, padj, alpha, zero)


def stat_graph(stat, idx, k):
    """The row-normalised kNN CSR of a statistic from plain neighbour lists: Gi* adds the self edge (k + 1 edges of
    float32(1 / (k + 1)), the self edge in its place in the ascending row)."""
    if stat == "getis_star":
        return knn_csr(star_lists(idx), knn_weight(k + 1))
    return knn_csr(idx, knn_weight(k))


def restated(stat, X, graph, perms):
    """Everything sc_local_stat returns, from the matrix X, a (indptr, indices, float64-held float32 weights) graph and a
    table of permutations."""
    ip, ix, w = graph
    w32 = np.asarray(w).astype(np.float32)
    assert (w32.astype(np.float64) == w).all()
    z, lag, _, zero = local_moran_arrays(X, X.dtype.type, ip, ix, w32)
    if stat == "geary":
        val = obs = geary_values(ip, ix, w32, z)
    else:
        val, obs = getis_values(ip, ix, w32, z, lag, stat == "getis_star"), lag
    ge, le = two_tail_counts(stat, ip, ix, w32, z, obs, perms)
    return {"z": z, "lag": lag, "stat": val, "ge": ge, "le": le, "zero_var": zero}
