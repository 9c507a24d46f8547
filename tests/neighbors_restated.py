"""numpy restatement of sc_knn_dense_gram's filter (sc_neighbors.hip) and the input recipes of its tests.

The filter's dot products come from the matrix cores in an order the restatement does not know, so its ``lo`` may differ
from the device's in the last bits; what is pinned is what does not depend on them: the bound ``|s - d2_dev| <= E``, the
final lists (``diffusion_restated.knn`` is the truth) and the certification counts on recipes whose margins are checked
here (tests/test_cpu_neighbors.py)."""
import numpy as np

import diffusion_restated as R

SLACK_DEFAULT = 8          # NB_SLACK_DEFAULT
CERT_SEED = 1              # pca_like(3000, 50, CERT_SEED): the sample of the certification counts (test_cpu_neighbors.py checks
                           # its margins: a margin is the gap between a row's k-th and L-th neighbour, a property of the sample)
TINY = 2.0 ** -1000


def padded(d):
    return -(-d // 8) * 8


def c_e(d):
    """c_E = 4 dp + 32 of the padded width."""
    return 4 * padded(d) + 32


def norms(X):
    """n_i = sum_c x_ic^2 in column order from the c = 0 term."""
    X = np.asarray(X, dtype=np.float64)
    s = X[:, 0] * X[:, 0]
    for c in range(1, X.shape[1]):
        s = s + X[:, c] * X[:, c]
    return s


def gram(q, X, order="matmul"):
    """q X^T in one of three summation orders: BLAS, reversed columns one at a time, pairwise halves."""
    q, X = np.asarray(q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    if order == "matmul":
        return q @ X.T
    if order == "reversed":
        g = np.zeros((q.shape[0], X.shape[0]))
        for c in range(X.shape[1] - 1, -1, -1):
            g = g + q[:, None, c] * X[None, :, c]
        return g
    if order == "pairwise":
        def rec(lo, hi):
            if hi - lo == 1:
                return q[:, None, lo] * X[None, :, lo]
            mid = (lo + hi) // 2
            return rec(lo, mid) + rec(mid, hi)
        return rec(0, X.shape[1])
    raise ValueError(order)


def bounds(X, rows, order="matmul", nrm=None):
    """(s, E, lo) of the queries ``rows`` against every cell: s = (n_i + n_j) - 2 g, E = c_E 2^-52 (n_i + n_j) + 2^-1000."""
    X = np.asarray(X, dtype=np.float64)
    nrm = norms(X) if nrm is None else nrm
    t = nrm[rows][:, None] + nrm[None, :]
    s = t - 2.0 * gram(X[rows], X, order)
    E = (c_e(X.shape[1]) * 2.0 ** -52) * t + TINY
    return s, E, s - E


def direct(X, rows):
    """d2_dev of the queries ``rows`` against every cell, in the direct form's order."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    r = np.repeat(np.asarray(rows), n)
    c = np.tile(np.arange(n), len(rows))
    return R.pair_d2(X, r, c).reshape(len(rows), n)


def filtered_knn(X, k, slack=0, order="matmul", block=256):
    """The five steps: (idx, d2, certified, margin).  ``certified`` marks the rows the filter certified; the others went
    through the fallback (the exact search).  ``margin[i]`` = lo_(L) - D of row i (inf where fewer than L were kept)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    L = k + (slack if slack else SLACK_DEFAULT)
    nrm = norms(X)
    idx = np.empty((n, k), dtype=np.int32)
    d2 = np.empty((n, k))
    certified = np.zeros(n, dtype=bool)
    margin = np.full(n, np.inf)
    for b in range(0, n, block):
        rows = np.arange(b, min(b + block, n))
        _, _, lo = bounds(X, rows, order, nrm)
        lo[np.arange(rows.size), rows] = np.inf
        m = min(L, n - 1)
        kept = np.argsort(lo, axis=1, kind="stable")[:, :m]          # the m smallest (lo, j)
        exact = R.pair_d2(X, np.repeat(rows, m), kept.ravel()).reshape(rows.size, m)
        best = np.lexsort((kept, exact), axis=1)[:, :k]              # the k smallest (d2, j) among them
        idx[rows] = np.take_along_axis(kept, best, axis=1)
        d2[rows] = np.take_along_axis(exact, best, axis=1)
        if m < L:
            certified[rows] = True
        else:
            lo_L = np.take_along_axis(lo, kept[:, -1:], axis=1)[:, 0]
            margin[rows] = lo_L - d2[rows, k - 1]
            certified[rows] = d2[rows, k - 1] < lo_L
    return idx, d2, certified, margin


def with_fallback(X, k, idx, d2, certified):
    """The uncertified rows replaced by the exact search's."""
    if certified.all():
        return idx, d2
    ti, td = R.knn(X, k)
    idx, d2 = idx.copy(), d2.copy()
    idx[~certified], d2[~certified] = ti[~certified], td[~certified]
    return idx, d2


# ---- recipes ----------------------------------------------------------------------------------------------------------
def pca_like(n, d=50, seed=0):
    """Gaussian columns whose standard deviation falls from 10 to 0.5: the scores of a PCA."""
    return np.random.default_rng(seed).standard_normal((n, d)) * np.linspace(10.0, 0.5, d)


def lattice(n, seed=0):
    """Points of {0..3}^33: integer squared distances, many ties, a few exact duplicates."""
    return np.random.default_rng(seed).integers(0, 4, size=(n, 33)).astype(np.float64)


def lattice_wide(n, seed=0):
    """``lattice`` with seven columns of zeros appended: the same distances and ties in 40 columns."""
    return np.hstack([lattice(n, seed), np.zeros((n, 7))])


def duplicates(distinct=100, copies=40, d=50, seed=0):
    """Every cell 40 times: the 39 nearest neighbours of a cell are at distance zero."""
    return np.tile(pca_like(distinct, d, seed), (copies, 1))


def far_copies(d, m, dtype=np.float64):
    """pca_like(1000, d, CERT_SEED) and, far from it, ``m`` copies of the point (1000, 0, .., 0).  A point repeated more
    than L = k + slack times has D = 0 and lo_(L) <= 0, so exactly the copies miss the certificate: the fallback's list
    holds ``m`` rows, the last ``m``."""
    far = np.zeros((m, d))
    far[:, 0] = 1000.0
    return np.vstack([pca_like(1000, d, CERT_SEED), far]).astype(dtype)


# (d, dtype, k, slack, m) of far_copies: the listed-row count at the edges of the fallback scan's block of 64 queries
# (DF_QB_L).  The fewest rows that can be listed (m = L + 1, at k = 2 and at k = 15); one row short of a block, a block, one
# and two blocks and a row (n = 1063 leaves a last candidate split of 7 < k: the merge sees sentinels); the LDS scan at the
# padded widths 8 and 40, which the direct search never gives it; float32 input.
LISTED_EDGE = [
    (50, np.float64, 2, 1, 4), (50, np.float64, 15, 0, 24),
    (50, np.float64, 15, 0, 63), (50, np.float64, 15, 0, 64), (50, np.float64, 15, 0, 65), (50, np.float64, 15, 0, 129),
    (3, np.float64, 15, 0, 65), (33, np.float64, 15, 0, 65), (50, np.float32, 15, 0, 65),
]
LISTED_EDGE_IDS = [f"d{d}-{np.dtype(t).name}-k{k}-slack{s}-m{m}" for d, t, k, s, m in LISTED_EDGE]


def recipes(n):
    """name -> features: the families of the bound and of the rule."""
    base = pca_like(n, 50, 1)
    return {
        "pca_like": base,
        "offset_1e3": base + 1e3,
        "offset_1e6": base + 1e6,
        "float32": base.astype(np.float32),
        "traj": R.traj(n, 40, 1)[0],
        "lattice": lattice(n, 2),
        "tiny": base * 2.0 ** -520,
        "huge": base * 2.0 ** 490,
    }
