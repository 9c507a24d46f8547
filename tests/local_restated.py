"""Local Moran's I and local Lee's L restated, independently of the device code (test infrastructure; numpy only).

The reference standardises in float32, takes ``lag = W32 @ Z32`` with scipy's row-sequential accumulation (every
product and every sum rounded on its own, edges in the row's stored order) and counts, per cell and gene, the
permutations with ``|I_perm| >= |I|``.  On count data a tenth of those comparisons are exact ties, so the restatement
keeps the reference's rounding everywhere and the device is compared with it bit for bit.

* ``row_sequential``: the sparse product with scipy's summation order and rounding.
* ``local_moran_arrays``: z, lag, I and the zero-variance mask (mean and mean of squares in numpy's summation order).
* ``local_moran_counts``: the per-cell permutation counts of local Moran, float32.
* ``lee_local_counts``: the per-cell permutation counts of local Lee, float64 sums stored as float32.
* ``count_hist``, ``classify``: the histogram of counts per gene and the LISA quadrants.
The input builders at the end are shared by tests/test_cpu_local_restated.py, which pins the restatement against
scipy, the oracle and the goldens before the GPU is asked anything, and tests/test_gpu_local.py.
"""
import numpy as np


def row_sequential(indptr, indices, w, Y):
    """s[i] = (((0 + w_e0 Y[c_e0]) + w_e1 Y[c_e1]) + ...) over the edges of row i in their stored order, in the dtype
    of Y: product and sum are rounded separately (numpy has no fused multiply-add in an expression of temporaries).
    Y is (n,) or (n, G); empty rows give 0."""
    Y = np.asarray(Y)
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    w = np.asarray(w).astype(Y.dtype)
    deg = np.diff(indptr)
    s = np.zeros(Y.shape, dtype=Y.dtype)
    for j in range(int(deg.max(initial=0))):
        rows = np.flatnonzero(deg > j)
        e = indptr[rows] + j
        we = w[e] if Y.ndim == 1 else w[e][:, None]
        term = we * Y[indices[e]]
        s[rows] = s[rows] + term
    return s


def column_moments(X, dtype):
    """(mean, mean of squares) per column as the reference's sparse ``.mean(axis=0)`` gives them, in ``dtype``: the
    stored (non-zero) entries of the column in cell order, each times dtype(1 / n), the first one plus numpy's
    pairwise sum of the rest (``np.add.reduce``)."""
    X = np.asarray(X, dtype=dtype)
    n, G = X.shape
    inv_n = np.dtype(dtype).type(1.0 / n)
    mean, sq = np.zeros(G, dtype=dtype), np.zeros(G, dtype=dtype)
    for g in range(G):
        v = X[:, g]
        v = np.ascontiguousarray(v[v != 0])
        if v.size:
            a, b = v * inv_n, (v * v) * inv_n
            mean[g] = a[0] + np.add.reduce(a[1:])
            sq[g] = b[0] + np.add.reduce(b[1:])
    return mean, sq


def local_moran_arrays(X, dtype, indptr, indices, w32):
    """(z, lag, I, zero): float32 (n, G) arrays and the zero-variance mask.  var = q - m m and its root in the matrix
    dtype, the sd cast to float32 and 1 where it is 0; z = (float32(x) - float32(m)) / sd; lag row-sequential; I = z
    lag.  Flagged genes keep what these expressions give (the public function zeroes them afterwards)."""
    X = np.asarray(X, dtype=dtype)
    m, q = column_moments(X, dtype)
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(q - m * m).astype(np.float32)
    zero = sd == 0
    sd[zero] = 1.0
    z = (X.astype(np.float32) - m.astype(np.float32)) / sd
    lag = row_sequential(indptr, indices, np.asarray(w32, dtype=np.float32), z)
    return z, lag, z * lag, zero


def local_moran_counts(indptr, indices, w32, Z32, I32, perms):
    """count[i, g] = #{p : |Y[i, g] * row_sequential(Y)[i, g]| >= |I32[i, g]|},  Y = Z32[perm_p], all in float32."""
    Z32 = np.asarray(Z32, dtype=np.float32)
    w32 = np.asarray(w32, dtype=np.float32)
    absI = np.abs(np.asarray(I32, dtype=np.float32))
    count = np.zeros(Z32.shape, dtype=np.int32)
    for perm in np.asarray(perms):
        Y = Z32[perm]
        count += np.abs(Y * row_sequential(indptr, indices, w32, Y)) >= absI
    return count


def lee_local_perm_values(indptr, indices, w64, zx, zy, perms):
    """(P, n) float32: float32(zx * row_sequential(zy[perm_p])) with float64 sums -- what the reference stores."""
    zx, zy = np.asarray(zx, dtype=np.float64), np.asarray(zy, dtype=np.float64)
    w64 = np.asarray(w64, dtype=np.float64)
    perms = np.asarray(perms)
    out = np.empty((perms.shape[0], zx.size), dtype=np.float32)
    for p, perm in enumerate(perms):
        out[p] = zx * row_sequential(indptr, indices, w64, zy[perm])
    return out


def lee_local_counts(indptr, indices, w64, zx, zy, L_local, perms):
    """count[i] = #{p : |float32(zx[i] * row_sequential(zy[perm_p])[i])| >= |L_local[i]|}; the float32 store comes
    before the comparison, which is made in float64."""
    lp = lee_local_perm_values(indptr, indices, w64, zx, zy, perms)
    return (np.abs(lp).astype(np.float64) >= np.abs(np.asarray(L_local, dtype=np.float64))[None, :]).sum(axis=0).astype(np.int32)


def lee_near_ties(indptr, indices, w64, zx, zy, perms):
    """(cell, permutation) pairs of a non-empty row with ``| |lp| - |L| | <= 1e-11 |L|`` (the project's near-tie rule):
    there a z-score that differs in its last bits may decide the comparison the other way.  A cell without edges has
    lp = L = 0 under any arithmetic and is left out."""
    zx = np.asarray(zx, dtype=np.float64)
    L = zx * row_sequential(indptr, indices, np.asarray(w64, dtype=np.float64), np.asarray(zy, dtype=np.float64))
    lp = np.abs(lee_local_perm_values(indptr, indices, w64, zx, zy, perms)).astype(np.float64)
    near = np.abs(lp - np.abs(L)[None, :]) <= 1e-11 * np.abs(L)[None, :]
    return int(near[:, np.diff(np.asarray(indptr)) > 0].sum())


def count_hist(count, P):
    """hist[g, c] = cells of gene g whose count is c, (G, P + 1) int64."""
    count = np.asarray(count)
    return np.stack([np.bincount(count[:, g], minlength=P + 1) for g in range(count.shape[1])]).astype(np.int64)


def classify(z, lag, padj, alpha, zero):
    """LISA quadrants, int8: 1 HH, 2 LL, 3 HL, 4 LH; 0 where padj >= alpha (both float32; padj None: no filter), where
    the gene is flagged, or where z or lag is 0."""
    z, lag = np.asarray(z), np.asarray(lag)
    q = np.zeros(z.shape, dtype=np.int8)
    q[(z > 0) & (lag > 0)] = 1
    q[(z < 0) & (lag < 0)] = 2
    q[(z > 0) & (lag < 0)] = 3
    q[(z < 0) & (lag > 0)] = 4
    if padj is not None:
        q[np.asarray(padj, dtype=np.float32) >= np.float32(alpha)] = 0
    zero = np.asarray(zero, dtype=bool)
    if zero.ndim:
        q[..., zero] = 0
    elif zero:
        q[...] = 0
    return q


def pvalue32(count, P):
    """float32((count + 1) / (P + 1)), the quotient in float64 as the reference takes it."""
    return ((np.asarray(count) + 1) / (P + 1)).astype(np.float32)


def zscores64(x):
    """numpy's own population z-score, float64."""
    x = np.asarray(x, dtype=np.float64)
    return (x - x.mean()) / x.std()


# ---- inputs shared by the CPU pin and the device tests -----------------------------------------------------------------

def knn_csr(idx, weight):
    """(indptr int64, indices int32, data float64) of a kNN result: every row ascending by column, one weight."""
    idx = np.sort(np.asarray(idx, dtype=np.int32), axis=1)
    n, k = idx.shape
    return np.arange(0, n * k + 1, k, dtype=np.int64), idx.ravel().copy(), np.full(n * k, float(weight))


def knn_weight(k):
    """The reference's float32 1 / k, as the float64 the library takes."""
    return float(np.float32(1) / np.float32(k))


def thinned_csr(idx, seed, equal_weights=False, empty_every=0, keep=0.7):
    """A CSR graph cut out of a kNN result: every edge kept with probability ``keep`` (unequal degrees), the rows of
    every ``empty_every``-th cell emptied (a radius graph's isolated points), weights either all float32(0.3) or
    float32 draws from [0.1, 1) -- float32 values held as float64.  Rows ascending by column."""
    rng = np.random.default_rng(seed)
    idx = np.sort(np.asarray(idx, dtype=np.int32), axis=1)
    n, k = idx.shape
    mask = rng.uniform(size=(n, k)) < keep
    if empty_every:
        mask[(np.arange(n) % empty_every) == empty_every // 2] = False
    deg = mask.sum(axis=1)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = idx[mask].astype(np.int32)
    w = np.full(indices.size, np.float32(0.3)) if equal_weights else rng.uniform(0.1, 1.0, indices.size).astype(np.float32)
    return indptr, indices, w.astype(np.float64)


def count_matrix(n, G, seed, dtype=np.float32, zero_var=None, all_zero=None):
    """Poisson counts below 32 with per-gene rates between 0.05 and 4 (the code-row input); column ``zero_var`` is the
    constant 2, column ``all_zero`` is empty."""
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.uniform(0.05, 4.0, G), (n, G)).astype(dtype)
    X[X > 31] = 31
    if zero_var is not None:
        X[:, zero_var] = 2
    if all_zero is not None:
        X[:, all_zero] = 0
    return X


def lognorm_matrix(n, G, seed, dtype=np.float32, lam=(0.05, 4.0)):
    """Size-factor normalised, log1p'ed counts: no non-zero value is an integer and no two cells share a depth (the
    float-row input)."""
    rng = np.random.default_rng(seed)
    C = rng.poisson(rng.uniform(lam[0], lam[1], G), (n, G)).astype(np.float64)
    depth = C.sum(axis=1, keepdims=True) + rng.uniform(0.5, 1.5, (n, 1))
    return np.log1p(C / depth * np.median(depth)).astype(dtype)


def uniform_coords(n, seed):
    return np.random.default_rng(seed).uniform(0, np.sqrt(n) * 10.0, (n, 2))


LEE_GENES = 4
LEE_SEED = 41


def lee_input(n):
    """(coords, X float64 (n, 4)) of the local Lee tests: log-normalised counts with rates of 3 to 8, so that hardly a
    value is 0 and no two neighbourhood sums are equal -- tests/test_cpu_local_restated.py asserts that no permuted
    value comes within the near-tie distance of the observed one."""
    return uniform_coords(n, LEE_SEED + n), lognorm_matrix(n, LEE_GENES, LEE_SEED + 7 * n, dtype=np.float64, lam=(3.0, 8.0))


def lee_graph(kind, idx):
    """"knn": the row-normalised kNN graph; "csr": unequal weights, unequal degrees, every 17th row empty."""
    if kind == "knn":
        return knn_csr(idx, knn_weight(idx.shape[1]))
    return thinned_csr(idx, seed=9, empty_every=17)


LEE_K = 6
LEE_PAIR = (0, 1)
LEE_GRAPHS = ("knn", "csr")
LEE_SIZES = (255, 256, 257, 3000)
LEE_PERMS = (1, 15, 16, 17, 40)
LEE_ROW0 = (0, 7)
LEE_TABLE_ROWS = 47          # the longest case: rows [7, 47)
LEE_TABLE_SEED = 77
LEE_SEEDED = ((19, 40), (0, 17))      # (permutations of the global statistic, of the per-cell counts)
LEE_SEEDED_SEED = 78
LEE_API = dict(n=1500, P=40, k=6, seed=5, alpha=0.3, pairs=((0, 1), (2, 3), (1, 0)))
