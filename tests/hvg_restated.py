"""Plain-numpy restatements for spatialcore_amd.preprocessing (test infrastructure, no GPU).

``textbook``: the definition on the densified matrix -- every residual, clipped, then a two-pass ``np.var`` per gene; a
cell or a gene without a count contributes residuals of 0.  ``ordered``: the device's split form (dense zero term plus
sparse correction) in the device's order of operations, csrc/sc_hvg.hip line by line; with ``dtype=np.float32`` the same
form carried in float32, which is what the tolerance of the device test must tell apart from fp64.  ``select`` /
``select_batches``: the ranking rules written out gene by gene.

CASES lists (name, recipe, cells, genes, seed, theta, clip, dtype) with the edge each one hits, against the constants of
csrc/sc_hvg.hip and csrc/sc_colsort.h: 1024-cell slices of the dense term, 256-gene blocks, 512-entry column chunks."""
import functools

import numpy as np
from scipy import sparse

import pca_restated

SLICE, MAX_SLICES, BLK, COL_CHUNK = 1024, 4096, 256, 512
INF = float("inf")


# ---- the count recipes -------------------------------------------------------------------------------------------------------
def base_counts(n, G, seed):
    """pca_restated.counts: gene G // 2 is all zero when G >= 4, cell n // 3 when n >= 9."""
    return pca_restated.counts(n, G, seed)


@functools.lru_cache(maxsize=None)
def edge_counts(n, G, seed):
    """The base recipe without its empty cell, and: gene 0 stored in EVERY cell (n stored entries: ceil(n / 512) column
    chunks, at n = 1025 a last chunk of one entry); gene 1 a single count of 1, in the cell of the smallest row sum, where
    mu < 1 / n and the residual exceeds +sqrt(n); gene G // 2 all zero."""
    rng = np.random.default_rng(seed + 1000)
    A = pca_restated.counts(n, G, seed).toarray()
    A[n // 3] = rng.poisson(1.0, G)
    A[:, 0] = 1.0 + rng.poisson(2.0, n)
    A[:, 1] = 0
    A[:, G // 2] = 0
    A[int(np.argmin(A.sum(axis=1))), 1] = 1.0
    X = sparse.csr_matrix(A)
    X.sort_indices()
    assert X[:, 0].nnz == n and X[:, 1].nnz == 1 and X[:, G // 2].nnz == 0 and np.diff(X.indptr).min() >= 1
    X.data.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def real_counts(n, G, seed):
    """The base recipe times 0.37 in float32: no sum of these values is exact, so every summation order shows."""
    X = pca_restated.counts(n, G, seed).copy()
    X.data = (X.data * 0.37).astype(np.float32)
    X = sparse.csr_matrix(X, dtype=np.float32)
    X.data.setflags(write=False)
    return X


RECIPES = {"base": base_counts, "edge": edge_counts, "real": real_counts}
SEED = 11    # chosen on the CPU: every case's smallest relative gap between positive textbook variances is >= 1e-8

CASES = (
    ("5x3", "base", 5, 3, SEED, 100.0, None, np.float64),                  # fewer cells than anything is cut into, no zero gene or cell
    ("300x9", "base", 300, 9, SEED, 100.0, None, np.float64),              # one slice, one gene block, one chunk per gene; zero gene and cell
    ("300x9-clip3", "base", 300, 9, SEED, 100.0, 3.0, np.float64),         # -clip engages (mu >~ 10) next to +clip
    ("777x37", "base", 777, 37, SEED, 100.0, None, np.float64),            # genes of two chunks (more than 512 stored entries)
    ("777x37-clip3", "base", 777, 37, SEED, 100.0, 3.0, np.float64),
    ("777x37-f32-real", "real", 777, 37, SEED, 100.0, None, np.float32),   # float32 input, widened exactly; inexact sums everywhere
    ("2000x200", "base", 2000, 200, SEED, 100.0, None, np.float64),        # two slices, the second of 976 cells
    ("2000x200-clip3", "base", 2000, 200, SEED, 100.0, 3.0, np.float64),
    ("1023x255", "edge", 1023, 255, SEED, 100.0, None, np.float64),        # one slice - 1 cell, one gene block - 1; gene 0: chunks of 512 + 511
    ("1024x256", "edge", 1024, 256, SEED, 100.0, None, np.float64),        # exactly one slice, one gene block, gene 0 two full chunks
    ("1025x257", "edge", 1025, 257, SEED, 100.0, None, np.float64),        # a second slice of one cell, a second block of one gene, gene 0: 512 + 512 + 1
    ("1025x257-poisson", "edge", 1025, 257, SEED, INF, None, np.float64),  # theta = inf
    ("2049x40", "base", 2049, 40, SEED, 100.0, None, np.float64),          # three slices, the last of one cell
)
IDS = [c[0] for c in CASES]
MEASURED = ("300x9", "300x9-clip3", "777x37", "777x37-clip3", "2000x200", "2000x200-clip3")   # the cases the tolerance was placed on


def matrix(case):
    _, recipe, n, G, seed, _, _, dtype = case
    X = RECIPES[recipe](n, G, seed)
    assert X.shape == (n, G) and X.dtype == dtype
    return X


# ---- the definition --------------------------------------------------------------------------------------------------------
def raw_residuals(X, theta=100.0):
    """The unclipped residuals of the dense matrix, (x - mu) / sqrt(mu + mu^2 / theta) with mu = s_i t_g / T; 0 where mu == 0."""
    A = np.asarray(X.toarray() if sparse.issparse(X) else X, dtype=np.float64)
    s, t = A.sum(axis=1, keepdims=True), A.sum(axis=0, keepdims=True)
    mu = s * t / t.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (A - mu) / np.sqrt(mu + mu ** 2 / theta)
    return np.where(mu > 0, z, 0.0), mu


def textbook(X, theta=100.0, clip=None):
    """residual_variances by the definition: clip to [-clip, clip] (default sqrt(cells)), np.var (two passes, ddof 0)."""
    z, _ = raw_residuals(X, theta)
    c = np.sqrt(z.shape[0]) if clip is None else clip
    return np.var(np.clip(z, -c, c), axis=0)


def moments(X):
    """(sum x, sum x^2) per gene in exact integer arithmetic (integer counts only), (means, sample variances)."""
    A = np.asarray(X.toarray())
    I = A.astype(np.int64)
    assert np.array_equal(I, A)
    n = A.shape[0]
    s1, s2 = I.sum(axis=0), (I * I).sum(axis=0)
    assert s2.max() < 2**53
    means = s1.astype(np.float64) / n
    return s1.astype(np.float64), s2.astype(np.float64), means, (s2.astype(np.float64) / n - means ** 2) * (n / (n - 1))


# ---- the device's order --------------------------------------------------------------------------------------------------------
def slice_rows(n):
    return SLICE * -(-n // (SLICE * MAX_SLICES))


def _running(M):
    """0.0 + M[:, 0] + M[:, 1] + ... one column at a time."""
    acc = np.zeros(M.shape[0], dtype=M.dtype)
    for k in range(M.shape[1]):
        acc = acc + M[:, k]
    return acc


def _chunk_table(colptr):
    """(gene of every chunk, its first entry, its length) of the column-sorted copy, and the first chunk of every gene."""
    lens = np.diff(colptr)
    per = -(-lens // COL_CHUNK)
    cptr = np.concatenate([[0], np.cumsum(per)])
    cgene = np.repeat(np.arange(lens.size), per)
    k = np.arange(cptr[-1]) - cptr[cgene]
    p0 = colptr[cgene] + k * COL_CHUNK
    return cgene, p0, np.minimum(p0 + COL_CHUNK, colptr[cgene + 1]) - p0, cptr


def _chunk_sums(values, p0, length, cgene, cptr, G):
    """Per gene: 0.0 + its chunk sums in chunk order, a chunk sum = 0.0 + its entries in stored (row) order.  A short chunk is
    padded with +0.0, which changes no sum."""
    pad = np.zeros((p0.size, COL_CHUNK), dtype=values.dtype)
    for c in range(p0.size):
        pad[c, :length[c]] = values[p0[c]:p0[c] + length[c]]
    part = _running(pad)
    out = np.zeros(G, dtype=values.dtype)
    per = np.diff(cptr)
    for j in range(int(per.max()) if per.size else 0):
        genes = np.flatnonzero(per > j)
        out[genes] = out[genes] + part[cptr[genes] + j]
    return out


def ordered(X, theta=100.0, clip=None, dtype=np.float64):
    """sc_hvg_pearson restated in its own order (the header of csrc/sc_hvg.hip): {"sum", "sumsq", "mean", "var"}."""
    dt = np.dtype(dtype).type
    X = sparse.csr_matrix(X)
    assert X.has_sorted_indices
    n, G = X.shape
    clip = dt(np.sqrt(n) if clip is None else clip)
    inv_theta = dt(1.0 / theta)
    data = X.data.astype(dt)
    # s_i = 0.0 + the row's stored values in index order
    s = np.zeros(n, dtype=dt)
    lens = np.diff(X.indptr)
    for j in range(int(lens.max())):
        rows = np.flatnonzero(lens > j)
        s[rows] = s[rows] + data[X.indptr[rows] + j]
    # the column-sorted copy: a stable sort by column keeps the rows ascending
    order = np.argsort(X.indices, kind="stable")
    crow = np.repeat(np.arange(n), lens)[order]
    cval = data[order]
    colptr = np.concatenate([[0], np.cumsum(np.bincount(X.indices, minlength=G))])
    cgene, p0, length, cptr = _chunk_table(colptr)
    t = _chunk_sums(cval, p0, length, cgene, cptr, G)
    q = _chunk_sums(cval * cval, p0, length, cgene, cptr, G)
    # T = 0.0 + a[0] + ... + a[255], a[j] = 0.0 + t_j + t_(j + 256) + ...
    tp = np.zeros(-(-G // BLK) * BLK, dtype=dt)
    tp[:G] = t
    T = dt(0.0)
    for a in _running(tp.reshape(-1, BLK).T):
        T = T + a
    p = t / T

    def z_of(x, mu):
        v = mu * (dt(1.0) + mu * inv_theta)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (x - mu) / np.sqrt(v)

    lo = dt(0.0) - clip
    # the dense zero term: per slice 0.0 + r0 in cell order, the slices in slice order
    mu = s[:, None] * p[None, :]
    z0 = z_of(dt(0.0), mu)
    r0 = np.where(mu > 0, np.where(z0 > lo, z0, lo), dt(0.0))
    R = slice_rows(n)
    d1, d2 = np.zeros(G, dtype=dt), np.zeros(G, dtype=dt)
    for i0 in range(0, n, R):
        a1, a2 = np.zeros(G, dtype=dt), np.zeros(G, dtype=dt)
        for i in range(i0, min(i0 + R, n)):
            a1 = a1 + r0[i]
            a2 = a2 + r0[i] * r0[i]
        d1, d2 = d1 + a1, d2 + a2
    # the sparse correction over the column-sorted copy
    egene = np.repeat(np.arange(G), np.diff(colptr))
    mu_e = s[crow] * p[egene]
    z0e, ze = z_of(dt(0.0), mu_e), z_of(cval, mu_e)
    r0e = np.where(mu_e > 0, np.where(z0e > lo, z0e, lo), dt(0.0))
    re = np.where(ze > lo, ze, lo)
    re = np.where(mu_e > 0, np.where(re < clip, re, clip), dt(0.0))
    c1 = _chunk_sums(re - r0e, p0, length, cgene, cptr, G)
    c2 = _chunk_sums(re * re - r0e * r0e, p0, length, cgene, cptr, G)
    dn = dt(n)
    mean = (d1 + c1) / dn
    var = (d2 + c2) / dn - mean * mean
    return {"sum": t, "sumsq": q, "mean": mean, "var": np.where(var > 0, var, dt(0.0))}


# ---- comparisons and the ranking rules -----------------------------------------------------------------------------------------
def rel_err(got, ref):
    """Per gene |got - ref| / ref, 0 where both are 0; the largest."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.all(got[ref == 0] == 0)
    pos = ref > 0
    return float(np.max(np.abs(got[pos] - ref[pos]) / ref[pos])) if pos.any() else 0.0


def smallest_gap(var):
    """The smallest relative gap between consecutive positive variances in sorted order."""
    v = np.sort(np.asarray(var, dtype=np.float64))
    v = v[v > 0]
    return float(np.min(np.diff(v) / v[1:])) if v.size > 1 else np.inf


def ranks(var):
    """rank[g] written out: the number of genes that come before g (larger variance, or equal variance and smaller index)."""
    var = np.asarray(var, dtype=np.float64)
    return np.array([sum(1 for h in range(var.size) if var[h] > var[g] or (var[h] == var[g] and h < g)) for g in range(var.size)])


def select(var, n_top):
    """(highly_variable, highly_variable_rank) of one matrix."""
    r = ranks(var)
    hv = r < n_top
    return hv, np.where(hv, r.astype(np.float64), np.nan)


def select_batches(V, n_top):
    """The batch rule gene by gene: {"nbatches", "intersection", "rank", "highly_variable", "residual_variances"}."""
    V = np.asarray(V, dtype=np.float64)
    B, G = V.shape
    rk = np.stack([ranks(V[b]) for b in range(B)])
    nb = np.array([sum(1 for b in range(B) if rk[b, g] < n_top) for g in range(G)])
    med = np.array([np.median([rk[b, g] for b in range(B) if rk[b, g] < n_top]) if nb[g] else np.nan for g in range(G)])
    order = sorted(range(G), key=lambda g: (np.isnan(med[g]), med[g] if nb[g] else 0.0, -nb[g], g))
    hv = np.zeros(G, dtype=bool)
    hv[order[:n_top]] = True
    return {"nbatches": nb, "intersection": nb == B, "rank": np.where(hv, med, np.nan), "highly_variable": hv,
            "residual_variances": V.mean(axis=0)}
