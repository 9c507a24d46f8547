"""Plain-numpy restatements for spatialcore_amd.pca (test infrastructure, no GPU).

``counts``: the seeded input recipe.  ``dense_pca``: the definition on the densified matrix (covariance, eigh, flip,
clip, sign rule).  ``ordered_project``: the projection in the device's summation order (a row's stored entries in index
order from 0.0, multiply and add rounded separately, then minus the offset).  ``log1p_norm``: the normalisation with the
row sum in index order.  ``sklearn_eigh`` / ``sklearn_full``: the reference itself.

SHAPES lists (N, G, n_comps) with the edge each one hits, against the constants of csrc/sc_pca.hip:
128-column Gram blocks, 32-row chunks, 16384-row slices, 4 rows per MFMA k-step, 256 / lanes rows per projection
workgroup (lanes = n_comps rounded up to a power of two, at least 2)."""
import functools

import numpy as np
from scipy import sparse

BLK, CHUNK, SLICE_ROWS, TPB = 128, 32, 16384, 256

SHAPES = (
    (5, 3, 2),            # fewer rows than one MFMA k-step pair; G below one 16-tile
    (300, 9, 1),          # one component
    (777, 37, 5),         # G not a multiple of 16
    (1031, 70, 64),       # a full wavefront of components; a partly filled last projection workgroup (4 rows each)
    (1029, 70, 64),       # ... and N one past a multiple of those 4 rows
    (2500, 130, 50),      # G two past one 128-column block: diagonal and off-diagonal blocks, a nearly empty panel
    (4100, 272, 33),      # three column blocks, all six upper blocks; N = 4 past a multiple of the 32-row chunk
    (4 * SLICE_ROWS + 1, 40, 3),   # five row slices, the last of one row; 2049 row chunks
)
LANE_SHAPE = (259, 200)   # one row stores every gene but the zero gene (199 > 3 x 64), one row a single entry
LANE_COMPS = (3, 20, 64)  # lane groups of 4, 32 and 64: the full row takes 50, 7 and 4 fetches


def lanes(K):
    tp = 2
    while tp < K:
        tp *= 2
    return tp


@functools.lru_cache(maxsize=None)
def counts(n, G, seed):
    """Poisson(0.3 + L F / r): L ~ Gamma(2, 1) is n x r, F ~ Gamma(1, 1) is r x G with row j scaled by 8 0.62^j,
    r = min(6, G).  Gene G // 2 is all zero when G >= 4, cell n // 3 when n >= 9.  float64 CSR, canonical."""
    rng = np.random.default_rng(seed)
    r = min(6, G)
    L = rng.gamma(2.0, 1.0, size=(n, r))
    F = rng.gamma(1.0, 1.0, size=(r, G)) * (8.0 * 0.62 ** np.arange(r))[:, None]
    A = rng.poisson(0.3 + L @ F / r).astype(np.float64)
    if G >= 4:
        A[:, G // 2] = 0
    if n >= 9:
        A[n // 3] = 0
    X = sparse.csr_matrix(A)
    X.sort_indices()
    X.data.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def lane_counts(seed=31):
    """The recipe at LANE_SHAPE with row 7 storing every gene but the zero gene and row 11 a single entry."""
    n, G = LANE_SHAPE
    A = counts(n, G, seed).toarray()
    A[7] = 1.0 + np.random.default_rng(seed + 1).poisson(1.5, G)
    A[7, G // 2] = 0
    A[11] = 0
    A[11, 5] = 3
    X = sparse.csr_matrix(A)
    X.sort_indices()
    assert X[7].nnz == G - 1 and X[11].nnz == 1 and X[:, G // 2].nnz == 0 and X[n // 3].nnz == 0
    X.data.setflags(write=False)
    return X


SEED = 11      # of every SHAPES case (chosen on the CPU, with sklearn alone, so that no gap of a kept component is near the filter)


# ---- normalisation -----------------------------------------------------------------------------------------------------------
def _row_walk(X):
    """Yields (j, rows with more than j stored entries, the position of their j-th entry)."""
    lens = np.diff(X.indptr)
    for j in range(int(lens.max()) if lens.size else 0):
        rows = np.flatnonzero(lens > j)
        yield j, rows, X.indptr[rows] + j


def log1p_norm(X, target_sum=1e4):
    """log1p(x / rowsum * target_sum) as float64 CSR; the row sum over the stored entries in index order from 0.0; a row
    whose sum is 0 stays 0."""
    X = sparse.csr_matrix(X, dtype=np.float64)
    X.sort_indices()
    s = np.zeros(X.shape[0])
    for _, rows, pos in _row_walk(X):
        s[rows] = s[rows] + X.data[pos]
    per = np.repeat(s, np.diff(X.indptr))
    with np.errstate(divide="ignore", invalid="ignore"):
        data = np.where(per > 0, np.log1p((X.data / per) * target_sum), 0.0)
    return sparse.csr_matrix((data, X.indices.copy(), X.indptr.copy()), shape=X.shape)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def sample_scale(A):
    """The sample standard deviation (ddof = 1) per column, 1 for a column of zero variance."""
    sd = np.std(np.asarray(A, dtype=np.float64), axis=0, ddof=1)
    return np.where(sd == 0, 1.0, sd)


def dense_pca(A, n_comps, scale=False, gram_dtype=np.float64):
    """PCA by the covariance matrix in plain numpy on the dense matrix ``A``: C = (A^T A - N mu mu^T) / (N - 1), optional
    D^-1 C D^-1, eigh, descending, negatives clipped, each component's largest-magnitude entry positive.
    ``gram_dtype=float32`` accumulates A^T A in float32 (what the tolerance must tell apart from fp64)."""
    A = np.asarray(A, dtype=np.float64)
    n, G = A.shape
    gram = (A.astype(gram_dtype).T @ A.astype(gram_dtype)).astype(np.float64)
    mean = A.sum(axis=0) / n
    C = (gram - n * np.outer(mean, mean)) / (n - 1)
    sigma = np.ones(G)
    if scale:
        var = np.clip(np.diag(C), 0, None)
        zero = var <= n * np.finfo(float).eps * var + (n * mean * np.finfo(float).eps) ** 2
        sigma = np.where(zero, 1.0, np.sqrt(var))
        C = C / np.outer(sigma, sigma)
        C[zero, :] = 0
        C[:, zero] = 0
    lam, vec = np.linalg.eigh(C)
    lam, Vt = np.clip(lam[::-1], 0, None), vec[:, ::-1].T
    top = np.argmax(np.abs(Vt), axis=1)
    sg = np.sign(Vt[np.arange(G), top])
    sg[sg == 0] = 1
    Vt = Vt * sg[:, None]
    scores = ((A - mean) / sigma) @ Vt[:n_comps].T
    return {"mean": mean, "scale": sigma, "variance": lam[:n_comps], "variance_ratio": lam[:n_comps] / lam.sum(),
            "components": Vt[:n_comps], "scores": scores, "spectrum": lam, "covariance": C}


def offsets(Vs, mean):
    """offset[c] = sum_g Vs[c][g] mean[g], genes in index order from 0.0, multiply and add rounded separately."""
    off = np.zeros(Vs.shape[0])
    for g in range(Vs.shape[1]):
        off = off + Vs[:, g] * mean[g]
    return off


def ordered_project(X, Vs, offset):
    """scores[i][c] = (0.0 + val[p] Vs[c][idx[p]] over row i's stored entries in index order) - offset[c], float64."""
    X = sparse.csr_matrix(X, dtype=np.float64)
    assert X.has_sorted_indices
    T = np.ascontiguousarray(np.asarray(Vs, dtype=np.float64).T)      # [gene][component]
    acc = np.zeros((X.shape[0], T.shape[1]))
    for _, rows, pos in _row_walk(X):
        acc[rows] = acc[rows] + X.data[pos][:, None] * T[X.indices[pos]]
    return acc - np.asarray(offset, dtype=np.float64)[None, :]


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _sklearn(X, n_comps, solver):
    from sklearn.decomposition import PCA

    m = PCA(n_components=min(X.shape), svd_solver=solver)
    scores = m.fit_transform(X)
    return {"variance": m.explained_variance_[:n_comps], "variance_ratio": m.explained_variance_ratio_[:n_comps],
            "components": m.components_[:n_comps], "scores": np.asarray(scores)[:, :n_comps], "mean": np.asarray(m.mean_).ravel(),
            "spectrum": m.explained_variance_}


def sklearn_eigh(X, n_comps):
    """sklearn's PCA(svd_solver="covariance_eigh") on ``X`` (CSR or dense), every component computed, ``n_comps`` kept;
    ``spectrum`` holds all eigenvalues for the gap filter."""
    return _sklearn(X, n_comps, "covariance_eigh")


def sklearn_full(A, n_comps):
    return _sklearn(np.asarray(A, dtype=np.float64), n_comps, "full")


def separated(spectrum, n_comps, rel=1e-5):
    """Mask over the first ``n_comps`` components: the gap to both neighbouring eigenvalues is >= rel * lambda_1."""
    lam = np.asarray(spectrum, dtype=np.float64)
    gap = np.full(lam.size, np.inf)
    d = lam[:-1] - lam[1:]
    gap[:-1] = np.minimum(gap[:-1], d)
    gap[1:] = np.minimum(gap[1:], d)
    return gap[:n_comps] >= rel * lam[0]


def rel(a, b):
    """max |a - b| relative to the largest absolute entry of the reference ``b``."""
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / np.max(np.abs(b)))


def differences(got, ref, mask):
    """The four figures test 4 bounds: variance and ratio over all components, loadings and scores over ``mask``."""
    return (rel(got["variance"], ref["variance"]), rel(got["variance_ratio"], ref["variance_ratio"]),
            rel(got["components"][mask], ref["components"][mask]), rel(got["scores"][:, mask], ref["scores"][:, mask]))


MODES = ("counts", "normalize", "normalize_scale")


@functools.lru_cache(maxsize=None)
def reference_case(n, G, K, mode, lane=False):
    """(the CSR handed to pca, the dense matrix sklearn sees, sklearn covariance_eigh's result, the gap mask)."""
    C = lane_counts() if lane else counts(n, G, SEED)
    X = C if mode == "counts" else log1p_norm(C)
    if mode == "normalize_scale":
        A = X.toarray()
        ref = sklearn_eigh(A / sample_scale(A), K)
    else:
        ref = sklearn_eigh(X, K)
    mask = separated(ref["spectrum"], K)
    return C, X, ref, mask
