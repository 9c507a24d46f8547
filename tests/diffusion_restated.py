"""numpy restatement of spatialcore_amd.diffusion in the device's own orders (sc_diffusion.hip): every
function here gives the bits the kernels must give, except where ``exp`` enters (the kernel weights of the search path).

Orders restated: a squared distance adds its d terms in column order from the c = 0 term; a neighbour list is the k
smallest (d2, index); a row sum runs over the stored entries in column order from 0; a dot product over the cells is cut
into chunks of CHUNK = 1024, inside a chunk element e = r * 64 + lane, every lane adds its 16 products for r ascending
from the first, the 64 lane sums meet in the adjacent-pair tree, a short chunk is padded with zero products, and the chunk
sums are added in chunk order from 0; the Gram-Schmidt update subtracts one vector at a time, ascending."""
import numpy as np
from scipy import sparse
from scipy.linalg import eigh_tridiagonal

CHUNK = 1024            # SUM_CHUNK (sc_chunk_sum.h): cells per partial of a dot product
LANES = 64
QUERY_BLOCK = 256       # DF_QB: queries per workgroup of the register form (padded d <= 32)
TILE = 128              # DF_TILE: candidates per LDS tile of the register form
QUERY_BLOCK_WIDE = 64   # DF_QB_L / DF_TILE_L: the same for 32 < padded d <= 64
TILE_WIDE = 32
SPLIT_BELOW = 100000    # DF_SPLIT_BELOW: fewer queries split the candidates over workgroups
CHECK_EVERY = 16


def traj(n, d, seed):
    """A branching trajectory: t ~ U(0, 1), a branch flag with probability 0.4, columns cos 3t, sin 3t and
    3 max(t - 0.5, 0) branch, truncated or zero-padded to d columns, plus 0.05 standard-normal noise.  Returns (X, t)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 1.0, n)
    branch = rng.uniform(0.0, 1.0, n) < 0.4
    base = np.stack([np.cos(3 * t), np.sin(3 * t), 3 * np.maximum(t - 0.5, 0.0) * branch], axis=1)
    X = np.zeros((n, d))
    X[:, :min(d, 3)] = base[:, :min(d, 3)]
    return X + 0.05 * rng.standard_normal((n, d)), t


# ---- steps 1 - 3 ----------------------------------------------------------------------------------------------------
def pair_d2(X, rows, cols):
    """d2 of the pairs (rows[p], cols[p]): the terms in column order, products and sums rounded separately."""
    X = np.asarray(X, dtype=np.float64)
    f = X[rows, 0] - X[cols, 0]
    acc = f * f
    for c in range(1, X.shape[1]):
        f = X[rows, c] - X[cols, c]
        acc = acc + f * f
    return acc


def knn(X, k, block=512):
    """(indices int32, d2) of the k smallest (d2, j), j != i, for every row i."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    idx = np.empty((n, k), dtype=np.int32)
    d2 = np.empty((n, k), dtype=np.float64)
    for b in range(0, n, block):
        q = X[b:b + block]
        f = q[:, None, 0] - X[None, :, 0]
        acc = f * f
        for c in range(1, X.shape[1]):
            f = q[:, None, c] - X[None, :, c]
            acc = acc + f * f
        acc[np.arange(q.shape[0]), np.arange(b, b + q.shape[0])] = np.inf
        order = np.argsort(acc, axis=1, kind="stable")[:, :k]    # stable: equal distances keep index order
        idx[b:b + block] = order
        d2[b:b + block] = np.take_along_axis(acc, order, axis=1)
    return idx, d2


def scales(d2):
    """Median of every row's k squared distances (ascending): the middle one or (a + b) / 2."""
    k = d2.shape[1]
    return d2[:, k // 2].copy() if k % 2 else (d2[:, k // 2 - 1] + d2[:, k // 2]) / 2.0


def union_edges(idx):
    """CSR pattern (indptr int64, indices int32, rows sorted by column) of {(i, j): j in N(i) or i in N(j)}."""
    n, k = idx.shape
    A = sparse.csr_matrix((np.ones(n * k), (np.repeat(np.arange(n), k), idx.ravel())), shape=(n, n))
    S = sparse.csr_matrix(((A + A.T) > 0).astype(np.float64))
    S.sort_indices()
    return S.indptr.astype(np.int64), S.indices.astype(np.int32)


def kernel_weights(X, indptr, indices, s2):
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    acc = pair_d2(X, rows, indices)
    si, sj = s2[rows], s2[indices]
    den = si + sj
    return np.sqrt(((2.0 * np.sqrt(si)) * np.sqrt(sj)) / den) * np.exp(-acc / den)


# ---- step 4 -----------------------------------------------------------------------------------------------------------
def row_sums(indptr, values):
    """Running sum from 0 over every row's stored entries, in order."""
    deg = np.diff(indptr)
    s = np.zeros(deg.size)
    for p in range(int(deg.max())):
        rows = np.flatnonzero(deg > p)
        s[rows] = s[rows] + values[indptr[rows] + p]
    return s


def transition(indptr, indices, w):
    """(T values, q, D): q_i = sum_j w_ij, K' = w / (q_i q_j), D_i = sum_j K'_ij, T = K' / (sqrt(D_i) sqrt(D_j))."""
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    q = row_sums(indptr, w)
    Kp = w / (q[rows] * q[indices])
    D = row_sums(indptr, Kp)
    return Kp / (np.sqrt(D[rows]) * np.sqrt(D[indices])), q, D


def n_components(indptr, indices):
    n = indptr.size - 1
    return sparse.csgraph.connected_components(sparse.csr_matrix((np.ones(indices.size), indices, indptr), shape=(n, n)),
                                               directed=False)[0]


# ---- step 5 -----------------------------------------------------------------------------------------------------------
def dots(V, w):
    """V_l . w for every row l of V (L, n), in the device's order."""
    V = np.atleast_2d(V)
    L, n = V.shape
    chunks = -(-n // CHUNK)
    P = np.zeros((L, chunks * CHUNK))
    P[:, :n] = V * w
    P = P.reshape(L, chunks, CHUNK // LANES, LANES)
    s = P[:, :, 0, :].copy()
    for r in range(1, CHUNK // LANES):
        s = s + P[:, :, r, :]
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    out = np.zeros(L)
    for ch in range(chunks):
        out = out + s[:, ch, 0]
    return out


def spmv(indptr, indices, T, x):
    return row_sums(indptr, T * x[indices])


def lanczos(indptr, indices, T, start, steps, V=None, alpha=None, beta=None):
    """``steps`` more steps; returns (V, alpha, beta) with beta[0] = ||start|| and beta[j + 1] the norm after step j."""
    n = indptr.size - 1
    if V is None:
        b0 = np.sqrt(dots(start, start)[0])
        V, alpha, beta = [start / b0], [], [b0]
    for _ in range(steps):
        j = len(alpha)
        w = spmv(indptr, indices, T, V[j])
        basis = np.asarray(V[:j + 1])
        c1 = dots(basis, w)
        for l in range(j + 1):
            w = w - basis[l] * c1[l]
        c2 = dots(basis, w)
        for l in range(j + 1):
            w = w - basis[l] * c2[l]
        alpha.append(c1[j] + c2[j])
        b = np.sqrt(dots(w, w)[0])
        beta.append(b)
        V.append(w / b)
    assert len(V) <= n + 1
    return V, alpha, beta


def ritz(indptr, indices, T, V, S, lam):
    """Unit Ritz vectors (n, c) of the coefficient columns S (m, c) and their true residuals."""
    m, c = S.shape
    vecs = np.empty((V[0].size, c))
    res = np.empty(c)
    for l in range(c):
        y = V[0] * S[0, l]
        for j in range(1, m):
            y = y + V[j] * S[j, l]
        y = y / np.sqrt(dots(y, y)[0])
        r = spmv(indptr, indices, T, y) - lam[l] * y
        vecs[:, l] = y
        res[l] = np.sqrt(dots(r, r)[0])
    return vecs, res


def sign(vecs):
    vecs = vecs.copy()
    lead = np.argmax(np.abs(vecs), axis=0)
    flip = vecs[lead, np.arange(vecs.shape[1])] < 0
    vecs[:, flip] = -vecs[:, flip]
    return vecs


def eigenpairs(indptr, indices, T, n_comps, tol=1e-10, max_basis=None, random_state=0):
    """The driver of diffusion_map: (values descending, signed vectors, residuals, steps)."""
    n = indptr.size - 1
    max_basis = min(n, 1024) if max_basis is None else min(max_basis, n)
    start = np.random.RandomState(random_state).standard_normal(n)
    V = alpha = beta = None
    m = 0
    while m < max_basis:
        V, alpha, beta = lanczos(indptr, indices, T, start, min(CHECK_EVERY, max_basis - m), V, alpha, beta)
        m = len(alpha)
        if m < n_comps:
            continue
        theta, S = eigh_tridiagonal(np.asarray(alpha), np.asarray(beta[1:m]))
        top = np.arange(m - 1, m - 1 - n_comps, -1)
        if np.abs(beta[m] * S[m - 1, top]).max() <= tol / 4 or m == max_basis:
            vecs, res = ritz(indptr, indices, T, V, S[:, top], theta[top])
            if res.max() <= tol:
                return theta[top].copy(), sign(vecs), res, m
    raise RuntimeError("not converged")


def graph(X, k):
    """Steps 1 - 4 from the features: a dict of every intermediate."""
    idx, d2 = knn(X, k)
    s2 = scales(d2)
    indptr, indices = union_edges(idx)
    w = kernel_weights(X, indptr, indices, s2)
    T, q, D = transition(indptr, indices, w)
    return {"idx": idx, "d2": d2, "s2": s2, "indptr": indptr, "indices": indices, "w": w, "T": T, "q": q, "D": D}


def dense(indptr, indices, values):
    n = indptr.size - 1
    return sparse.csr_matrix((values, indices, indptr), shape=(n, n)).toarray()


# ---- step 7 -----------------------------------------------------------------------------------------------------------
def pseudotime(psi, lam, root, n_dcs):
    acc = np.zeros(psi.shape[0])
    for l in range(1, n_dcs):
        term = (lam[l] / (1.0 - lam[l])) * (psi[:, l] - psi[root, l])
        acc = acc + term * term
    dpt = np.sqrt(acc)
    return dpt / dpt.max()
