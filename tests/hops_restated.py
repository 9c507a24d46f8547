"""numpy / scipy restatement of the neighbourhood shells and their aggregates (sc_hop_*, spatial.aggregate_neighbors;
DESIGN.md 4.6x), the published algorithm of CellCharter's ``aggregate_neighbors`` (Varrone et al. 2024):

  (a) shells_textbook: the shells by the textbook recursion, hop <- hop @ A, drop what was visited, visited += hop;
  (b) shells_bfs:      the shells by a plain breadth-first search per cell;
  (c) ordered:         mean and variance in the device's order: the entries of a row added one by one in ascending
                       index from 0.0, one division; variance = (sum x x) / c - m m, every operation rounded on its own;
  (d) textbook:        the textbook's normalize(adj) @ X and normalize(adj) @ (X X) - mean^2;
  (e) ari:             the adjusted Rand index;
and the graphs the tests run on.  A shell is a canonical scipy CSR pattern (int64 indptr after .astype, int32 indices)."""
import functools

import numpy as np
from scipy import sparse
from scipy.spatial import cKDTree

U = 2.0 ** -53


# ---- graphs ------------------------------------------------------------------------------------------------------------------
def pattern(rows, cols, n) -> sparse.csr_matrix:
    """Canonical CSR pattern (data 1.0) of the stored entries (rows[k], cols[k]), diagonal dropped."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    keep = rows != cols
    A = sparse.csr_matrix((np.ones(int(keep.sum())), (rows[keep], cols[keep])), shape=(n, n))
    A.sum_duplicates()
    A.sort_indices()
    A.data[:] = 1.0
    return A


def knn_union(xy, k) -> sparse.csr_matrix:
    """The symmetric union of the exact k nearest-neighbour lists (uniform points: no ties)."""
    n = xy.shape[0]
    _, idx = cKDTree(xy).query(xy, k=k + 1)
    src, dst = np.repeat(np.arange(n), k), idx[:, 1:].ravel()
    return pattern(np.concatenate([src, dst]), np.concatenate([dst, src]), n)


def uniform_points(n, seed):
    return np.random.default_rng(seed).uniform(size=(n, 2))


def directed(n, out_degree, seed) -> sparse.csr_matrix:
    """Every cell points at out_degree random other cells; no entry is mirrored on purpose."""
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(n), out_degree)
    dst = (src + rng.integers(1, n, size=src.size)) % n
    return pattern(src, dst, n)


def star(h, pendant=False) -> sparse.csr_matrix:
    """Undirected star: hub 0, leaves 1 .. h; pendant: one more cell h + 1 joined to leaf 1 alone.  At the hop from shell 1
    to shell 2 the bound 1 + |S_1| + sum of the degrees of S_1's members is 2 h + 1 (+ 1 with the pendant) for the hub
    and h + 2 for a leaf other than leaf 1."""
    src, dst = np.zeros(h, dtype=np.int64), np.arange(1, h + 1)
    if pendant:
        src, dst = np.append(src, 1), np.append(dst, h + 1)
    return pattern(np.concatenate([src, dst]), np.concatenate([dst, src]), h + 1 + int(pendant))


def directed_star(h) -> sparse.csr_matrix:
    """Hub 0 points at the leaves 1 .. h, leaf 1 points back at the hub, the other leaves at nothing.  At the hop from
    shell 1 to shell 2 the hub's bound is 1 + h + 1 and leaf 1's is 1 + 1 + h: both h + 2, and leaf 1's table really takes
    h + 2 keys (itself, the hub, every leaf)."""
    return pattern(np.append(np.zeros(h, dtype=np.int64), 1), np.append(np.arange(1, h + 1), 0), h + 1)


def hub_graph(n=5000, k=6, seed=5) -> sparse.csr_matrix:
    """The union k-NN graph of uniform points plus cell 0 joined to every second cell."""
    A = knn_union(uniform_points(n, seed), k).tocoo()
    other = np.arange(2, n, 2)
    return pattern(np.concatenate([A.row, np.zeros(other.size, dtype=np.int64), other]),
                   np.concatenate([A.col, other, np.zeros(other.size, dtype=np.int64)]), n)


def path(n) -> sparse.csr_matrix:
    a = np.arange(n - 1)
    return pattern(np.concatenate([a, a + 1]), np.concatenate([a + 1, a]), n)


def with_isolated_cell(A, cell) -> sparse.csr_matrix:
    coo = A.tocoo()
    keep = (coo.row != cell) & (coo.col != cell)
    return pattern(coo.row[keep], coo.col[keep], A.shape[0])


def two_components(n_a, n_b, k, seed) -> sparse.csr_matrix:
    return sparse.block_diag([knn_union(uniform_points(n_a, seed), k), knn_union(uniform_points(n_b, seed + 1), k)], format="csr")


# ---- (a), (b) the shells -----------------------------------------------------------------------------------------------------
def _canonical(S) -> sparse.csr_matrix:
    S = sparse.csr_matrix(S)
    S.eliminate_zeros()
    S.sum_duplicates()
    S.sort_indices()
    S.data[:] = 1.0
    return S


def shells_textbook(A, L):
    """[S_1 .. S_L]: S_1 = A; S_{l+1} = pattern(S_l @ A) minus everything visited (the diagonal and S_1 .. S_l)."""
    n = A.shape[0]
    hop = _canonical(A)
    visited = (hop + sparse.identity(n, format="csr")).tocsr()
    out = [hop]
    for _ in range(1, L):
        nxt = _canonical(hop @ A)
        nxt = _canonical(nxt - nxt.multiply(visited))
        visited = (visited + nxt).tocsr()
        hop = nxt
        out.append(hop)
    return out


def shells_bfs(A, L):
    """The same shells by a breadth-first search from every cell: (indptr, indices) per shell."""
    n = A.shape[0]
    ptr, idx = A.indptr, A.indices
    rows = [[None] * n for _ in range(L)]
    seen_from = np.full(n, -1, dtype=np.int64)     # the last search that reached the cell
    nothing = np.zeros(0, dtype=np.int32)
    for i in range(n):
        seen_from[i] = i
        frontier = np.array([i], dtype=np.int32)
        for l in range(L):
            reached = np.unique(np.concatenate([idx[ptr[j]:ptr[j + 1]] for j in frontier])) if frontier.size else nothing
            frontier = reached[seen_from[reached] != i].astype(np.int32)
            seen_from[frontier] = i
            rows[l][i] = frontier
    out = []
    for l in range(L):
        indptr = np.zeros(n + 1, dtype=np.int64)
        indptr[1:] = np.cumsum([r.size for r in rows[l]])
        out.append((indptr, np.concatenate(rows[l]).astype(np.int32)))
    return out


def as_arrays(S):
    """(int64 indptr, int32 indices) of a canonical CSR: what sc_hop_get returns."""
    return S.indptr.astype(np.int64), S.indices.astype(np.int32)


def key_bounds(A, shells):
    """Per cell, the bound that classes its row at the hop from shells[-1] to the next shell:
    1 + sum_s |S_s(i)| + sum_{j in S_last(i)} deg(j)."""
    degree = np.diff(A.indptr).astype(np.int64)
    return 1 + sum(np.diff(S.indptr).astype(np.int64) for S in shells) + (shells[-1] @ degree).astype(np.int64)


def largest_visited_set(shells):
    """max over the cells of 1 + sum_l |S_l(i)|."""
    return int(1 + np.max(sum(np.diff(S.indptr) for S in shells)))


# ---- (c), (d) the aggregates ---------------------------------------------------------------------------------------------------
def ordered(S, X):
    """(mean, var) over the rows of the shell S in the device's order; an empty row gives zeros."""
    X = np.asarray(X).astype(np.float64)    # float32 is widened on load
    n, d = X.shape
    mean, var = np.zeros((n, d)), np.zeros((n, d))
    ptr, idx = S.indptr, S.indices
    for i in range(n):
        c = ptr[i + 1] - ptr[i]
        if c:
            G = X[idx[ptr[i]:ptr[i + 1]]]
            s = np.cumsum(G, axis=0)[-1]         # ((x_0 + x_1) + x_2) + ...: accumulate is sequential by definition
            q = np.cumsum(G * G, axis=0)[-1]
            m = s / float(c)
            mean[i] = m
            var[i] = q / float(c) - m * m
    return mean, var


def textbook(S, X):
    """(mean, var) as the textbook writes them: the row-normalised shell times X, and times X X minus mean^2."""
    X = np.asarray(X).astype(np.float64)
    c = np.diff(S.indptr).astype(np.float64)
    inv = np.divide(1.0, c, out=np.zeros_like(c), where=c > 0)
    N = sparse.diags(inv) @ S
    mean = N @ X
    return mean, N @ (X * X) - mean * mean


def bounds(S, X):
    """The first-order bounds on |ordered - textbook| per entry, c = the row's length, u = 2^-53:
    mean 2 (c + 2) u sum|x_j| / c, variance 4 (c + 2) u sum x_j^2 / c (0 for an empty row)."""
    X = np.abs(np.asarray(X).astype(np.float64))
    c = np.diff(S.indptr).astype(np.float64)[:, None]
    safe = np.maximum(c, 1.0)
    return 2 * (c + 2) * U * (S @ X) / safe, 4 * (c + 2) * U * (S @ (X * X)) / safe


def features(A, X, layers, aggs):
    """The columns aggregate_neighbors writes: layers ascending, inside a layer >= 1 the aggregations in the order given."""
    layers = sorted(layers)
    shells = shells_textbook(A, max(max(layers), 1))
    blocks = []
    for l in layers:
        if l == 0:
            blocks.append(np.asarray(X).astype(np.float64))
            continue
        mean, var = ordered(shells[l - 1], X)
        blocks.extend(mean if a == "mean" else var for a in aggs)
    return np.concatenate(blocks, axis=1)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def ari(a, b) -> float:
    """Adjusted Rand index of two labelings (Hubert & Arabie 1985)."""
    _, ai = np.unique(np.asarray(a), return_inverse=True)
    _, bi = np.unique(np.asarray(b), return_inverse=True)
    table = np.zeros((ai.max() + 1, bi.max() + 1), dtype=np.int64)
    np.add.at(table, (ai, bi), 1)
    pairs = lambda v: float(np.sum(v * (v - 1) // 2))   # noqa: E731
    together, rows, cols, total = pairs(table), pairs(table.sum(axis=1)), pairs(table.sum(axis=0)), pairs(np.int64(ai.size))
    expected = rows * cols / total
    return (together - expected) / (0.5 * (rows + cols) - expected)


# ---- the shared cases ----------------------------------------------------------------------------------------------------------
KNN_CASES = {"knn3000k6": (3000, 6, 3, 11), "knn3000k15": (3000, 15, 3, 12), "knn2000k6L6": (2000, 6, 6, 13)}   # n, k, L, seed


@functools.lru_cache(maxsize=None)
def knn_case(name):
    n, k, L, seed = KNN_CASES[name]
    return knn_union(uniform_points(n, seed), k), L


def domain_recipe(seed, n=4000, d=8):
    """The end-to-end recipe: two domains split at x = 0.5, two cell types mixed 0.7 / 0.3 and 0.3 / 0.7, an embedding whose
    type centres are 3 normal(2, d).  (xy, X, domain)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(size=(n, 2))
    domain = (xy[:, 0] > 0.5).astype(np.int64)
    kind = (rng.uniform(size=n) >= np.where(domain == 0, 0.7, 0.3)).astype(np.int64)   # type 0 with probability 0.7 / 0.3
    X = 3.0 * rng.normal(size=(2, d))[kind] + rng.normal(size=(n, d))
    return xy, X, domain
