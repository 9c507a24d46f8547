"""A plain numpy / Python-integer restatement of spatialcore_amd.cluster.louvain: synchronous Louvain
rounds with the alternating direction rule, a connectivity split of the best partition, aggregation, all in exact integer
arithmetic.  It shares no code with the native layer and returns the per-level record sc_louvain_level returns.

Qnum and the reported S are Python integers.  The per-candidate S of a round, of which there are as many as stored
entries, are compared as two 64-bit limbs in numpy (mul_u64 / s_limbs below, themselves checked against Python integers
by tests/test_cpu_louvain.py), because a Python loop over them would take minutes on the recipes.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

G_ONE = 1 << 16
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def canonical(A):
    """scipy matrix -> (indptr int64, indices int32, q int64) with sorted, unique columns"""
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.int64)


def quantise(w):
    """q = max(1, rint(w / w_max * 65535)) and the scale w_max / 65535"""
    w = np.asarray(w, dtype=np.float64)
    w_max = float(w.max()) if w.size else 1.0
    q = np.maximum(1, np.rint(w / w_max * 65535.0)).astype(np.int64)
    return q, w_max / 65535.0


def resolution_g(resolution):
    return int(np.rint(float(resolution) * G_ONE))


def mul_u64(a, b):
    """(hi, lo) uint64 limbs of the 128-bit product of two uint64 arrays"""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    a0, a1, b0, b1 = a & MASK32, a >> S32, b & MASK32, b >> S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> S32) + (p01 & MASK32) + (p10 & MASK32)
    lo = (p00 & MASK32) | ((mid & MASK32) << S32)
    hi = p11 + (p01 >> S32) + (p10 >> S32) + (mid >> S32)
    return hi, lo


def s_limbs(M, g, kic, ki, t):
    """S = 2^16 M kic - g ki t as (hi int64, lo uint64): two's complement limbs of a signed 128-bit integer.
    2^16 M < 2^63, kic <= M < 2^47, g <= 2^23, ki t < 2^94: every product stays below 2^117."""
    ah, al = mul_u64(np.uint64(M << 16), kic)
    bh, bl = mul_u64(ki, t)                      # ki t, then times g limb by limb
    ch, cl = mul_u64(bl, np.uint64(g))
    ch = ch + bh * np.uint64(g)
    lo = al - cl
    hi = ah - ch - (al < cl).astype(np.uint64)
    return hi.view(np.int64), lo


def qnum(indptr, indices, data, k, comm, M, g):
    """(Qnum, in-community weight, sum of tot^2) as Python integers"""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    inside = int(data[comm[rows] == comm[indices]].sum())
    tot = np.zeros(n, dtype=np.int64)
    np.add.at(tot, comm, k)
    sq = sum(int(t) * int(t) for t in tot[tot > 0])
    return G_ONE * M * inside - g * sq, inside, sq


def one_round(indptr, indices, data, k, comm, M, g, r, record):
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    off = rows != indices
    tot = np.zeros(n, dtype=np.int64)
    np.add.at(tot, comm, k)
    # the candidates of vertex i: its neighbours' communities and, with weight 0 if need be, its own
    ci = np.concatenate([rows[off], np.arange(n, dtype=np.int64)])
    cc = np.concatenate([comm[indices[off]].astype(np.int64), comm.astype(np.int64)])
    cw = np.concatenate([data[off], np.zeros(n, dtype=np.int64)])
    order = np.lexsort((cc, ci))
    ci, cc, cw = ci[order], cc[order], cw[order]
    head = np.ones(len(ci), dtype=bool)
    head[1:] = (ci[1:] != ci[:-1]) | (cc[1:] != cc[:-1])
    start = np.flatnonzero(head)
    kic = np.add.reduceat(cw, start)
    ci, cc = ci[start], cc[start]
    own = cc == comm[ci]
    t = tot[cc] - np.where(own, k[ci], 0)
    hi, lo = s_limbs(M, g, kic, k[ci], t)
    if record is not None and len(kic):
        big = int(np.argmax(kic))
        s_big = G_ONE * M * int(kic[big]) - g * int(k[ci[big]]) * int(t[big])
        record["max_abs_S"] = max(record.get("max_abs_S", 0), abs(s_big), G_ONE * M * int(kic[big]))
    allowed = own | ((cc > comm[ci]) if r % 2 == 0 else (cc < comm[ci]))
    ci, cc, hi, lo, own = ci[allowed], cc[allowed], hi[allowed], lo[allowed], own[allowed]
    # per vertex: largest S, then the current community, then the lowest c
    order = np.lexsort((cc, ~own, ~lo, ~hi, ci))
    ci, cc = ci[order], cc[order]
    first = np.ones(len(ci), dtype=bool)
    first[1:] = ci[1:] != ci[:-1]
    new = comm.copy()
    new[ci[first]] = cc[first]
    return new


def split(indptr, indices, comm):
    """components of the edges inside communities, numbered by their smallest vertex, ascending"""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    keep = (comm[rows] == comm[indices]) & (rows != indices)
    B = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int8), (rows[keep], indices[keep])), shape=(n, n))
    _, lab = connected_components(B, directed=False)
    _, first = np.unique(lab, return_index=True)       # smallest vertex of each component
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[lab].astype(np.int32)


def aggregate(indptr, indices, data, label, nc):
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    B = sp.coo_matrix((data, (label[rows], label[indices])), shape=(nc, nc)).tocsr()
    return canonical(B)


def one_level(indptr, indices, data, M, g, max_rounds, record=None):
    n = len(indptr) - 1
    k = np.zeros(n, dtype=np.int64)
    np.add.at(k, np.repeat(np.arange(n), np.diff(indptr)), data)
    comm = np.arange(n, dtype=np.int32)
    best = comm.copy()
    best_q = qnum(indptr, indices, data, k, comm, M, g)
    stale = rounds = 0
    while rounds < max_rounds and stale < 2:
        comm = one_round(indptr, indices, data, k, comm, M, g, rounds, record)
        rounds += 1
        q = qnum(indptr, indices, data, k, comm, M, g)
        if q[0] > best_q[0]:
            best, best_q, stale = comm.copy(), q, 0
        else:
            stale += 1
    label = split(indptr, indices, best)
    nc = int(label.max()) + 1
    tot = np.zeros(nc, dtype=np.int64)
    np.add.at(tot, label, k)
    q_split = G_ONE * M * best_q[1] - g * sum(int(t) * int(t) for t in tot)
    return {"n_vertices": n, "rounds": rounds, "n_best": int(len(np.unique(best))), "n_communities": nc, "qnum": q_split,
            "labels": label, "hit_max_rounds": bool(stale < 2)}


def rank_by_size(label):
    """clusters numbered by descending size, ties to the smaller smallest-member index"""
    _, first, inverse, counts = np.unique(label, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -counts))
    rank = np.empty(len(order), dtype=np.int32)
    rank[order] = np.arange(len(order), dtype=np.int32)
    return rank[inverse]


def louvain(indptr, indices, q, g, max_rounds=500, record=None):
    """-> (final labels int32, levels, M).  `record`, a dict, receives max_abs_S: the largest |term of S| met."""
    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int32), np.asarray(q, np.int64)
    n = len(indptr) - 1
    M = int(data.sum())
    mapping = np.arange(n, dtype=np.int32)
    levels = []
    while True:
        lv = one_level(indptr, indices, data, M, g, max_rounds, record)
        levels.append(lv)
        if lv["n_communities"] == lv["n_vertices"]:
            break
        mapping = lv["labels"][mapping]
        indptr, indices, data = aggregate(indptr, indices, data, lv["labels"], lv["n_communities"])
    return rank_by_size(mapping), levels, M


def modularity(levels, M):
    return levels[-1]["qnum"] / (G_ONE * M * M) if M else 0.0


# ---- the recipes of the tests: kNN graphs (symmetric union) of point clouds, built with numpy alone ----------------------
def knn_union(X, k):
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    sq = (X * X).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * X @ X.T
    d2[np.arange(n), np.arange(n)] = np.inf
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    rows = np.repeat(np.arange(n), k)
    A = sp.csr_matrix((np.ones(n * k), (rows, idx.ravel())), shape=(n, n))
    A = ((A + A.T) > 0).astype(np.float64)
    return sp.csr_matrix(A)


def blobs(n, centres, dim, spread, seed):
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(centres, dim)) * 10.0
    lab = np.arange(n) % centres
    return C[lab] + rng.normal(size=(n, dim)) * spread, lab


def symmetric_integer_weights(A, seed, lo=1, hi=65535):
    """the pattern of A with random integer weights in [lo, hi], w_ij = w_ji"""
    A = sp.triu(sp.csr_matrix(A), k=0).tocoo()
    rng = np.random.default_rng(seed)
    w = rng.integers(lo, hi + 1, size=A.nnz).astype(np.float64)
    U = sp.csr_matrix((w, (A.row, A.col)), shape=A.shape)
    return sp.csr_matrix(U + sp.triu(U, k=1).T)


def recipe(name):
    """-> (symmetric scipy matrix with integer weights in [1, 65535], planted labels or None)"""
    if name == "blobs_binary":
        X, lab = blobs(2000, 8, 10, 1.0, BLOB_SEED)
        return knn_union(X, 15), lab
    if name == "blobs_weighted":
        X, lab = blobs(2000, 8, 10, 1.0, BLOB_SEED)
        return symmetric_integer_weights(knn_union(X, 15), 2), lab
    if name == "overlap":
        rng = np.random.default_rng(3)
        C = rng.normal(size=(6, 5)) * 2.0
        lab = np.arange(2000) % 6
        return symmetric_integer_weights(knn_union(C[lab] + rng.normal(size=(2000, 5)), 15), 4), lab
    if name == "uniform":
        return knn_union(np.random.default_rng(UNIFORM_SEED).uniform(size=(3000, 2)), 15), None
    if name == "two_blobs":
        X, lab = blobs(400, 2, 3, 0.5, 5)
        return knn_union(X, 6), lab
    raise KeyError(name)


BLOB_SEED = 2       # chosen on the CPU with this restatement and networkx alone: see tests/test_cpu_louvain.py
UNIFORM_SEED = 0    # ... so that a level of the uniform recipe has more components than communities (the split)


# ---- the edge shapes of tests/test_gpu_louvain.py, against sc_louvain.hip's row classes (<= 64, <= 2048, more entries) ----
def from_edges(n, edges, weights=None):
    """the symmetric matrix of an edge list (i, j), i != j or a loop, weight 1 or weights[e]"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(e)) if weights is None else np.asarray(weights, dtype=np.float64)
    loop = e[:, 0] == e[:, 1]
    rows = np.concatenate([e[:, 0], e[~loop, 1]])
    cols = np.concatenate([e[:, 1], e[~loop, 0]])
    A = sp.csr_matrix((np.concatenate([w, w[~loop]]), (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    A.data[:] = np.minimum(A.data, 65535.0) if weights is not None else 1.0
    return A


def pair():
    return from_edges(2, [(0, 1)])


def triangle_and_isolated():
    return from_edges(4, [(0, 1), (1, 2), (0, 2)])


def hubs(degrees=(63, 64, 65, 300)):
    """hubs with rows of exactly `degrees` entries over their own leaves; leaves 2 q and 2 q + 1 of a hub are joined"""
    n = len(degrees) + sum(degrees)
    edges, leaf = [], len(degrees)
    for h, d in enumerate(degrees):
        edges += [(h, leaf + q) for q in range(d)]
        edges += [(leaf + q, leaf + q + 1) for q in range(0, d - 1, 2)]
        leaf += d
    A = from_edges(n, edges)
    assert tuple(np.diff(A.indptr)[:len(degrees)]) == tuple(degrees)
    return A


def star(leaves=20000, extra=300, seed=7):
    """one hub whose row is longer than any LDS table, and a few hundred random edges among the leaves"""
    rng = np.random.default_rng(seed)
    ij = rng.integers(1, leaves + 1, size=(extra, 2))
    ij = ij[ij[:, 0] != ij[:, 1]]
    return from_edges(leaves + 1, [(0, q) for q in range(1, leaves + 1)] + [tuple(r) for r in ij])


def clique_ring(cliques=40, size=60):
    edges = []
    for c in range(cliques):
        base = c * size
        edges += [(base + a, base + b) for a in range(size) for b in range(a + 1, size)]
        edges.append((base + size - 1, ((c + 1) % cliques) * size))
    return from_edges(cliques * size, edges)


def joined_cliques(cliques=150, size=6):
    """heavy cliques of which every two are joined by one light edge: the rows of level 1 have `cliques` entries"""
    edges, w = [], []
    for c in range(cliques):
        base = c * size
        for a in range(size):
            for b in range(a + 1, size):
                edges.append((base + a, base + b)), w.append(65535)
    for c in range(cliques):
        for d in range(c + 1, cliques):
            edges.append((c * size + d % size, d * size + c % size)), w.append(1)
    return from_edges(cliques * size, edges, w)


def mixed_weights(A, seed=9):
    """the pattern of A with weights 1 or 65535 at random, symmetric"""
    U = sp.triu(sp.csr_matrix(A), k=0).tocoo()
    w = np.where(np.random.default_rng(seed).integers(0, 2, size=U.nnz) == 1, 65535.0, 1.0)
    U = sp.csr_matrix((w, (U.row, U.col)), shape=A.shape)
    return sp.csr_matrix(U + sp.triu(U, k=1).T)
