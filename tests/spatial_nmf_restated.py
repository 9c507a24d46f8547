"""Test infrastructure: sc_nmf_fit_graph restated in numpy (include/spatialcore_hip.h, N12).

Graph-regularised NMF (Cai, He, Han & Huang 2011), Frobenius loss:

    F(W, H) = 1/2 ||X - W H||_F^2 + (lam / 2) tr(W^T L W),   L = diag(d) - A,   d_i = sum_j a_ij
    W_ik <- W_ik ((X H^T)_ik + lam (A W)_ik) / ((W H H^T)_ik + lam d_i W_ik),   H as the plain Frobenius pass

``ordered`` follows the device's documented summation order term for term (on top of ``nmf_restated``'s, whose helpers
it uses), so W, H, both traces and the penalty must equal the device's bit for bit; ``dense`` is the same definition
with scipy / numpy products, in no particular order.  Both take a canonical scipy CSR ``X``, a symmetric scipy CSR ``A``
(no diagonal, weights > 0) and return the keys of ``Context.nmf_fit_graph``."""

import numpy as np
from scipy import sparse

from nmf_restated import EPS, LOSS_FRO, _Ordered, _seg_sum, _seq, _tree


def _graph_arrays(A, n):
    A = sparse.csr_matrix(A, dtype=np.float64)
    assert A.shape == (n, n) and A.has_canonical_format
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)


class _OrderedGraph(_Ordered):
    def __init__(self, X, K, A, lam):
        super().__init__(X, K, LOSS_FRO)
        self.lam = float(lam)
        self.gptr, self.gcol, self.a = _graph_arrays(A, self.n)
        self.grow = np.repeat(np.arange(self.n), np.diff(self.gptr))
        self.deg = _seg_sum(self.a, self.gptr)                  # d_i: the row's weights in index order from 0

    def w_terms(self, W, H, HHt):
        """(num, den) of the W pass before the den == 0 -> EPS guard."""
        Ht = H.T
        nx = _seg_sum(self.x[:, None] * Ht[self.col], self.indptr)
        dx = _seq(W[:, :, None] * HHt[None, :, :], 1)
        g = _seg_sum(self.a[:, None] * W[self.gcol], self.gptr)
        num = nx + self.lam * g
        den = dx + (self.lam * self.deg)[:, None] * W
        return num, den

    def w_pass(self, W, H, HHt, Hsum):
        """Jacobi: every row reads the W it was handed, the previous iteration's, for its neighbours."""
        num, den = self.w_terms(W, H, HHt)
        den[den == 0] = EPS
        return W * (num / den)

    def row_penalties(self, W):
        """r_i = sum_e a_e T_k((w_ik - w_jk)^2), the graph row's stored entries in index order from 0."""
        diff = W[self.grow] - W[self.gcol]
        return _seg_sum(self.a * _tree(diff * diff), self.gptr)

    def penalty(self, W):
        """tr(W^T L W) = R / 2, R = sum_i r_i, cells in chunks of 1024."""
        R = float(_seq(_seg_sum(self.row_penalties(W), self.cell_ptr), 0))
        return R / 2.0

    def evaluate(self, W, H):
        """(sqrt(2 max(D, 0)), sqrt(2 max(F, 0)), tr(W^T L W)) with D as nmf_restated's Frobenius D."""
        HHt, _ = self.hprep(H)
        cs = self.cellsums(W)
        rowerr = _seg_sum(self.x * _tree(W[self.row] * H.T[self.col]), self.indptr)
        s = float(_seq(_seg_sum(rowerr, self.cell_ptr), 0))
        tr = float(_seq((cs * HHt.T).ravel(), 0))
        D = ((self.sumsq + tr) - 2.0 * s) / 2.0
        pen = self.penalty(W)
        F = D + (self.lam * pen) / 2.0
        return float(np.sqrt(2.0 * max(D, 0.0))), float(np.sqrt(2.0 * max(F, 0.0))), pen


def _loop(evaluate, hprep, w_pass, h_pass, W, H, max_iter, tol):
    """sklearn's schedule on the objective; the check runs at every tenth iteration whatever tol is, and stops only
    with tol > 0."""
    err0, e0, _ = evaluate(W, H)
    errs, objs, prev, n_iter, checked = [err0], [e0], e0, 0, 0
    last = (err0, e0, None)
    for it in range(1, max_iter + 1):
        HHt, Hsum = hprep(H)
        W = w_pass(W, H, HHt, Hsum)
        H = h_pass(W, H)
        n_iter = it
        if it % 10 == 0:
            last = evaluate(W, H)
            errs.append(last[0])
            objs.append(last[1])
            checked = it
            if tol > 0:
                with np.errstate(invalid="ignore", divide="ignore"):
                    stop = (np.float64(prev) - last[1]) / np.float64(e0) < tol
                if stop:
                    break
                prev = last[1]
    if checked != n_iter:
        last = evaluate(W, H)
    return {"W": W, "H": H, "n_iter": n_iter, "reconstruction_err": last[0], "penalty": last[2],
            "error_trace": np.asarray(errs), "objective_trace": np.asarray(objs)}


def ordered(X, A, lam, W0, H0, max_iter=200, tol=1e-4):
    W, H = np.array(W0, dtype=np.float64), np.array(H0, dtype=np.float64)
    o = _OrderedGraph(X, W.shape[1], A, lam)
    return _loop(o.evaluate, o.hprep, o.w_pass, lambda W, H: o.h_pass(W, H, o.cellsums(W)), W, H, max_iter, tol)


def dense(X, A, lam, W0, H0, max_iter=200, tol=1e-4):
    """The same definition with scipy's and numpy's products (no particular summation order)."""
    Xd = np.asarray(sparse.csr_matrix(X, dtype=np.float64).todense())
    A = sparse.csr_matrix(A, dtype=np.float64)
    d = np.asarray(A.sum(axis=1)).ravel()
    lam = float(lam)
    W, H = np.array(W0, dtype=np.float64), np.array(H0, dtype=np.float64)

    def hprep(H):
        return H @ H.T, None

    def w_pass(W, H, HHt, _):
        num = Xd @ H.T + lam * (A @ W)
        den = W @ HHt + lam * d[:, None] * W
        den[den == 0] = EPS
        return W * (num / den)

    def h_pass(W, H):
        num, den = W.T @ Xd, (W.T @ W) @ H
        den[den == 0] = EPS
        return H * (num / den)

    def evaluate(W, H):
        D = 0.5 * float(((Xd - W @ H) ** 2).sum())
        pen = float((W * (d[:, None] * W - A @ W)).sum())
        F = D + lam * pen / 2.0
        return float(np.sqrt(2.0 * max(D, 0.0))), float(np.sqrt(2.0 * max(F, 0.0))), pen

    return _loop(evaluate, hprep, w_pass, h_pass, W, H, max_iter, tol)


def roughness(W, A):
    """Scale-invariant roughness sum_ij a_ij ||w^_i - w^_j||^2 with the columns of W scaled to unit norm."""
    A = sparse.coo_matrix(A)
    norms = np.linalg.norm(W, axis=0)
    Wn = W / np.where(norms > 0, norms, 1.0)
    return float((A.data * ((Wn[A.row] - Wn[A.col]) ** 2).sum(axis=1)).sum())


# ---- inputs of the tests ---------------------------------------------------------------------------------------------
def planted(n, G, P, seed):
    """Uniform coordinates in the unit square, Gaussian-bump usages around P random centres (sigma = 0.15 of the extent),
    Gamma(0.6) programs, Poisson(6 U P) counts: (X float64 CSR, xy, U)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 1.0, size=(n, 2))
    centres = rng.uniform(0.0, 1.0, size=(P, 2))
    d2 = ((xy[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)
    U = np.exp(-d2 / (2.0 * 0.15 ** 2))
    prog = rng.gamma(0.6, 1.0, size=(P, G))
    X = rng.poisson(6.0 * (U @ prog)).astype(np.float64)
    return sparse.csr_matrix(X), xy, U


def _symmetric_csr(rows, cols, vals, n):
    A = sparse.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def knn_union(xy, k):
    """The symmetric union of the k-nearest-neighbour lists (scipy.spatial.cKDTree), weight 1.0, no diagonal."""
    from scipy.spatial import cKDTree

    n = xy.shape[0]
    _, idx = cKDTree(xy).query(xy, k=k + 1)
    rows = np.repeat(np.arange(n), k + 1)
    cols = idx.ravel()
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    pairs = np.unique(np.stack([np.minimum(rows, cols), np.maximum(rows, cols)], axis=1), axis=0)
    r = np.concatenate([pairs[:, 0], pairs[:, 1]])
    c = np.concatenate([pairs[:, 1], pairs[:, 0]])
    return _symmetric_csr(r, c, np.ones(r.size), n)


def edge_degrees(kp):
    """The degrees edge_graph plants on purpose, besides 0 (the isolated cell 0) and 1 (the chain's end n - 1)."""
    return sorted({d for d in (3, 4, 5, kp - 1, kp, kp + 1) if d >= 3})


def edge_graph(n, kp, seed):
    """A symmetric graph for the lane and workgroup edges of the W pass (kp = the lanes of a row's group):
     - cell 0 is isolated (degree 0); a chain i -- i + 1 runs over the cells 1 .. n - 1, so neighbours sit in other
       workgroups whatever the rows per workgroup are, and its end n - 1 has degree 1;
     - one cell each of degree 3, 4, 5, kp - 1, kp, kp + 1 (those >= 3: a fetch of the group just not filled, just
       filled, one entry into the second) and one hub of degree 2 kp + 3, reached by extra edges to cells that are
       not special themselves;
     - weights symmetric, uniform in [0.1, 3].
    Returns (A, special) with special = {degree: cell}."""
    rng = np.random.default_rng(seed)
    degs = sorted(set(edge_degrees(kp)) | {2 * kp + 3})   # kp = 1: the hub is the cell of degree 5
    assert n >= max(2 * kp + len(degs) + 8, 3 * len(degs) + 16), "too few cells for the hub"
    # special cells sit three apart in the first half of the chain: never adjacent, never each other's chain neighbours
    special = {d: 5 + 3 * q for q, d in enumerate(degs)}
    reserved = set(special.values()) | {0, 1, n - 1, n - 2}
    edges = {(i, i + 1) for i in range(1, n - 1)}
    fillers = np.asarray([i for i in range(1, n - 1) if i not in reserved])
    for d, cell in special.items():
        cand = fillers[np.abs(fillers - cell) > 1]
        for j in rng.choice(cand, size=d - 2, replace=False):
            edges.add((min(cell, int(j)), max(cell, int(j))))
    e = np.asarray(sorted(edges), dtype=np.int64)
    w = rng.uniform(0.1, 3.0, size=e.shape[0])
    A = _symmetric_csr(np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), np.concatenate([w, w]), n)
    special = {**special, 0: 0, 1: n - 1}
    deg = np.diff(A.indptr)
    assert all(deg[c] == d for d, c in special.items())
    return A, special
