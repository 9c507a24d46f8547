"""Test infrastructure: sc_nmf_fit restated in numpy (include/spatialcore_hip.h, N12).

``ordered`` follows the device's documented summation order term for term, so its W and H must equal the device's bit
for bit (they involve + x / only); ``dense`` is the same definition on a dense matrix with numpy's own matrix
products, i.e. in no particular order.  Both take a canonical scipy CSR and return a dict with the keys of
``Context.nmf_fit``.  ``np.add.accumulate`` is numpy's strictly sequential running sum: its last entry is the sum in
index order from 0."""

import numpy as np
from scipy import sparse

EPS = float(np.finfo(np.float32).eps)      # 2^-23, sklearn's EPSILON
TINY = float(np.finfo(np.float64).eps)     # 2^-52
COL_CHUNK = 512                            # stored entries of a gene column per partial sum
CELL_CHUNK = 1024                          # cells per partial sum
LOSS_FRO, LOSS_KL = "frobenius", "kullback-leibler"


def w_rows_per_workgroup(K: int) -> int:
    """Rows a workgroup of the device's W pass holds (256 threads, K rounded up to a power of two lanes per row)."""
    kp = 1
    while kp < K:
        kp *= 2
    return 256 // kp


def _seq(a, axis):
    """Sum along ``axis`` in index order from 0."""
    if a.shape[axis] == 0:
        return np.zeros(a.shape[:axis] + a.shape[axis + 1:])
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def _seg_sum(vals, ptr):
    """out[s] = vals[ptr[s]] + vals[ptr[s] + 1] + ... in index order from 0, for every segment s."""
    ptr = np.asarray(ptr, dtype=np.int64)
    lens = np.diff(ptr)
    out = np.zeros((lens.size,) + vals.shape[1:])
    for j in range(int(lens.max()) if lens.size else 0):
        m = np.nonzero(lens > j)[0]
        out[m] = out[m] + vals[ptr[m] + j]
    return out


def _tree(prod):
    """The adjacent-pair tree over the last axis, padded with zeros to a power of two."""
    K = prod.shape[-1]
    kp = 1
    while kp < K:
        kp *= 2
    v = np.zeros(prod.shape[:-1] + (kp,))
    v[..., :K] = prod
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _chunks(ptr, size):
    """Boundaries of the pieces of ``size`` entries of every segment, and the first piece of every segment."""
    bounds, first = [], [0]
    for a, b in zip(ptr[:-1], ptr[1:]):
        bounds.extend(range(int(a), int(b), size))
        first.append(len(bounds))
    return np.asarray(bounds + [int(ptr[-1])], dtype=np.int64), np.asarray(first, dtype=np.int64)


class _Ordered:
    def __init__(self, X, K, loss):
        X = sparse.csr_matrix(X, dtype=np.float64)
        assert X.has_canonical_format
        self.n, self.G = X.shape
        self.K, self.loss = K, loss
        self.indptr = X.indptr.astype(np.int64)
        self.col = X.indices.astype(np.int64)
        self.x = X.data.astype(np.float64)
        self.row = np.repeat(np.arange(self.n), np.diff(self.indptr))
        order = np.lexsort((self.row, self.col))            # by column, rows ascending inside a column
        self.c_row, self.c_col, self.c_x = self.row[order], self.col[order], self.x[order]
        colptr = np.concatenate([[0], np.cumsum(np.bincount(self.col, minlength=self.G))])
        self.chunk_ptr, self.gene_first_chunk = _chunks(colptr, COL_CHUNK)
        self.cell_ptr = np.asarray(list(range(0, self.n, CELL_CHUNK)) + [self.n], dtype=np.int64)
        self.sumsq = float(_seq(self.x * self.x, 0))
        self.sumpos = float(_seq(self.x[self.x > EPS], 0))

    # ---- small sums ----
    def hprep(self, H):
        HHt = _seq(H[:, None, :] * H[None, :, :], 2)
        return HHt, _seq(H, 1)

    def cellsums(self, W):
        vals = W[:, :, None] * W[:, None, :] if self.loss == LOSS_FRO else W
        parts = np.stack([_seq(vals[a:b], 0) for a, b in zip(self.cell_ptr[:-1], self.cell_ptr[1:])])
        return _seq(parts, 0)

    # ---- passes ----
    def w_pass(self, W, H, HHt, Hsum):
        Ht = H.T
        if self.loss == LOSS_FRO:
            num = _seg_sum(self.x[:, None] * Ht[self.col], self.indptr)
            den = _seq(W[:, :, None] * HHt[None, :, :], 1)
        else:
            d = _tree(W[self.row] * Ht[self.col])
            d = np.where(d < EPS, EPS, d)
            num = _seg_sum((self.x / d)[:, None] * Ht[self.col], self.indptr)
            den = np.broadcast_to(Hsum[None, :], W.shape).copy()
        den[den == 0] = EPS
        return W * (num / den)

    def h_pass(self, W, H, cellsum):
        if self.loss == LOSS_FRO:
            vals = W[self.c_row] * self.c_x[:, None]
        else:
            d = _tree(W[self.c_row] * H.T[self.c_col])
            d = np.where(d < EPS, EPS, d)
            vals = W[self.c_row] * (self.c_x / d)[:, None]
        part = _seg_sum(vals, self.chunk_ptr)                 # [chunk][k]
        num = _seg_sum(part, self.gene_first_chunk).T         # [k][g]
        if self.loss == LOSS_FRO:
            den = _seq(cellsum[:, :, None] * H[None, :, :], 1)
            den[den == 0] = EPS
        else:
            den = cellsum.copy()
            den[den == 0] = 1.0
            den = np.broadcast_to(den[:, None], H.shape)
        Hn = H * (num / den)
        if self.loss == LOSS_KL:
            Hn[Hn < TINY] = 0.0
        return Hn

    def error(self, W, H):
        HHt, Hsum = self.hprep(H)
        cs = self.cellsums(W)
        d = _tree(W[self.row] * H.T[self.col])
        if self.loss == LOSS_FRO:
            terms = self.x * d
        else:
            d = np.where(d < EPS, EPS, d)
            terms = np.zeros_like(self.x)
            big = self.x > EPS
            terms[big] = self.x[big] * np.log(self.x[big] / d[big])
        # (entries with x <= EPS are skipped on the device; their + 0.0 here changes no bit)
        rowerr = _seg_sum(terms, self.indptr)
        s = float(_seq(_seg_sum(rowerr, self.cell_ptr), 0))
        if self.loss == LOSS_FRO:
            tr = float(_seq((cs * HHt.T).ravel(), 0))
            D = ((self.sumsq + tr) - 2.0 * s) / 2.0
        else:
            sw = float(_seq(cs * Hsum, 0))
            D = s + (sw - self.sumpos)
        return float(np.sqrt(2.0 * max(D, 0.0)))


def ordered(X, W0, H0, loss, update_H=True, max_iter=200, tol=1e-4):
    W, H = np.array(W0, dtype=np.float64), np.array(H0, dtype=np.float64)
    o = _Ordered(X, W.shape[1], loss)
    return _loop(o.error, o.hprep, o.w_pass, lambda W, H: o.h_pass(W, H, o.cellsums(W)), W, H, update_H, max_iter, tol)


def _loop(error, hprep, w_pass, h_pass, W, H, update_H, max_iter, tol):
    e0 = error(W, H)
    trace, prev, e, n_iter, checked = [e0], e0, e0, 0, 0
    for it in range(1, max_iter + 1):
        if update_H or it == 1:
            HHt, Hsum = hprep(H)
        W = w_pass(W, H, HHt, Hsum)
        if update_H:
            H = h_pass(W, H)
        n_iter = it
        if tol > 0 and it % 10 == 0:
            e = error(W, H)
            trace.append(e)
            checked = it
            with np.errstate(invalid="ignore", divide="ignore"):
                stop = (np.float64(prev) - e) / np.float64(e0) < tol
            if stop:
                break
            prev = e
    if checked != n_iter:
        e = error(W, H)
    return {"W": W, "H": H, "n_iter": n_iter, "reconstruction_err": e, "error_trace": np.asarray(trace)}


def dense(X, W0, H0, loss, update_H=True, max_iter=200, tol=1e-4):
    """The same definition with numpy's matrix products on the dense matrix (no particular summation order)."""
    A = np.asarray(sparse.csr_matrix(X, dtype=np.float64).todense())
    stored = A != 0
    W, H = np.array(W0, dtype=np.float64), np.array(H0, dtype=np.float64)

    def quotient(W, H):
        return np.where(stored, A / np.maximum(W @ H, EPS), 0.0)

    def hprep(H):
        return H @ H.T, H.sum(axis=1)

    def w_pass(W, H, HHt, Hsum):
        if loss == LOSS_FRO:
            num, den = A @ H.T, W @ HHt
        else:
            num, den = quotient(W, H) @ H.T, np.broadcast_to(Hsum[None, :], W.shape).copy()
        den[den == 0] = EPS
        return W * (num / den)

    def h_pass(W, H):
        if loss == LOSS_FRO:
            num, den = W.T @ A, (W.T @ W) @ H
            den[den == 0] = EPS
        else:
            ws = W.sum(axis=0)
            ws[ws == 0] = 1.0
            num, den = W.T @ quotient(W, H), ws[:, None]
        Hn = H * (num / den)
        if loss == LOSS_KL:
            Hn[Hn < TINY] = 0.0
        return Hn

    def error(W, H):
        WH = W @ H
        if loss == LOSS_FRO:
            D = ((A[stored] ** 2).sum() + np.trace((W.T @ W) @ (H @ H.T)) - 2.0 * (A[stored] * WH[stored]).sum()) / 2.0
        else:
            big = A > EPS
            D = (A[big] * np.log(A[big] / np.maximum(WH[big], EPS))).sum() + (W.sum(axis=0) @ H.sum(axis=1) - A[big].sum())
        return float(np.sqrt(2.0 * max(D, 0.0)))

    return _loop(error, hprep, w_pass, h_pass, W, H, update_H, max_iter, tol)


# ---- inputs of the tests ---------------------------------------------------------------------------------------------
def counts(n, G, programs, seed, scale=6.0):
    """Gamma programs x Dirichlet usages -> Poisson counts (float64 CSR), with two all-zero cells (one of them the last)
    and two all-zero genes (one of them the last) planted."""
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.6, 1.0, size=(programs, G))
    U = rng.dirichlet(np.full(programs, 0.4), size=n)
    A = rng.poisson(scale * (U @ P)).astype(np.float64)
    A[n // 3] = 0
    A[-1] = 0
    A[:, G // 2] = 0
    A[:, -1] = 0
    return sparse.csr_matrix(A)


def start(X, K, seed):
    """sklearn's init="random" for this matrix (the draws of _initialize_nmf)."""
    from spatialcore_amd.nmf.factorize import random_init

    avg = float(np.sqrt(sparse.csr_matrix(X, dtype=np.float64).mean() / K))
    return random_init(avg, X.shape[0], X.shape[1], K, seed)


def guard_margin(trace, tol):
    """Smallest |(prev - e) / e0 - tol| / tol over the checks of an error trace (sklearn's stopping rule)."""
    t = np.asarray(trace, dtype=np.float64)
    if t.size < 2:
        return np.inf
    return float(np.min(np.abs((t[:-1] - t[1:]) / t[0] - tol)) / tol)


def sklearn_fit(X, W0, H0, loss, max_iter=200, tol=1e-4):
    """sklearn's own result from the same start: W, H, n_iter, reconstruction_err."""
    import warnings

    from sklearn.decomposition import NMF

    m = NMF(n_components=W0.shape[1], init="custom", solver="mu", beta_loss=loss, max_iter=max_iter, tol=tol)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W = m.fit_transform(sparse.csr_matrix(X, dtype=np.float64), W=W0.copy(), H=H0.copy())
    return {"W": W, "H": m.components_, "n_iter": m.n_iter_, "reconstruction_err": float(m.reconstruction_err_), "model": m}
