"""The annotation module's definition restated in numpy -- test infrastructure, never imported by the
product.

 - ``dense_*``: plain numpy on the densified standardised matrix Z;
 - ``ordered_*``: prediction in the device's summation order (bit for bit: + x / only; the transforms use exp);
 - ``sklearn_fit``: T binary ``LogisticRegression(C, solver="newton-cholesky", tol=1e-12)`` fits with sample_weight;
 - ``NumpyProblem``: the training passes of sc_annot_train_* behind the method names of ``_lib.Context``, so that the
   host's optimiser (annotation/training.py: fit) can be run without a device."""
import functools

import numpy as np
from scipy import sparse

COL_CHUNK = 512
CELL_CHUNK = 1024
CLIP = 10.0
# the issue's shapes (n, G, T, seed)
SHAPES = [(300, 9, 2, 31), (777, 37, 5, 32), (2500, 130, 33, 33), (1031, 70, 64, 34)]
WIDE_SHAPES = [(400, 40, 65, 35), (700, 30, 130, 36)]     # past one wavefront of classes


def lanes(T):
    tp = 2
    while tp < T and tp < 64:
        tp *= 2
    return tp


def rows_per_workgroup(T):
    return 256 // lanes(T)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def log1p_10k(counts):
    """log1p(x / rowsum * 1e4) of a CSR of counts, the row sum over the stored entries in index order."""
    C = sparse.csr_matrix(counts, dtype=np.float64)
    C.sort_indices()
    out = C.copy()
    for i in range(C.shape[0]):
        p0, p1 = C.indptr[i], C.indptr[i + 1]
        s = 0.0
        for p in range(p0, p1):
            s = s + C.data[p]
        out.data[p0:p1] = np.log1p((C.data[p0:p1] / s) * 1e4)
    return out


@functools.lru_cache(maxsize=None)
def recipe(n, G, T, seed, held_out=False):
    """Counts (CSR), their log1p(10k) values (CSR, float64), labels (codes) and the special rows / columns: per-class
    Poisson rates log-uniform in [0.02, 3]; gene 0 expressed in 3 cells only (entries with z > 10); gene G // 2 all zero;
    cell n // 3 all zero; cell 1 with every other gene stored; the last class has exactly 5 cells."""
    rng = np.random.default_rng(seed)
    rates = np.exp(rng.uniform(np.log(0.02), np.log(3.0), size=(T, G)))
    rng = np.random.default_rng(seed + (1000 if held_out else 0))
    labels = np.concatenate([np.repeat(np.arange(T), 5), rng.integers(0, T - 1, n - 5 * T)])
    rng.shuffle(labels)
    A = rng.poisson(rates[labels]).astype(np.float64)
    empty, full, zero_gene, rare = n // 3, 1, G // 2, 0
    A[full] = np.maximum(A[full], 1.0)
    A[:, rare] = 0
    others = np.setdiff1d(np.arange(n), [empty, full])
    A[rng.choice(others, 2, replace=False), rare] = 1.0
    A[full, rare] = 3.0
    A[:, zero_gene] = 0
    A[empty] = 0
    counts = sparse.csr_matrix(A)
    return {"counts": counts, "X": log1p_10k(counts), "labels": labels.astype(np.int32), "empty": empty, "full": full,
            "zero_gene": zero_gene, "rare": rare, "n": n, "G": G, "T": T}


def weights_of(labels, T, balance):
    n = labels.size
    return n / (T * np.bincount(labels, minlength=T)[labels]) if balance else np.ones(n)


# ---- scaler and standardised values ------------------------------------------------------------------------------------------
def scaler(X):
    """mean, scale, z0 over the columns of a CSR: the population variance counts the zeros; a constant feature scales by 1."""
    Xd = np.asarray(X.todense(), dtype=np.float64)
    n = Xd.shape[0]
    mean = Xd.sum(axis=0) / n
    var = ((Xd - mean) ** 2).sum(axis=0) / n
    eps = np.finfo(np.float64).eps
    const = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.where(const, 1.0, np.sqrt(var))
    return mean, scale


def dense_z(X, mean, scale):
    return np.minimum((np.asarray(X.todense(), dtype=np.float64) - mean) / scale, CLIP)


def d_values(X, mean, scale):
    """(z0, CSR of d = min((x - mean) / scale, 10) - z0 on X's own pattern)."""
    z0 = (0.0 - mean) / scale
    D = X.copy().astype(np.float64)
    g = D.indices
    D.data = np.minimum((D.data - mean[g]) / scale[g], CLIP) - z0[g]
    return z0, D


def dense_scores(X, coef, intercept, mean, scale):
    return dense_z(X, mean, scale) @ coef.T + intercept


# ---- prediction in the device's order --------------------------------------------------------------------------------------------
def ordered_scores(X, coef, intercept, mean, scale):
    """fp64 scores: base_t = intercept_t + (sum_g z0_g w_tg, gene order from 0), then + d_ig w_tg in column order."""
    z0, D = d_values(X, mean, scale)
    T, G = coef.shape
    b = np.zeros(T)
    for g in range(G):
        b = b + z0[g] * coef[:, g]
    base = intercept + b
    ct = np.ascontiguousarray(coef.T)
    out = np.empty((X.shape[0], T))
    for i in range(X.shape[0]):
        acc = base.copy()
        for p in range(D.indptr[i], D.indptr[i + 1]):
            acc = acc + D.data[p] * ct[D.indices[p]]
        out[i] = acc
    return out, base


def group_sum(V, T):
    """Row sums of V (n, T) in the epilogue's order: lane l adds its classes 64 b + l for b ascending, the lane sums meet
    in the adjacent-pair tree over the group's lanes."""
    tp, nb = lanes(T), (T + 63) // 64
    P = np.zeros((V.shape[0], nb * 64))
    P[:, :T] = V
    P = P.reshape(V.shape[0], nb, 64)[:, :, :tp]
    lane = np.zeros((V.shape[0], tp))
    for b in range(nb):
        lane = lane + P[:, b, :]
    while lane.shape[1] > 1:
        lane = lane[:, 0::2] + lane[:, 1::2]
    return lane[:, 0]


def confidences(F, exp=np.exp):
    """The reference's four transforms of the rows of F (fp64 arithmetic, first argmax), in the epilogue's order."""
    F = np.asarray(F, dtype=np.float64)
    n, T = F.shape
    win = np.argmax(F, axis=1)
    best = F[np.arange(n), win]
    mean = group_sum(F, T) / float(T)
    dev = F - mean[:, None]
    sd = np.sqrt(group_sum(dev * dev, T) / float(T))
    sd = np.where(sd < 1e-10, 1.0, sd)
    zscore = 1.0 / (1.0 + exp(-((best - mean) / sd)))
    softmax = 1.0 / group_sum(exp(F - best[:, None]), T)
    mn = F.min(axis=1)
    rng = best - mn
    rng = np.where(rng < 1e-10, 1.0, rng)
    return {"raw": best, "zscore": zscore, "softmax": softmax, "minmax": (best - mn) / rng, "argmax": win}


def ordered_predict(X, coef, intercept, mean, scale, exp=np.exp):
    S, base = ordered_scores(X, coef, intercept, mean, scale)
    lab = np.argmax(S, axis=1)
    out = confidences(S.astype(np.float32).astype(np.float64), exp)
    out.update(scores64=S, scores=S.astype(np.float32), labels=lab.astype(np.int32), base=base,
               confidence_raw=1.0 / (1.0 + exp(-S[np.arange(S.shape[0]), lab])))
    return out


def ulp_tolerance(fn, keys):
    """16 x the largest change of fn(exp)[key] when every exp result moves by one ulp, per key and element."""
    base = fn(np.exp)
    up = fn(lambda v: np.nextafter(np.exp(v), np.inf))
    dn = fn(lambda v: np.nextafter(np.exp(v), 0.0))
    return base, {k: 16.0 * np.maximum(np.abs(up[k] - base[k]), np.abs(dn[k] - base[k])) for k in keys}


# ---- the objective -----------------------------------------------------------------------------------------------------------
def expit(u):
    return 1.0 / (1.0 + np.exp(-u))


def gradient(Z, labels, s, coef, intercept, C):
    """grad F_t for every class: (T, G + 1), the intercept last."""
    T = coef.shape[0]
    Y = (labels[:, None] == np.arange(T)[None, :]).astype(np.float64)
    R = s[:, None] * (expit(Z @ coef.T + intercept) - Y)
    return np.hstack([R.T @ Z + coef / C, R.sum(axis=0)[:, None]])


def coefficient_bound(Z, s, coef, intercept, C, tol):
    """2 tol sum(s) sqrt(G + 1) / lambda_min(H_t) per class, H_t the Hessian of F_t at (coef, intercept)."""
    n, G = Z.shape
    Za = np.hstack([Z, np.ones((n, 1))])
    pen = np.diag(np.r_[np.full(G, 1.0 / C), 0.0])
    out = np.empty(coef.shape[0])
    for t in range(coef.shape[0]):
        p = expit(Z @ coef[t] + intercept[t])
        H = Za.T @ (Za * (s * p * (1 - p))[:, None]) + pen
        out[t] = 2.0 * tol * s.sum() * np.sqrt(G + 1) / np.linalg.eigvalsh(H)[0]
    return out


def sklearn_fit(Z, labels, s, T, C=1.0):
    from sklearn.linear_model import LogisticRegression

    coef, intercept = np.empty((T, Z.shape[1])), np.empty(T)
    for t in range(T):
        lr = LogisticRegression(C=C, solver="newton-cholesky", tol=1e-12, max_iter=1000)
        lr.fit(Z, (labels == t).astype(int), sample_weight=s)
        coef[t], intercept[t] = lr.coef_[0], lr.intercept_[0]
    return coef, intercept


@functools.lru_cache(maxsize=None)
def reference_model(n, G, T, seed, balance, C=1.0):
    """The sklearn pipeline on a recipe: features (the expressed genes), scaler, coefficients, the bound's Hessian data."""
    r = recipe(n, G, T, seed)
    keep = np.flatnonzero(np.diff(r["X"].tocsc().indptr) > 0)
    X = r["X"][:, keep]
    mean, scale = scaler(X)
    Z = dense_z(X, mean, scale)
    s = weights_of(r["labels"], T, balance)
    coef, intercept = sklearn_fit(Z, r["labels"], s, T, C)
    return {"keep": keep, "X": X, "mean": mean, "scale": scale, "Z": Z, "s": s, "coef": coef, "intercept": intercept}


# ---- the training passes, for the host optimiser without a device ---------------------------------------------------------
class NumpyProblem:
    """sc_annot_train_* in plain numpy (no fixed order: the optimiser's contract is its stopping rule)."""

    def __init__(self, X, labels, weights, T):
        self.mean, self.scale = scaler(X)
        self.Z = dense_z(X, self.mean, self.scale)
        self.Y = (labels[:, None] == np.arange(T)[None, :]).astype(np.float64)
        self.s = np.asarray(weights, dtype=np.float64)
        self.S = self.Dir = None

    def annot_train_forward(self, coef, bias, direction=False):
        out = self.Z @ np.asarray(coef).T + np.asarray(bias)
        if direction:
            self.Dir = out
        else:
            self.S = out

    def annot_train_grad(self):
        R = self.s[:, None] * (expit(self.S) - self.Y)
        loss = (self.s[:, None] * (np.logaddexp(0.0, self.S) - self.Y * self.S)).sum(axis=0)
        return np.hstack([R.T @ self.Z, R.sum(axis=0)[:, None]]), loss

    def annot_train_line(self, alpha):
        p = expit(self.S + alpha * self.Dir)
        return ((self.s[:, None] * (p - self.Y)) * self.Dir).sum(axis=0), ((self.s[:, None] * p * (1 - p)) * self.Dir**2).sum(axis=0)

    def annot_train_step(self, alpha):
        self.S = self.S + alpha * self.Dir
