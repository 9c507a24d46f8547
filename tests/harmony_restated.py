"""Harmony (Korsunsky et al. 2019) as sc_harmony.hip computes it, restated in numpy, the textbook forms it is
checked against, and the inputs of the tests.

Restated: the algorithm with the device's on-purpose choices (strided blocks, one table per block and no subtraction, the
row-minimum shift).  Bit-equality with the device is claimed only where the arithmetic is correctly rounded and the order is
restated exactly: the unit rows (unit_rows: the sum of squares in feature order, sqrt, division), the block membership and the
(block, batch, cell) sort (device_order).  Everything else (matrix products, exp, log, pow, the sums over cells) is numpy's
own order and agrees with the device within the tolerances that scripts/harmony_probe.py --tolerances measures.

Textbook, independent of the closed form and of the per-block tables: correct_dense (Phi_moe = [1; one-hot], np.linalg.solve
of Phi_Rk Phi_moe^T + diag(0, lamb, ..)) and update_subtract (harmonypy's subtract-and-re-add block update on running O and
E, over the same strided blocks)."""
import math

import numpy as np


def n_blocks(n, block_size):
    return min(int(math.ceil(1.0 / block_size)), int(n))


def device_order(n, nb, batch):
    """The cell at every position of the device's sort: by block (cell mod nb), then batch, then cell index."""
    cells = np.arange(n, dtype=np.int64)
    return np.lexsort((cells, np.asarray(batch), cells % nb)).astype(np.int64)


def unit_rows(Z):
    """Rows scaled to unit L2 norm: q = 0.0 + z_0 z_0 + z_1 z_1 + .. in feature order, z / sqrt(q)."""
    Z = np.asarray(Z, dtype=np.float64)
    q = np.zeros(Z.shape[0])
    for j in range(Z.shape[1]):
        q = q + Z[:, j] * Z[:, j]
    return Z / np.sqrt(q)[:, None]


def soft_assign(Zc, Y, sigma, shift=True):
    """dist = 2 (1 - Zc Y^T) and S = exp(-(dist - rowmin) / sigma) (shift=False: harmonypy's exp(-dist / sigma))."""
    dist = 2.0 * (1.0 - Zc @ Y.T)
    m = dist.min(axis=1, keepdims=True) if shift else 0.0
    return dist, np.exp(-(dist - m) / sigma)


def xlogx(R):
    out = np.zeros_like(R)
    pos = R > 0
    out[pos] = R[pos] * np.log(R[pos])
    return out


class Harmony:
    """The state the device keeps, with the same four steps: the constructor is sc_harmony_begin."""

    def __init__(self, Z, batch, n_batches, Y, nb, sigma, theta, lamb):
        self.Z = np.asarray(Z, dtype=np.float64)
        self.batch = np.asarray(batch)
        self.n, self.d = self.Z.shape
        self.B, self.K, self.nb = int(n_batches), Y.shape[0], int(nb)
        self.sigma, self.theta, self.lamb = float(sigma), float(theta), float(lamb)
        self.Phi = np.eye(self.B)[self.batch]                      # n x B one-hot
        self.Pr = np.bincount(self.batch, minlength=self.B) / self.n
        self.blocks = [np.arange(t, self.n, self.nb) for t in range(self.nb)]
        self.Zc = unit_rows(self.Z)
        self.Zcorr = self.Z.copy()
        self.Y = unit_rows(Y)
        self.W = np.zeros((self.K, self.B, self.d))
        self.dist, self.S = soft_assign(self.Zc, self.Y, self.sigma)
        self.R = self.S / self.S.sum(axis=1, keepdims=True)
        self.O = np.stack([self.R[idx].T @ self.Phi[idx] for idx in self.blocks])   # blocks x K x B
        self.objective = self._objective()

    def _tables(self, skip=None):
        O = np.zeros((self.K, self.B))
        for t in range(self.nb):
            if t != skip:
                O = O + self.O[t]
        return O, O.sum(axis=1, keepdims=True) * self.Pr[None, :]

    def _objective(self):
        O, E = self._tables()
        ratio = np.log((O + 1.0) / (E + 1.0))
        return float(np.sum(self.R * self.dist) + self.sigma * np.sum(xlogx(self.R))
                     + self.sigma * self.theta * np.sum(self.R * ratio[:, self.batch].T))

    def round(self):
        V = self.R.T @ self.Zc
        mass = np.sqrt((V * V).sum(axis=1)) > 0
        self.Y[mass] = unit_rows(V[mass])                          # a cluster without mass keeps its centre
        self.dist, self.S = soft_assign(self.Zc, self.Y, self.sigma)
        for t, idx in enumerate(self.blocks):
            Om, Em = self._tables(skip=t)
            pen = ((Em + 1.0) / (Om + 1.0)) ** self.theta
            u = self.S[idx] * pen[:, self.batch[idx]].T
            self.R[idx] = u / u.sum(axis=1, keepdims=True)
            self.O[t] = self.R[idx].T @ self.Phi[idx]
        self.objective = self._objective()
        return self.objective

    def cluster(self, max_iter, epsilon):
        obj = []
        for r in range(max_iter):
            obj.append(self.round())
            if epsilon >= 0 and r > 3:
                old, new = obj[r - 1] + obj[r - 2] + obj[r - 3], obj[r] + obj[r - 1] + obj[r - 2]
                if abs(old - new) / abs(old) < epsilon:
                    break
        return np.array(obj)

    def correct(self):
        self.W, self.Zcorr = correct_closed(self.Z, self.R, self._tables()[0], self.batch, self.B, self.lamb)
        self.Zc = unit_rows(self.Zcorr)

    def get(self, name):
        return {"Zcorr": self.Zcorr, "Zc": self.Zc, "R": self.R, "Y": self.Y, "O": self.O, "W": self.W, "dist": self.dist,
                "order": device_order(self.n, self.nb, self.batch)}[name]


def correct_closed(Z, R, O, batch, B, lamb):
    """The arrowhead system [[s, o^T], [o, diag(o + lamb)]] per cluster in closed form: (W (K, B, d), Zcorr)."""
    K, d = R.shape[1], Z.shape[1]
    Phi = np.eye(B)[batch]
    W = np.zeros((K, B, d))
    for k in range(K):
        o = O[k]
        rb = (Phi * R[:, k:k + 1]).T @ Z                           # B x d
        s, r0 = o.sum(), rb.sum(axis=0)
        den = s - np.sum(o * o / (o + lamb))
        w0 = (r0 - np.sum((o / (o + lamb))[:, None] * rb, axis=0)) / den if den > 0 else np.zeros(d)
        W[k] = (rb - o[:, None] * w0[None, :]) / (o + lamb)[:, None]
    return W, Z - np.einsum("ik,ikd->id", R, W[:, batch, :].transpose(1, 0, 2))


def correct_dense(Z, R, batch, B, lamb):
    """harmonypy's moe_correct_ridge, dense: per cluster solve (Phi_Rk Phi_moe^T + diag(0, lamb, ..)) W = Phi_Rk Z, drop the
    intercept row, subtract.  Returns (W without the intercept (K, B, d), Zcorr)."""
    n, d = Z.shape
    K = R.shape[1]
    Phi_moe = np.vstack([np.ones(n), np.eye(B)[batch].T])          # (B + 1) x n
    ridge = np.diag(np.r_[0.0, np.full(B, lamb)])
    Zcorr = Z.copy()
    W = np.zeros((K, B, d))
    for k in range(K):
        Phi_Rk = Phi_moe * R[:, k][None, :]
        Wk = np.linalg.solve(Phi_Rk @ Phi_moe.T + ridge, Phi_Rk @ Z)
        Wk[0] = 0.0
        Zcorr = Zcorr - (Wk.T @ Phi_Rk).T
        W[k] = Wk[1:]
    return W, Zcorr


def update_subtract(S, R, batch, B, nb, theta):
    """harmonypy's update_R on running tables: per block subtract its mass from O and E, reassign, add it back."""
    n = R.shape[0]
    R = R.copy()
    Phi = np.eye(B)[batch]
    Pr = np.bincount(batch, minlength=B) / n
    O = R.T @ Phi
    E = np.outer(R.sum(axis=0), Pr)
    for t in range(nb):
        idx = np.arange(t, n, nb)
        O = O - R[idx].T @ Phi[idx]
        E = E - np.outer(R[idx].sum(axis=0), Pr)
        u = S[idx] * (((E + 1.0) / (O + 1.0)) ** theta)[:, batch[idx]].T
        R[idx] = u / u.sum(axis=1, keepdims=True)
        O = O + R[idx].T @ Phi[idx]
        E = E + np.outer(R[idx].sum(axis=0), Pr)
    return R, O


# ---- the steps every comparison walks through ------------------------------------------------------------------------------------
ARRAYS = ("R", "Y", "O", "W", "Zcorr")
CHECKPOINTS = ("begin", "round1", "round5", "correct1", "outer3")


def walk(engine, begin):
    """{checkpoint: {array: copy, "objective": value}}: after begin, after 1 and 5 clustering rounds, after the correction, and
    after 3 outer rounds of 5.  ``begin()`` starts the engine and returns the starting objective; the engine has
    cluster(max_iter, epsilon) -> objectives, correct() and get(name).  The epsilons are negative: the full count."""
    out = {}

    def snap(name, objective):
        out[name] = {a: np.array(engine.get(a), dtype=np.float64) for a in ARRAYS}
        out[name]["objective"] = float(objective)

    last = begin()
    snap("begin", last)
    last = engine.cluster(1, -1.0)[-1]
    snap("round1", last)
    last = engine.cluster(4, -1.0)[-1]
    snap("round5", last)
    engine.correct()
    snap("correct1", last)
    for _ in range(2):
        last = engine.cluster(5, -1.0)[-1]
        engine.correct()
    snap("outer3", last)
    return out


def relative_differences(got, want):
    """{(checkpoint, array): max |got - want| / max |want|}"""
    out = {}
    for cp in CHECKPOINTS:
        for a in ARRAYS + ("objective",):
            g, w = np.asarray(got[cp][a]), np.asarray(want[cp][a])
            scale = np.max(np.abs(w))
            out[(cp, a)] = float(np.max(np.abs(g - w)) / scale) if scale > 0 else float(np.max(np.abs(g)))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def mixture(sizes, d, n_types, seed, shift=1.5, spread=3.0, noise=0.5, sort=False):
    """Cells of ``n_types`` Gaussian types (centres ~ N(0, spread^2)) in batches of the given sizes, every batch moved by
    its own vector (~ N(0, shift^2)).  The cells are interleaved (a random order) unless ``sort``: then batch by batch.
    Returns (Z float64 (n, d), batch codes int32, type codes)."""
    rng = np.random.default_rng(seed)
    n, B = int(sum(sizes)), len(sizes)
    batch = np.repeat(np.arange(B), sizes)
    types = rng.integers(0, n_types, size=n)
    Z = spread * rng.normal(size=(n_types, d))[types] + shift * rng.normal(size=(B, d))[batch] + noise * rng.normal(size=(n, d))
    if not sort:
        p = rng.permutation(n)
        Z, batch, types = Z[p], batch[p], types[p]
    return np.ascontiguousarray(Z), batch.astype(np.int32), types


def spread_start(Z, K):
    """K starting centres: the unit rows of K cells spread over the input."""
    n = Z.shape[0]
    return unit_rows(Z)[(np.arange(K) * n) // K].copy()


# (name, batch sizes, d, types, K, block_size, sigma, theta, lamb, dtype, sorted by batch); what each is there for:
CASES = [
    ("n17", (9, 8), 3, 2, 2, 0.05, 0.1, 2.0, 1.0, np.float64, False),          # fewer cells than blocks: 17 blocks of 1; B = 2, K = 2, d = 3
    ("n20", (12, 8), 3, 2, 2, 0.05, 0.1, 2.0, 1.0, np.float64, False),         # one cell per block
    ("n21", (12, 9), 3, 2, 3, 0.05, 0.1, 2.0, 1.0, np.float64, False),         # unequal blocks: one of 2 cells
    ("n1201", (700, 400, 101), 10, 4, 17, 0.05, 0.1, 2.0, 1.0, np.float64, False),   # unequal blocks, 700 / 400 / ~100, K = 17 (no multiple of 4 or 16)
    ("slice", (129, 128), 5, 3, 4, 1.0, 0.1, 2.0, 1.0, np.float64, False),     # one block; a segment of 129 = a slice of 128 + 1; n = 257 = two tiles of 128 + 1
    ("d1", (30, 30), 1, 2, 2, 0.25, 2.0, 2.0, 1.0, np.float64, False),         # d = 1: unit rows are +-1 (sigma = 2 keeps the assignment soft)
    ("d64-k128", (150, 150), 64, 5, 128, 0.05, 0.1, 2.0, 1.0, np.float64, False),   # the largest d and K
    ("b64", (3,) * 64, 8, 3, 5, 0.05, 0.1, 2.0, 1.0, np.float64, False),       # the largest B: most (block, batch) segments are empty
    ("pair", (300, 98, 2), 6, 3, 7, 0.05, 0.1, 2.0, 1.0, np.float64, False),   # a batch of exactly 2 cells
    ("theta0", (150, 150), 6, 3, 6, 0.05, 0.1, 0.0, 1.0, np.float64, False),   # no penalty; the correction still runs
    ("sigma1e-3", (150, 150), 6, 3, 6, 0.05, 1e-3, 2.0, 1.0, np.float64, False),   # harmonypy's exp(-dist / sigma) underflows here
    ("f32", (150, 150), 6, 3, 6, 0.05, 0.1, 2.0, 0.5, np.float32, False),      # float32 input
    ("sorted", (200, 200, 200), 6, 3, 8, 0.05, 0.1, 2.0, 1.0, np.float64, True),    # cells batch by batch ...
    ("interleaved", (200, 200, 200), 6, 3, 8, 0.05, 0.1, 2.0, 1.0, np.float64, False),   # ... and the same recipe interleaved
]


def case_inputs(case):
    """(Z in the case's dtype, batch, B, Y, nb, sigma, theta, lamb) of one of CASES."""
    name, sizes, d, n_types, K, block_size, sigma, theta, lamb, dtype, sort = case
    seed = 100 + [c[0] for c in CASES].index(name if name != "interleaved" else "sorted")
    Z, batch, _ = mixture(sizes, d, n_types, seed, sort=True)
    if not sort:                                   # "interleaved" permutes exactly the cells of "sorted"
        p = np.random.default_rng(7).permutation(Z.shape[0])
        Z, batch = np.ascontiguousarray(Z[p]), batch[p]
    Z = Z.astype(dtype)
    return Z, batch, len(sizes), spread_start(Z, K), n_blocks(Z.shape[0], block_size), sigma, theta, lamb


def restated_walk(case):
    Z, batch, B, Y, nb, sigma, theta, lamb = case_inputs(case)
    box = {}

    class Engine:
        cluster = staticmethod(lambda m, e: box["h"].cluster(m, e))
        correct = staticmethod(lambda: box["h"].correct())
        get = staticmethod(lambda a: box["h"].get(a))

    def begin():
        box["h"] = Harmony(Z, batch, B, Y, nb, sigma, theta, lamb)
        return box["h"].objective

    return walk(Engine, begin)


def device_walk(ctx, case):
    """walk() on the device: ``ctx`` is a spatialcore_amd._lib.Context.  Leaves no problem resident."""
    Z, batch, B, Y, nb, sigma, theta, lamb = case_inputs(case)

    class Engine:
        cluster = staticmethod(ctx.harmony_cluster)
        correct = staticmethod(ctx.harmony_correct)
        get = staticmethod(ctx.harmony_get)

    try:
        return walk(Engine, lambda: ctx.harmony_begin(Z, batch, B, Y, nb, sigma, theta, lamb))
    finally:
        ctx.harmony_end()


# ---- quality: the neighbours' batches and types ------------------------------------------------------------------------------------
def neighbour_shares(X, batch, types, k=15):
    """(share of the k exact nearest neighbours in the cell's own batch, share of its own type), averaged over the cells."""
    X = np.asarray(X, dtype=np.float64)
    sq = (X * X).sum(axis=1)
    D = sq[:, None] + sq[None, :] - 2.0 * (X @ X.T)
    np.fill_diagonal(D, np.inf)
    nn = np.argpartition(D, k, axis=1)[:, :k]
    return float(np.mean(batch[nn] == batch[:, None])), float(np.mean(types[nn] == types[:, None]))


# (name, batch sizes, nclust): 10-D, 4 types, the batch shift of `mixture`; the restatement reaches chance within 0.05 at
# these nclust (tests/test_cpu_harmony.py asserts it)
RECIPES = [("three", (400, 400, 400), 10), ("uneven", (700, 400, 100), 10)]

# name: (same-batch share before, after, chance = sum Pr_b^2, same-type share after, outer rounds, converged) over the 15
# exact nearest neighbours; the restatement with nclust = 10 and harmony_integrate's defaults
RECIPE_FIGURES = {
    "three": (1.0, 0.33205555555555555, 1.0 / 3.0, 1.0, 3, True),
    "uneven": (1.0, 0.4662777777777778, 0.45833333333333337, 1.0, 4, True),
}


def recipe(name):
    sizes = dict((r[0], r[1]) for r in RECIPES)[name]
    return mixture(sizes, 10, 4, 11 if name == "three" else 12)


def restated_integrate(Z, batch, B, Y, *, theta=2.0, lamb=1.0, sigma=0.1, max_iter_harmony=10, max_iter_kmeans=20,
                       epsilon_cluster=1e-5, epsilon_harmony=1e-4, block_size=0.05):
    """harmony_integrate's loop on the restatement: (Zcorr, objectives per outer round, converged)."""
    h = Harmony(Z, batch, B, Y, n_blocks(Z.shape[0], block_size), sigma, theta, lamb)
    objectives, converged = [], False
    for _ in range(max_iter_harmony):
        objectives.append(h.cluster(max_iter_kmeans, epsilon_cluster))
        h.correct()
        if len(objectives) > 1 and abs(objectives[-2][-1] - objectives[-1][-1]) / abs(objectives[-2][-1]) < epsilon_harmony:
            converged = True
            break
    return h.Zcorr, objectives, converged
