"""numpy restatement of sc_kmeans_fit (spatialcore_amd/csrc/sc_kmeans.hip): sklearn 1.7.2's KMeans(init="k-means++")
with the kernels' arithmetic choices -- fp64 distances summed feature by feature, D^2 stored in the input type, the
potentials and the searched prefix sum in the kernels' one summation order (chunks of 64 points, 64 chunks per group,
each level sequential), fp64 Lloyd sums, the first index on ties, relocation ties to the lowest point index.

Test helper only: not used by the package."""

import numpy as np

CH = 64
GRP = CH * CH


def first_index(u0, n, dtype):
    """numpy's RandomState.choice(n, p=w / w.sum()) for unit weights of the input type, given its random_sample()."""
    w = np.ones(n, dtype=dtype)
    p = (w / w.sum()).astype(np.float64)
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    return min(int(cdf.searchsorted(u0, side="right")), n - 1)


def _levels(D):
    """The kernels' summation levels of one D^2 vector (fp64, zero-padded to whole groups)."""
    n = D.size
    G = -(-n // GRP)
    Dp = np.zeros(G * GRP, dtype=np.float64)
    Dp[:n] = D
    P0 = np.cumsum(Dp.reshape(G, CH, CH), axis=2)    # within a chunk
    P1 = np.cumsum(P0[:, :, -1], axis=1)             # chunk sums within a group
    P2 = np.cumsum(P1[:, -1])                        # group sums
    return Dp, P0, P1, P2


def hsum(D):
    return _levels(np.asarray(D, dtype=np.float64))[3][-1]


def search(D, v):
    """Index of the draw v in the prefix sums of D (the kernels' level-by-level searchsorted, side='left')."""
    n = D.size
    Dp, P0, P1, P2 = _levels(np.asarray(D, dtype=np.float64))
    g = int(np.searchsorted(P2, v, side="left"))
    if g == P2.size:
        return n - 1
    base2 = P2[g - 1] if g > 0 else 0.0
    j = min(int(np.searchsorted(base2 + P1[g], v, side="left")), CH - 1)
    base1 = base2 + P1[g, j - 1] if j > 0 else base2
    chunk = Dp[(g * CH + j) * CH:(g * CH + j + 1) * CH]
    e = min(int(np.searchsorted(base1 + np.cumsum(chunk), v, side="left")), CH - 1)
    return min((g * CH + j) * CH + e, n - 1)


def _seq_dot(A, b):
    acc = np.zeros(A.shape[0], dtype=np.float64)
    for c in range(A.shape[1]):
        acc = acc + A[:, c] * b[c]
    return acc


def _d2(X64, xn, q, dtype):
    d = (-2.0 * _seq_dot(X64, X64[q]) + xn[q]) + xn
    d = d.astype(dtype)
    return np.maximum(d, dtype(0))


def seeding(Xc, K, draws):
    """k-means++ of one run: draws = [random_sample, uniform(size=L) per later centre]; returns the K indices."""
    n = Xc.shape[0]
    dtype = Xc.dtype.type
    X64 = Xc.astype(np.float64)
    xn = _seq_dot(X64 * X64, np.ones(X64.shape[1]))   # sequential |x|^2
    L = 2 + int(np.log(K))
    idx = [first_index(draws[0], n, Xc.dtype)]
    D = _d2(X64, xn, idx[0], dtype)
    for c in range(1, K):
        pot = float(dtype(hsum(D)))
        cands = [search(D, u * pot) for u in draws[1 + (c - 1) * L:1 + c * L]]
        mins = [np.minimum(D, _d2(X64, xn, q, dtype)) for q in cands]
        pots = [dtype(hsum(m)) for m in mins]
        b = int(np.argmin(pots))
        idx.append(cands[b])
        D = mins[b]
    return np.array(idx, dtype=np.int64)


def _dist_all(X64, cent64):
    d = np.empty((X64.shape[0], cent64.shape[0]), dtype=np.float64)
    for k in range(cent64.shape[0]):
        acc = np.zeros(X64.shape[0])
        for c in range(X64.shape[1]):
            t = X64[:, c] - cent64[k, c]
            acc = acc + t * t
        d[:, k] = acc
    return d


def lloyd(Xc, centers, max_iter, tol):
    """sklearn's _kmeans_single_lloyd with fp64 arithmetic; returns labels, inertia, centres, n_iter, strict."""
    dtype = Xc.dtype.type
    n, C = Xc.shape
    K = centers.shape[0]
    X64 = Xc.astype(np.float64)
    cent = centers.astype(dtype).copy()
    labels = np.full(n, -1, dtype=np.int64)
    strict = False
    it = 0
    for it in range(max_iter):
        new = np.argmin(_dist_all(X64, cent.astype(np.float64)), axis=1)
        changed = int(np.count_nonzero(new != labels))
        labels = new
        counts = np.bincount(labels, minlength=K).astype(np.int64)
        sums = np.zeros((K, C))
        np.add.at(sums, labels, X64)
        empties = np.flatnonzero(counts == 0)
        if empties.size:
            old = cent.astype(np.float64)
            dist = ((X64 - old[labels]) ** 2).sum(axis=1)
            far = np.lexsort((np.arange(n), -dist))[:empties.size]
            for nk, f in zip(empties, far):
                ok = labels[f]
                sums[ok] -= X64[f]
                sums[nk] = X64[f]
                counts[nk] = 1
                counts[ok] -= 1
        newc = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], sums).astype(dtype)
        shift = float(((newc.astype(np.float64) - cent.astype(np.float64)) ** 2).sum())
        cent = newc
        if changed == 0:
            strict = True
            break
        if shift <= tol:
            break
    if not strict:
        labels = np.argmin(_dist_all(X64, cent.astype(np.float64)), axis=1)
    inertia = float(((X64 - cent.astype(np.float64)[labels]) ** 2).sum())
    return labels, inertia, cent, it + 1, strict


def is_same_clustering(a, b, K):
    mapping = np.full(K, -1)
    for i in range(a.size):
        if mapping[a[i]] == -1:
            mapping[a[i]] = b[i]
        elif mapping[a[i]] != b[i]:
            return False
    return True


def fit(X, K, n_init, max_iter, draws, seeding_only=False):
    """KMeans.fit: tol and centring in the input type, every run, the best-run rule, best_centers += X_mean."""
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    tol = np.mean(np.var(X, axis=0)) * 1e-4
    x_mean = X.mean(axis=0)
    Xc = X - x_mean
    seeds = np.stack([seeding(Xc, K, draws[r]) for r in range(n_init)])
    if seeding_only:
        return {"seeds": seeds}
    best = None
    for r in range(n_init):
        labels, inertia, cent, n_iter, strict = lloyd(Xc, Xc[seeds[r]], max_iter, float(tol))
        if best is None or (inertia < best["inertia"] and not is_same_clustering(labels, best["labels"], K)):
            best = {"labels": labels, "inertia": inertia, "centers": cent, "n_iter": n_iter, "strict": strict}
    best["centers"] = best["centers"] + x_mean
    best["seeds"] = seeds
    best["distinct"] = int(np.unique(best["labels"]).size)
    return best
