"""numpy restatement of sc_kmeans_fit (spatialcore_amd/csrc/sc_kmeans.hip): sklearn 1.7.2's KMeans(init="k-means++")
with the kernels' arithmetic choices -- fp64 distances summed feature by feature, D^2 stored in the input type, the
potentials and the searched prefix sum in the kernels' one summation order (chunks of 64 points, 64 chunks per group,
each level sequential), fp64 Lloyd sums, the first index on ties, relocation ties to the lowest point index.

Two modes of the Lloyd part.  The default sums in point order (np.add.at, numpy's pairwise .sum()): the algorithm, in
an order of its own.  With ``nb`` (lloyd) / ``kernel_order=True`` (fit) every floating-point sum is taken in the
kernels' own order, so the result equals sc_kmeans_fit's bit for bit (the library is built with -ffp-contract=off and
every operation is an IEEE add, multiply, divide or conversion):
 - sums: workgroup b of NB owns the tiles (256 points) b, b + NB, ...; per (cluster, feature) it adds its points in
   index order; then the workgroups are added in order;
 - inertia: thread tid of workgroup b adds the points tid of its tiles in order; then threads 0..255 in order, then
   the workgroups in order;
 - shift: thread tid adds the entries tid, tid + 256, ... of the flat K x C array in order; then the threads in order;
 - relocation distances: feature by feature.
NB = workgroups(n, C, K, R) depends on the number of runs R in the call, as in kmeans_fit.

Test helper only: not used by the package."""

import numpy as np

CH = 64
GRP = CH * CH
TPB = 256


def workgroups(n, C, K, R):
    """NB of kmeans_fit: Lloyd workgroups per run (every one has a tile; the partial sums stay below 256 MiB)."""
    tiles = -(-n // TPB)
    return max(1, min(tiles, 256, (1 << 25) // max(1, R * K * C)))


def _seq(a, axis=0):
    """Sum along an axis one element after the other (accumulate is sequential by definition; .sum() is pairwise)."""
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


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


def flat_prefix(D):
    """The prefix sum the kernels search a draw in, per point: (P2[g-1] + P1[g][j-1]) + P0[g][j][e], fp64."""
    n = D.size
    _, P0, P1, P2 = _levels(np.asarray(D, dtype=np.float64))
    G = P2.size
    base2 = np.concatenate(([0.0], P2[:-1]))
    base1 = np.concatenate((base2[:, None], base2[:, None] + P1[:, :-1]), axis=1)
    return (base1[:, :, None] + P0).ravel()[:n]


def tie_draws(D, pot):
    """(i, u): the points i whose draw u = prefix[i] / pot gives u * pot == prefix[i] exactly in fp64 (0 < u < 1), so
    that the search for u decides between ">=" and ">" at point i."""
    pre = flat_prefix(D)
    u = pre / pot
    i = np.flatnonzero((u * pot == pre) & (u > 0.0) & (u < 1.0))
    return i, u[i]


def draws_for_seeds(Xc, seeds):
    """One run's uniforms that make k-means++ on the centred Xc pick exactly ``seeds``: the first draw is
    (q + 0.5) / n; all L draws of a later round are the midpoint of the target's D^2 interval divided by pot."""
    n = Xc.shape[0]
    dtype = Xc.dtype.type
    K = len(seeds)
    L = 2 + int(np.log(K))
    X64 = Xc.astype(np.float64)
    xn = _seq_dot(X64 * X64, np.ones(X64.shape[1]))
    out = np.empty(1 + (K - 1) * L, dtype=np.float64)
    out[0] = (seeds[0] + 0.5) / n
    if first_index(out[0], n, Xc.dtype) != seeds[0]:
        raise ValueError(f"no first draw for point {seeds[0]}")
    D = _d2(X64, xn, seeds[0], dtype)
    for c in range(1, K):
        t = int(seeds[c])
        pot = float(dtype(hsum(D)))
        pre = flat_prefix(D)
        u = 0.5 * ((pre[t - 1] if t > 0 else 0.0) + pre[t]) / pot
        if not (D[t] > 0 and 0.0 <= u < 1.0 and search(D, u * pot) == t):
            raise ValueError(f"point {t} cannot be drawn as centre {c}")
        out[1 + (c - 1) * L:1 + c * L] = u
        D = np.minimum(D, _d2(X64, xn, t, dtype))
    return out


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


def _wg_sums(X64, labels, K, nb):
    """Per workgroup and (cluster, feature): its points in index order; then the workgroups in order."""
    n, C = X64.shape
    wg = (np.arange(n) // TPB) % nb
    part = np.zeros((nb * K, C))
    np.add.at(part, wg * K + labels, X64)          # unbuffered: one point after the other, in index order
    return _seq(part.reshape(nb, K, C), axis=0)


def _wg_inertia(dmin, nb):
    """Thread tid of workgroup b: its tiles in order; then the threads in order; then the workgroups in order."""
    tiles = -(-dmin.size // TPB)
    per = -(-tiles // nb)
    d = np.zeros(per * nb * TPB)
    d[:dmin.size] = dmin
    return float(_seq(_seq(_seq(d.reshape(per, nb, TPB), axis=0), axis=1)))


def _thread_shift(newc, cent):
    """Thread tid: the entries tid, tid + 256, ... of the flat K x C array in order; then the threads in order."""
    d = (newc.astype(np.float64) - cent.astype(np.float64)).ravel()
    sq = np.zeros(-(-d.size // TPB) * TPB)
    sq[:d.size] = d * d
    return float(_seq(_seq(sq.reshape(-1, TPB), axis=0)))


def lloyd(Xc, centers, max_iter, tol, nb=None, trace=None):
    """sklearn's _kmeans_single_lloyd with fp64 arithmetic; returns labels, inertia, centres, n_iter, strict.
    nb: sum in the kernels' orders for nb workgroups (module docstring); None: in point order.
    trace: a list that receives one dict per relocation (iteration, the empty clusters, the points they took, the
    clusters those came from, and whether the choice or its order rested on equal distances)."""
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
        if nb is None:
            sums = np.zeros((K, C))
            np.add.at(sums, labels, X64)
        else:
            sums = _wg_sums(X64, labels, K, nb)
        empties = np.flatnonzero(counts == 0)
        if empties.size:
            old = cent.astype(np.float64)
            if nb is None:
                dist = ((X64 - old[labels]) ** 2).sum(axis=1)
            else:
                dist = np.zeros(n)
                for c in range(C):
                    t = X64[:, c] - old[labels, c]
                    dist = dist + t * t
            far = np.lexsort((np.arange(n), -dist))[:empties.size]
            if trace is not None:
                trace.append({"iteration": it, "empties": empties.tolist(), "points": far.tolist(),
                              "donors": labels[far].tolist(), "distances": dist[far].tolist(),
                              "tied": bool(np.count_nonzero(dist >= dist[far[-1]]) > far.size
                                           or np.unique(dist[far]).size < far.size)})
            for nk, f in zip(empties, far):
                ok = labels[f]
                sums[ok] -= X64[f]
                sums[nk] = X64[f]
                counts[nk] = 1
                counts[ok] -= 1
        newc = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], sums).astype(dtype)
        if nb is None:
            shift = float(((newc.astype(np.float64) - cent.astype(np.float64)) ** 2).sum())
        else:
            shift = _thread_shift(newc, cent)
        cent = newc
        if changed == 0:
            strict = True
            break
        if shift <= tol:
            break
    if not strict or nb is not None:
        d = _dist_all(X64, cent.astype(np.float64))
    if not strict:
        labels = np.argmin(d, axis=1)
    if nb is None:
        inertia = float(((X64 - cent.astype(np.float64)[labels]) ** 2).sum())
    else:
        inertia = _wg_inertia(d[np.arange(n), labels], nb)
    return labels, inertia, cent, it + 1, strict


def is_same_clustering(a, b, K):
    mapping = np.full(K, -1)
    for i in range(a.size):
        if mapping[a[i]] == -1:
            mapping[a[i]] = b[i]
        elif mapping[a[i]] != b[i]:
            return False
    return True


def fit(X, K, n_init, max_iter, draws, seeding_only=False, kernel_order=False):
    """KMeans.fit: tol and centring in the input type, every run, the best-run rule, best_centers += X_mean.
    kernel_order: the Lloyd sums in sc_kmeans_fit's orders for a call with these n_init runs (module docstring).
    Beside the best run's result: every run's inertia, the best run's index, for every later run the decision
    (inertia lower than the best so far, same partition as the best so far) and every run's relocations."""
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    tol = np.mean(np.var(X, axis=0)) * 1e-4
    x_mean = X.mean(axis=0)
    Xc = X - x_mean
    seeds = np.stack([seeding(Xc, K, draws[r]) for r in range(n_init)])
    if seeding_only:
        return {"seeds": seeds}
    nb = workgroups(X.shape[0], X.shape[1], K, n_init) if kernel_order else None
    best = None
    inertias, decisions, relocations = [], [], []
    for r in range(n_init):
        trace = []
        labels, inertia, cent, n_iter, strict = lloyd(Xc, Xc[seeds[r]], max_iter, float(tol), nb, trace)
        inertias.append(inertia)
        relocations.append(trace)
        if best is not None:
            decisions.append((inertia < best["inertia"], is_same_clustering(labels, best["labels"], K)))
        if best is None or (decisions[-1][0] and not decisions[-1][1]):
            best = {"labels": labels, "inertia": inertia, "centers": cent, "n_iter": n_iter, "strict": strict,
                    "best_run": r}
    best["centers"] = best["centers"] + x_mean
    best["seeds"] = seeds
    best["distinct"] = int(np.unique(best["labels"]).size)
    best["inertias"] = inertias
    best["decisions"] = decisions
    best["relocations"] = relocations
    return best
