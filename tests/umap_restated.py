"""numpy restatement of sc_fuzzy_graph and sc_umap_layout in the device's documented orders (sc_umap.hip, DESIGN.md 4.6r;
the definitions are in include/spatialcore_hip.h) and the input recipes of their tests.

Everything here gives the bits the kernels must give except where ``exp``, ``pow`` and the divisions by a value that came
out of them enter: ``rho``, the union's pattern, the firing schedule, the negative samples, the skips and the branches are
exact; ``sigma``, the weights and the positions agree to a few units in the last place."""
import math

import numpy as np

import diffusion_restated as R
import neighbors_restated as N
import oracle as orc

ITERS = 64                    # UM_ITERS
A_DEFAULT, B_DEFAULT = 0.58303, 1.33417     # scanpy's published defaults (min_dist = 0.5, spread = 1)
np_power = np.power           # the one pow of an interaction (``conditioning`` perturbs it)


# ---- fuzzy simplicial set -----------------------------------------------------------------------------------------------
def smooth_knn(d2):
    """(rho, sigma, info) of the lists' squared distances (n, k): umap's bisection and floor.  ``info`` = {``iterations``
    (evaluations of psum per row), ``converged``, ``floored``, ``row_sums``, ``global_mean``, ``target``}."""
    d = np.sqrt(np.asarray(d2, dtype=np.float64))
    n, k = d.shape
    pos = d > 0
    rho = np.where(pos.any(axis=1), np.min(np.where(pos, d, np.inf), axis=1), 0.0)
    S = np.zeros(n)
    for j in range(k):
        S = S + d[:, j]
    target = math.log2(float(k + 1))
    t = d - rho[:, None]
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    active = np.ones(n, dtype=bool)
    converged = np.zeros(n, dtype=bool)
    iterations = np.zeros(n, dtype=np.int64)
    with np.errstate(over="ignore", under="ignore"):
        for _ in range(ITERS):
            rows = np.flatnonzero(active)
            if rows.size == 0:
                break
            tt, m = t[rows], mid[rows]
            psum = np.zeros(rows.size)
            for j in range(k):
                psum = psum + np.where(tt[:, j] > 0, np.exp(-(tt[:, j] / m)), 1.0)
            iterations[rows] += 1
            done = np.abs(psum - target) < 1e-5
            converged[rows[done]] = True
            active[rows[done]] = False
            r, ps = rows[~done], psum[~done]
            up = r[ps > target]
            hi[up] = mid[up]
            mid[up] = (lo[up] + hi[up]) / 2.0
            dn = r[~(ps > target)]
            lo[dn] = mid[dn]
            grow = dn[np.isinf(hi[dn])]
            half = dn[~np.isinf(hi[dn])]
            mid[grow] = mid[grow] * 2.0
            mid[half] = (lo[half] + hi[half]) / 2.0
    global_mean = R.dots(S[None, :], np.ones(n))[0] / float(n * (k + 1))
    mean = np.where(rho > 0, S / float(k + 1), global_mean)
    floor = 1e-3 * mean
    sigma = np.where(mid < floor, floor, mid)
    return rho, sigma, {"iterations": iterations, "converged": converged, "floored": mid < floor, "row_sums": S,
                        "global_mean": global_mean, "target": target}


def memberships(d2, rho, sigma):
    """p (n, k) of the list entries: 1 where d - rho <= 0, else exp(-((d - rho) / sigma))."""
    t = np.sqrt(np.asarray(d2, dtype=np.float64)) - rho[:, None]
    with np.errstate(over="ignore", under="ignore"):
        return np.where(t > 0, np.exp(-(t / sigma[:, None])), 1.0)


def fuzzy_graph(idx, d2):
    """The whole of sc_fuzzy_graph on lists (idx, d2): {rho, sigma, p, indptr, indices, w, info}."""
    n, k = idx.shape
    rho, sigma, info = smooth_knn(d2)
    p = memberships(d2, rho, sigma)
    indptr, indices = R.union_edges(idx)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    keys = (np.repeat(np.arange(n, dtype=np.int64), k) * n + idx.ravel().astype(np.int64))
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], p.ravel()[order]

    def directed(i, j):
        want = i * n + j
        at = np.minimum(np.searchsorted(keys, want), keys.size - 1)
        return np.where(keys[at] == want, vals[at], 0.0)

    pij = directed(rows, indices.astype(np.int64))
    pji = directed(indices.astype(np.int64), rows)
    w = (pij + pji) - pij * pji
    return {"rho": rho, "sigma": sigma, "p": p, "indptr": indptr, "indices": indices, "w": w, "info": info}


# ---- layout ---------------------------------------------------------------------------------------------------------------
def firing(w, e, w_max=None):
    """Which stored entries fire in epoch e.  ``w_max`` replaces the exact maximum (a recipe's host check asks what a
    wrong one would change)."""
    r = np.asarray(w, dtype=np.float64) / (np.max(w) if w_max is None else w_max)
    return np.floor(float(e + 1) * r) > np.floor(float(e) * r)


def firing_float32(w, e):
    """``firing`` with the epoch index converted through float32, which is exact only up to 2^24: what a kernel that
    converted e to float would compute."""
    r = np.asarray(w, dtype=np.float64) / np.max(w)
    return np.floor(float(np.float32(e + 1)) * r) > np.floor(float(np.float32(e)) * r)


def negatives(t, e, q, n, seed):
    """Sample q of the stored entries t (global CSR positions) in epoch e."""
    t = np.asarray(t, dtype=np.uint64)
    ctr = np.stack([t & np.uint64(0xFFFFFFFF), t >> np.uint64(32), np.full(t.size, e, dtype=np.uint64),
                    np.full(t.size, q >> 2, dtype=np.uint64)], axis=1).astype(np.uint32)
    o = orc.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1, 4)
    return ((o[:, q & 3].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _step(cur, y, attract, a, b, gamma, alpha, stats):
    dlt = cur - y
    d2 = dlt[:, 0] * dlt[:, 0]
    for c in range(1, cur.shape[1]):
        d2 = d2 + dlt[:, c] * dlt[:, c]
    m = d2 > 0
    stats["coincident"] += int((~m).sum())
    dd = d2[m]
    pb = np_power(dd, b)
    den = a * pb + 1.0
    coef = (((-2.0 * a) * b) * (pb / dd)) / den if attract else ((2.0 * gamma) * b) / ((0.001 + dd) * den)
    g = coef[:, None] * dlt[m]
    stats["clipped"] += int((np.abs(g) > 4.0).sum())
    g = np.clip(g, -4.0, 4.0)
    out = cur.copy()
    out[m] = cur[m] + alpha * g
    return out


def epoch(indptr, indices, w, Y_old, e, n_epochs, a, b, gamma, alpha0, neg, seed, stats, w_max=None):
    """Y_new of epoch e: every vertex walks its firing entries in stored order, reading Y_old only.  Vectorised over the
    vertices: pass p handles the p-th firing entry of every row that has one."""
    n = Y_old.shape[0]
    alpha = alpha0 * (1.0 - e / n_epochs)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    ft = np.flatnonzero(firing(w, e, w_max))
    fi = rows[ft]
    count = np.bincount(fi, minlength=n)
    rank = np.arange(ft.size) - (np.cumsum(count) - count)[fi]
    cur = np.array(Y_old, dtype=np.float64, copy=True)
    stats["firings"] += int(ft.size)
    for p in range(int(rank.max()) + 1 if ft.size else 0):
        sel = ft[rank == p]
        i, j = rows[sel], indices[sel].astype(np.int64)
        cur[i] = _step(cur[i], Y_old[j], True, a, b, gamma, alpha, stats)
        for q in range(neg):
            s = negatives(sel, e, q, n, seed)
            ok = s != i
            stats["skipped"] += int((~ok).sum())
            cur[i[ok]] = _step(cur[i[ok]], Y_old[s[ok]], False, a, b, gamma, alpha, stats)
    return cur


def new_stats():
    return {"firings": 0, "clipped": 0, "skipped": 0, "coincident": 0}


def layout(indptr, indices, w, Y, n_epochs, e0=0, e1=None, a=A_DEFAULT, b=B_DEFAULT, gamma=1.0, alpha0=1.0, neg=5, seed=0,
           stats=None, w_max=None):
    """Epochs [e0, e1) of sc_umap_layout from the positions Y."""
    stats = new_stats() if stats is None else stats
    Y = np.array(Y, dtype=np.float64, copy=True)
    for e in range(e0, n_epochs if e1 is None else e1):
        Y = epoch(indptr, indices, w, Y, e, n_epochs, a, b, gamma, alpha0, neg, seed, stats, w_max)
    return Y


def never_fires(w, n_epochs):
    """Stored entries that fire in no epoch of the schedule."""
    fired = np.zeros(np.size(w), dtype=bool)
    for e in range(n_epochs):
        fired |= firing(w, e)
    return ~fired


# ---- recipes --------------------------------------------------------------------------------------------------------------
FUZZY_SHAPES = [(3, 2, 2), (17, 3, 16), (129, 8, 15), (257, 50, 32), (1000, 20, 15)]


def features(n, d):
    """The features of the neighbour tests: the branching trajectory with seed 7 n + d."""
    return R.traj(n, d, 7 * n + d)[0]


def fuzzy_recipes():
    """name -> (features, k) of every fuzzy-graph case: the five shapes, the (129, 8, 15) shape scaled by 1e3 (mid doubles
    while hi is inf) and by 1e-3, two copies of every cell (one zero distance, rho is the second entry), six copies (five
    memberships of 1 exceed log2(16) = 4: the bisection runs all 64 times and the row takes the floor), forty copies (every
    distance zero: rho = 0, the global mean, every p = 1)."""
    out = {f"traj-n{n}-d{d}-k{k}": (features(n, d), k) for n, d, k in FUZZY_SHAPES}
    out["scaled-1e3"] = (features(129, 8) * 1e3, 15)
    out["scaled-1e-3"] = (features(129, 8) * 1e-3, 15)
    out["copies-2"] = (np.tile(N.pca_like(75, 8, 3), (2, 1)), 15)
    out["copies-6"] = (np.tile(N.pca_like(30, 8, 4), (6, 1)), 15)
    out["copies-40"] = (N.duplicates(100, 40, 50, 0), 15)
    return out


def star(n=300):
    """A centre in every row beside rows of degree 2 (the centre and one partner) and one of degree 1; the weights run
    from 0.05 (below w_max / 10: never fires in 10 epochs) to 1."""
    rows, cols, vals = [], [], []

    def edge(i, j, v):
        rows.extend((i, j))
        cols.extend((j, i))
        vals.extend((v, v))

    for i in range(1, n):
        edge(0, i, 0.05 + 0.95 * ((i * 37) % 100) / 99.0)
    for i in range(1, n - 2, 2):
        edge(i, i + 1, 0.05 + 0.95 * ((i * 11) % 50) / 49.0)
    from scipy import sparse

    A = sparse.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)


def start(n, C, seed):
    return np.random.default_rng(seed).uniform(-10.0, 10.0, size=(n, C))


def layout_graph(n, d, k):
    """(indptr, indices, w) of the restated fuzzy graph of features(n, d)."""
    g = fuzzy_graph(*R.knn(features(n, d), k))
    return g["indptr"], g["indices"], g["w"]


def layout_recipes():
    """name -> (graph, start positions, neg): n = 3 with k = 2 (a negative equals i in a third of the draws), the n = 17
    and n = 257 fuzzy graphs in 2 and 3 dimensions, the star, neg = 0, and a start in which two adjacent vertices coincide
    (the d2 = 0 branch).

    The starts are uniform draws whose seeds were taken in order, with one exception made on the host: from seed 7 the star's
    hub passes a leaf at d2 ~ 1e-3, where a repulsion has the gain 2 gamma b / 0.001 ~ 2.7e3 per interaction, and the
    restatement ITSELF moves by 2e-10 of the extent when its pow is changed by one unit in the last place
    (``conditioning``); a difference to the device from that start would measure the recipe, not the kernel.  From seed 8
    it moves by 2e-15, as every other recipe here does (tests/test_cpu_umap.py asserts 1e-12 for all of them)."""
    g3, g17, g257, st = layout_graph(3, 2, 2), layout_graph(17, 3, 5), layout_graph(257, 8, 15), star(300)
    twin = start(257, 2, 5)
    first = g257[0][:-1]                                 # a vertex whose first stored entry has the largest weight, so that it
    v = int(np.flatnonzero(g257[2][first] == g257[2].max())[0])   # fires in every epoch before the vertex has moved
    twin[int(g257[1][first[v]])] = twin[v]               # ... and that neighbour start at one point
    return {
        "n3-C2": (g3, start(3, 2, 1), 5),
        "n17-C2": (g17, start(17, 2, 2), 5),
        "n17-C3": (g17, start(17, 3, 3), 5),
        "n257-C2": (g257, start(257, 2, 4), 5),
        "n257-C3": (g257, start(257, 3, 6), 5),
        "n257-C2-neg0": (g257, start(257, 2, 4), 0),
        "n257-C2-coincident": (g257, twin, 5),
        "star-C2": (st, start(300, 2, 8), 5),
    }


def conditioning(graph, Y0, neg, reps=4, seed=0, extent=10.0, run=None):
    """The largest movement (of the extent 10) of three restated epochs when every pow result is changed by -1, 0 or +1
    unit in the last place at random: what the reference itself cannot tell apart.  ``run`` replaces the arguments of
    ``layout`` (an edge case's own epochs, seed, a, b, gamma and neg) and ``extent`` the start's extent."""
    global np_power
    rng = np.random.default_rng(seed)
    run = dict(n_epochs=10, e0=0, e1=3, neg=neg, seed=11) if run is None else run
    ref = layout(*graph, Y0, **run)
    exact, worst = np_power, 0.0
    try:
        np_power = lambda x, b: exact(x, b) * (1.0 + rng.integers(-1, 2, size=np.shape(x)) * 2.0 ** -52)   # noqa: E731
        for _ in range(reps):
            worst = max(worst, float(np.abs(layout(*graph, Y0, **run) - ref).max()) / extent)
    finally:
        np_power = exact
    return worst


# ---- recipes at the kernels' constants --------------------------------------------------------------------------------
MIXED_CASES = [(1023, 16), (1024, 8), (1024, 9), (1025, 17), (2049, 16)]    # (n, k) around SUM_CHUNK = 1024 rows
WIDTH_KS = [2, 8, 9, 17, 31]        # sc_knn_dense admits k >= 2; 8 | 9 and 16 | 17 are the edges of k_um_sigma<8/16/32>
WMAX_GRID = 2048 * 256              # threads of k_um_wmax's largest grid: stored entries from here on are strided
HIGH_SEED = (5 << 32) | 11          # the seed of the other tests with a non-zero high word (Philox key word k1)
LATE_EPOCHS, LATE_E0 = 2 ** 31 - 1, 1_000_000_000      # epoch indices a float32 cannot tell apart (exact up to 2^24)


def mixed(n, k):
    """pca_like(n - k - 1, 8, 5) and k + 1 further copies of its row 0: the k + 2 identical cells list zero distances only
    (rho = 0, so their floor is 1e-3 of the global mean, which the other rows make non-zero).  The few cells whose nearest
    cell is row 0 list k of the copies at one distance d > 0 (rho = d, every t = 0, psum = k: the row-mean floor); every
    other row is ordinary and converges.  Returns (features, the indices of the identical cells)."""
    X = N.pca_like(n - k - 1, 8, 5)
    return np.concatenate([X, np.tile(X[0], (k + 1, 1))]), np.concatenate([[0], np.arange(n - k - 1, n)])


def plain_mean(row_sums, k):
    """The mean of all distances with the row sums added in row order, a running sum from 0: NOT the device's order."""
    s = 0.0
    for v in row_sums.tolist():
        s = s + v
    return s / float(row_sums.size * (k + 1))


def fuzzy_edge_recipes():
    """name -> (features, k): ``mixed`` at one chunk of row sums less one, one chunk, one chunk and one, two chunks and one,
    with list widths on both sides of the k_um_sigma instantiations; the (129, 8) trajectory at those widths, the widest
    but one and the smallest the search admits."""
    out = {f"mixed-n{n}-k{k}": (mixed(n, k)[0], k) for n, k in MIXED_CASES}
    out.update({f"width-k{k}": (features(129, 8), k) for k in WIDTH_KS})
    return out


def ring(n=20000, reach=14):
    """A ring lattice, every vertex joined to ``reach`` neighbours on either side: w{lo, hi} = 0.05 + 0.5 ((31 lo + 17 hi)
    % 97) / 96 <= 0.55, and the edge {n - 2, n - 1} set to 1.0.  With n = 20,000 its two stored positions are 559,971 and
    559,999 of 560,000: the maximum lies in the part of w that k_um_wmax reaches only by striding.  Returns (graph, the two
    positions)."""
    i = np.repeat(np.arange(n, dtype=np.int64), 2 * reach)
    off = np.tile(np.concatenate([np.arange(-reach, 0), np.arange(1, reach + 1)]), n)
    j = (i + off) % n
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    w = 0.05 + 0.5 * ((31 * lo + 17 * hi) % 97).astype(np.float64) / 96
    top = np.flatnonzero((lo == n - 2) & (hi == n - 1))
    w[top] = 1.0
    indptr = np.arange(n + 1, dtype=np.int64) * (2 * reach)
    return (indptr, j.astype(np.int32), w), top


def star_with_empty_rows():
    """The star with a vertex without stored entries put in front (every index moves up by one) and one appended."""
    indptr, indices, w = star(300)
    return np.concatenate([[0], indptr, indptr[-1:]]).astype(np.int64), (indices + 1).astype(np.int32), w


def _case(graph, Y0, neg=5, seed=11, n_epochs=10, e0=0, e1=3, a=A_DEFAULT, b=B_DEFAULT, gamma=1.0, extent=10.0):
    return {"graph": graph, "Y0": Y0, "extent": extent,
            "run": dict(n_epochs=n_epochs, e0=e0, e1=e1, a=a, b=b, gamma=gamma, neg=neg, seed=seed)}


def layout_edge_recipes():
    """name -> {graph, Y0, extent, run (the arguments of ``layout``)}: the n = 257 graph with the negatives ending inside
    and exactly at every block of four (k_um_epoch draws four per Philox call) up to UM_NEG_MAX = 16, a seed with a high
    word, the ring whose largest weight lies past k_um_wmax's grid, rows without entries, gamma = 0 and its neg = 0 twin,
    another a and b, and three epochs of a 2^31 - 1 epoch schedule from the 10^9-th.

    The starts are the ones of ``layout_recipes`` (seed 4 in two dimensions, 8 for the star) and seed 9 for the ring,
    with two exceptions made on the host as for the star there.  With a = 1.5, b = 0.9 the restatement itself moves by
    1.1e-12 of the extent from seed 4 under a one-ulp change of its pow (``conditioning``), above the 1e-12 that
    tests/test_cpu_umap.py asserts for every case; from seed 5, the next, it moves by 1.3e-14.  In three dimensions no
    step of neg = 4 is clipped from seed 6, the start of ``n257-C3``; from seed 7, the next, one is, for both neg."""
    g257 = layout_graph(257, 8, 15)
    y2, y3 = start(257, 2, 4), start(257, 3, 7)
    out = {f"neg{q}-C2": _case(g257, y2, neg=q) for q in (1, 3, 4, 8, 9, 16)}
    out.update({f"neg{q}-C3": _case(g257, y3, neg=q) for q in (4, 16)})
    out["seed-high-word"] = _case(g257, y2, seed=HIGH_SEED)
    out["ring-wmax-tail"] = _case(ring()[0], np.random.default_rng(9).uniform(-100.0, 100.0, size=(20000, 2)), n_epochs=4, e1=2,
                                  extent=100.0)
    out["star-empty-rows"] = _case(star_with_empty_rows(), start(302, 2, 8))
    out["gamma0"] = _case(g257, y2, gamma=0.0)
    out["gamma0-neg0"] = _case(g257, y2, gamma=0.0, neg=0)
    out["a1.5-b0.9"] = _case(g257, start(257, 2, 5), a=1.5, b=0.9)
    out["late-epochs"] = _case(g257, y2, n_epochs=LATE_EPOCHS, e0=LATE_E0, e1=LATE_E0 + 3)
    return out


def layout_case_epochs(case, stats=None, w_max=None):
    """[(e1, restated positions after the epochs [e0, e1))] of an edge case, one epoch at a time."""
    run, ref, out = case["run"], case["Y0"], []
    for e1 in range(run["e0"] + 1, run["e1"] + 1):
        ref = layout(*case["graph"], ref, **{**run, "e0": e1 - 1, "e1": e1}, stats=stats, w_max=w_max)
        out.append((e1, ref))
    return out


def blobs(n=1500, seed=0):
    """The quality recipe: ten blobs at 8 e_c in 10 dimensions, unit noise.  Returns (X, labels)."""
    rng = np.random.default_rng(seed)
    labels = np.arange(n) % 10
    X = rng.standard_normal((n, 10))
    X[np.arange(n), labels] += 8.0
    return X, labels


def pca2(X, extent=10.0):
    """The first two principal components scaled to max |.| = extent."""
    Z = X - X.mean(axis=0)
    _, _, Vt = np.linalg.svd(Z, full_matrices=False)
    Y = Z @ Vt[:2].T
    return Y * (extent / np.abs(Y).max())


def one_nn_accuracy(Y, labels):
    from sklearn.neighbors import NearestNeighbors

    nb = NearestNeighbors(n_neighbors=2).fit(Y).kneighbors(Y, return_distance=False)[:, 1]
    return float(np.mean(labels[nb] == labels))
