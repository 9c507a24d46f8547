"""Inputs that drive the kernels of sc_threshold.hip to the edges of their own constants (plain numpy, no GPU).

  metagene   TH_FMAX = 64 features; np_row_sum has no accumulator loop below 16 features, one pass from 16, several from
             24, and a tail whenever F is no multiple of 8; row_select breaks ties by index; a workgroup owns 2048 rows
  KS         ordered_bits has one branch per sign; the background count m = max(int(n q), 10) ends k_th_sum inside a
             workgroup (2047), at its end (2048) or one point into the next (2049); at most 64 order statistics
  GMM        GMM_KMAX = 8 components = 33 partials per (run, workgroup); 1 .. 1024 runs that stop at different iterations

Every input comes from a fixed seed.  tests/test_cpu_threshold_edges.py proves, against numpy, scipy and sklearn alone,
that each input is what tests/test_gpu_threshold_edges.py says it is; the restated fits are computed once per process and
handed out read-only."""
import functools

import numpy as np

import threshold_restated as tr
from spatialcore_amd.spatial.neighborhoods import kmeans_draws

N_PERTURB = 4
FEATURE_COUNTS = (7, 8, 9, 15, 16, 17, 24, 33, 63, 64)
EXACT_METHODS = ("arithmetic_mean", "median", "minimum")
REG_COVAR = 1e-6


# ---- metagene ----------------------------------------------------------------------------------------------------------
def edge_features(n, F, dtype, seed):
    """Log-normal markers with dropout zeros.  Rows i % 4 == 1 are rounded to one decimal (exact ties: row_select decides
    by index); rows i % 16 == 2 hold -0.0 in their first and +0.0 in their last column; row n // 3 has a NaN and row n - 1
    a +Inf, as ``features`` of tests/test_gpu_threshold.py."""
    rng = np.random.default_rng(seed)
    M = rng.lognormal(0.0, 1.0, (n, F)) * (rng.random((n, F)) > 0.25)
    ties = np.arange(n) % 4 == 1
    M[ties] = np.round(M[ties], 1)
    zeros = np.arange(n) % 16 == 2
    M[zeros, 0] = -0.0
    M[zeros, F - 1] = 0.0
    M[n // 3, F - 1] = np.nan
    M[n - 1, 0] = np.inf
    return M.astype(dtype)


def negative_features(n, F, dtype, seed):
    """edge_features with one row in three moved down by its own shift in [0.2, 4): those rows hold negative values, and
    some of them a negative median and mean.  The two rows that are not valid hold a negative value too (not counted)."""
    M = edge_features(n, F, np.float64, seed)
    rng = np.random.default_rng(seed + 1000)
    rows = rng.random(n) < 1.0 / 3.0
    M[rows] -= rng.uniform(0.2, 4.0, (int(rows.sum()), 1))
    M[n // 3, 0] = -1.0
    M[n - 1, F - 1] = -2.0
    return M.astype(dtype)


def invalid_block_features(dtype, F=3, seed=77):
    """n = 4097: rows 2048 .. 4095 (the whole second workgroup) are not valid -- NaN, +Inf and -Inf by turns, in turning
    columns; row 4096, the third workgroup's only row, is valid."""
    M = edge_features(4097, F, np.float64, seed)
    bad = np.arange(2048, 4096)
    M[bad, bad % F] = np.array([np.nan, np.inf, -np.inf])[bad % 3]
    M[4096, 0] = 1.5                    # (edge_features put its +Inf here)
    return M.astype(dtype)


def all_invalid_features(dtype, n=300, F=3, seed=78):
    M = edge_features(n, F, np.float64, seed)
    rows = np.arange(n)
    M[rows, rows % F] = np.array([np.nan, np.inf, -np.inf])[rows % 3]
    return M.astype(dtype)


def stats_of_scores(score, valid):
    """min, max, mean that k_metagene owes to a score vector: exact functions of the scores it wrote (block order)."""
    nv = int(valid.sum())
    sv = np.asarray(score)[valid].astype(np.float64)
    full = np.where(valid, np.asarray(score).astype(np.float64), 0.0)
    return (float(sv.min()) if nv else np.inf, float(sv.max()) if nv else -np.inf,
            float(tr.block_sum(full)) / nv if nv else np.nan)


# ---- KS ----------------------------------------------------------------------------------------------------------------
def ks_key_scores(dtype, extremes=True, seed=31):
    """About 3000 scores in ``dtype`` that take both branches of ordered_bits: normals of both signs, -0.0 and +0.0,
    subnormals of both signs, runs of equal values, neighbours that differ by a few fp64 ulps (in float32 they collapse
    into runs of equal keys) and, with ``extremes``, the largest finite values of both signs.  Shuffled."""
    rng = np.random.default_rng(seed)
    fi = np.finfo(dtype)
    base = rng.normal(0.0, 1.0, 40).astype(np.float32).astype(np.float64)
    close = (base[:, None] * (1.0 + np.arange(5)[None, :] * 2.0 ** -50)).reshape(-1)     # float32: 40 runs of 5
    sub = float(fi.smallest_subnormal) * rng.integers(1, 1000, 60)
    parts = [rng.normal(-0.5, 1.5, 1500), rng.lognormal(0.0, 1.0, 500), np.round(rng.normal(0.0, 1.0, 600), 1), close,
             np.full(20, -0.0), np.full(20, 0.0), sub, -sub]
    if extremes:
        parts.append(np.array([float(fi.max), -float(fi.max)]))
    x = np.concatenate(parts)
    return rng.permutation(x).astype(dtype)


def background_count(n, q):
    """sc_ks_prepare's m."""
    return min(max(int(n * q), 10), n)


BACKGROUND_CASES = ((4094, 0.5, 2047), (4096, 0.5, 2048), (4098, 0.5, 2049), (10, 0.5, 10), (12, 0.99, 11))


def background_scores(n, dtype, seed=41):
    return np.random.default_rng(seed + n).normal(-0.3, 1.2, n).astype(dtype)


def rank_requests(n, seed=43):
    """64 ranks: both ends, one rank twice, the rest at random (with repeats)."""
    r = np.random.default_rng(seed).integers(0, n, 64)
    r[:4] = [0, n - 1, n // 2, n // 2]
    return r.astype(np.int64)


def classify_scores(n, dtype, seed=47):
    """Scores on a grid of 0.1 around zero, and a threshold that many of them equal exactly."""
    x = np.round(np.random.default_rng(seed + n).normal(0.0, 1.0, n), 1).astype(dtype)
    return x, float(dtype(-0.3))


def ks_gap(x, q):
    """(gap between the two largest D at distinct scores, the tolerance of D) -- the golden generator's rule."""
    thr, dev, lab, p = tr.ks(x, q)
    D = tr.ks_deviation(p["sorted"], p["background_mean"], p["background_std"])
    others = D[p["sorted"] != p["sorted"][p["argmax"]]]
    tol = 16 * spread(lambda: [np.array(tr.ks(x, q)[3]["D"])], [np.array(p["D"])])[0] + 2.0 ** -52
    return float(D.max() - others.max()), tol, p


def spread(fn, base):
    """Largest deviation of fn() from base (lists of arrays) over N_PERTURB one-ulp perturbations of exp / log / erf /
    erfc in the restatement."""
    worst = [0.0] * len(base)
    for t in range(N_PERTURB):
        with tr.perturbed(np.random.default_rng(500 + t)):
            got = fn()
        for i, (a, b) in enumerate(zip(got, base)):
            worst[i] = max(worst[i], float(np.max(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float)))))
    return worst


# ---- GMM ---------------------------------------------------------------------------------------------------------------
def mixture(n, K, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, K, n)
    return rng.normal(0.9 * c, 0.35 + 0.05 * c)


def zero_inflated(n, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.55, 0.0, rng.gamma(3.0, 0.7, n))


# name: (scores, K, n_init, seed of the draws, max_iter, type)
GMM_CASES = {
    "k8_mixed_stop_f64": (lambda: mixture(600, 8, 4), 8, 10, 4, 6, np.float64),
    "k8_mixed_stop_f32": (lambda: mixture(600, 8, 4), 8, 10, 4, 6, np.float32),
    "k8_block_2048": (lambda: mixture(2048, 8, 11), 8, 10, 11, 100, np.float64),
    "k8_block_2049": (lambda: mixture(2049, 8, 12), 8, 10, 12, 100, np.float64),
    "k8_three_groups": (lambda: mixture(4097, 8, 5), 8, 3, 5, 100, np.float64),
    "k5_one_run": (lambda: mixture(300, 5, 6), 5, 1, 6, 100, np.float64),
    "k4_many_runs": (lambda: mixture(777, 4, 13), 4, 33, 13, 100, np.float64),
    "zero_inflated_k3": (lambda: zero_inflated(3000, 9), 3, 10, 9, 100, np.float64),
    "zero_inflated_k8_f32": (lambda: zero_inflated(3000, 9), 8, 10, 9, 100, np.float32),
    # the fit classify_by_threshold(median, gmm, n_components=4, seed=42) makes on public_gmm_matrix()
    "public_k4": (lambda: tr.metagene(public_gmm_matrix(), "median")["score"], 4, 10, 42, 100, np.float64),
}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def gmm_case(name):
    """scores (in the case's type), K, n_init, draws, max_iter and the restated fit of the case; read-only."""
    make, K, n_init, seed, max_iter, dtype = GMM_CASES[name]
    x = make().astype(dtype)
    draws = kmeans_draws(seed, n_init, K)
    want = tr.gmm_fit(x, K, draws, max_iter=max_iter)
    return _frozen({"x": x, "K": K, "n_init": n_init, "draws": draws, "max_iter": max_iter, "want": _frozen(want)})


def change_margin(want, tol=1e-3):
    return min(abs(abs(c) - tol) for t in want["changes"] for c in t if np.isfinite(c))


def sklearn_kmeans_labels(x, K, n_init, seed):
    """labels_ of the n_init KMeans fits GaussianMixture(n_init, random_state=seed) starts from: one shared RandomState."""
    from sklearn.cluster import KMeans

    rs = np.random.RandomState(seed)
    X = np.asarray(x).reshape(-1, 1)
    return np.array([KMeans(K, n_init=1, random_state=rs).fit(X).labels_ for _ in range(n_init)])


def equal_label_groups(km_labels):
    """Lists of runs whose k-means labels are identical, cell for cell (two runs or more)."""
    groups = {}
    for r, lab in enumerate(km_labels):
        groups.setdefault(lab.tobytes(), []).append(r)
    return [g for g in groups.values() if len(g) > 1]


# ---- posteriors --------------------------------------------------------------------------------------------------------
def k8_posterior_setup():
    """The best run of k8_block_2048, the seven components above the lowest mean in argsort order, the case's scores."""
    c = gmm_case("k8_block_2048")
    f = c["want"]
    b = f["best"]
    w, mu, var = f["weights"][b], f["means"][b], f["variances"][b]
    return c["x"], w, mu, var, [int(k) for k in np.argsort(mu)[1:]]


FAR_SDS = 400.0
EXP_UNDERFLOW = 745.14      # exp(-x) is exactly 0 in fp64 from here on


def far_scores(mu, var):
    """Scores FAR_SDS of the widest component's standard deviations below the lowest and above the highest mean, and a
    few steps on.  (At 40 standard deviations the neighbouring component's responsibility is about 1e-80, not 0: with
    unequal variances the exponents part only quadratically.  From here on one component's weighted log-probability
    exceeds every other's by more than EXP_UNDERFLOW, with room for the last places of exp and log.)"""
    sd = float(np.sqrt(np.max(var)))
    steps = np.array([1.0, 1.5, 2.0, 3.0])
    return np.concatenate([np.min(mu) - FAR_SDS * sd * steps, np.max(mu) + FAR_SDS * sd * steps])


def responsibilities(x, w, mu, var):
    """(n, K): gmm_posterior with one high component at a time."""
    return np.stack([tr.gmm_posterior(x, w, mu, var, [k], 0.5)[0] for k in range(len(w))], axis=1)


# ---- the public function -------------------------------------------------------------------------------------------------
def public_ks_matrix(n=600, F=17, seed=61):
    """17 float32 markers with negative values: a high group of cells above a background around zero."""
    rng = np.random.default_rng(seed)
    hi = rng.random(n) < 0.3
    return (rng.normal(0.0, 0.4, (n, F)) + np.where(hi, 2.5, 0.0)[:, None]).astype(np.float32)


def public_gmm_matrix(n=600, F=33, seed=62):
    """33 float64 markers around four levels."""
    rng = np.random.default_rng(seed)
    level = rng.integers(0, 4, n)
    return np.abs(rng.normal(1.2 * level[:, None], 0.3, (n, F)))
