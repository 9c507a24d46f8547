"""sc_mixture_fit / sc_mixture_predict restated in numpy (spatialcore_amd/csrc/sc_mixture.hip), and the
input recipes of the mixture tests.

The restatement follows the device's structure: the M-step's two passes (the second around the NEW mean) over slices of
``mixture_slice_rows`` rows added in ascending slice order, Cholesky -> P = L^-T -> log det and b = mu^T P, the E-step as
||x P - b||^2, log-sum-exp as max + log sum exp, the log-likelihood from 256-row block sums added in the device's two levels, and sklearn's
loop and stop rule.  Inside a slice (and inside a dot product) numpy's own order stands in for the device's, so the
restatement agrees with the device to rounding, not bit for bit; the tests state the distances."""

import numpy as np
from scipy import linalg

from spatialcore_amd._lib import mixture_slice_rows

EPS10 = 10 * np.finfo(np.float64).eps


# ---- recipes ---------------------------------------------------------------------------------------------------------
def planted(n, D, K, sep, seed=0, correlated=0, weights=None, dtype=np.float64):
    """K centres N(0, sep^2); per component A_k = I + G / sqrt(D); rows mu_z + A_z eps, from ONE default_rng(seed).
    ``correlated`` > 0 appends that many columns 0.7 X[:, :correlated] + 0.3 noise (columns correlated like aggregated
    layers).  Returns (X, z)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, sep, size=(K, D))
    A = np.eye(D)[None] + rng.standard_normal((K, D, D)) / np.sqrt(D)
    z = rng.choice(K, size=n, p=weights) if weights is not None else rng.integers(0, K, size=n)
    eps = rng.standard_normal((n, D))
    X = centres[z] + np.einsum("nij,nj->ni", A[z], eps)
    if correlated:
        X = np.hstack([X, 0.7 * X[:, :correlated] + 0.3 * rng.standard_normal((n, correlated))])
    return np.ascontiguousarray(X.astype(dtype)), z


# ---- the device's steps ------------------------------------------------------------------------------------------------
def m_step(X, resp, reg_covar, covariance_type):
    n, D = X.shape
    K = resp.shape[1]
    S = mixture_slice_rows(n, D, K, covariance_type)
    nk = np.zeros(K)
    sums = np.zeros((K, D))
    for s0 in range(0, n, S):
        nk = nk + resp[s0:s0 + S].sum(axis=0)
        sums = sums + resp[s0:s0 + S].T @ X[s0:s0 + S]
    nk = nk + EPS10
    mu = sums / nk[:, None]
    tot = 0.0
    for k in range(K):
        tot = tot + nk[k]
    w = nk / tot
    if covariance_type == "full":
        cov = np.zeros((K, D, D))
        for k in range(K):
            for s0 in range(0, n, S):
                d = X[s0:s0 + S] - mu[k]
                cov[k] = cov[k] + (resp[s0:s0 + S, k, None] * d).T @ d
            cov[k] = cov[k] / nk[k]
            cov[k] = np.triu(cov[k]) + np.triu(cov[k], 1).T      # the upper triangle, mirrored
            cov[k][np.diag_indices(D)] += reg_covar
    else:
        cov = np.zeros((K, D))
        for k in range(K):
            for s0 in range(0, n, S):
                d = X[s0:s0 + S] - mu[k]
                cov[k] = cov[k] + (resp[s0:s0 + S, k, None] * (d * d)).sum(axis=0)
            cov[k] = cov[k] / nk[k] + reg_covar
    return w, mu, cov


class IllDefined(ValueError):
    pass


def precisions(mu, cov, covariance_type):
    """(P, log det, b): "full" P[k] = L^-T upper triangular, "diag" P[k] = 1 / sqrt(var)."""
    K, D = mu.shape
    if covariance_type == "diag":
        if not (np.isfinite(cov).all() and (cov > 0).all()):
            raise IllDefined("variance not > 0")
        P = 1.0 / np.sqrt(cov)
        return P, np.log(P).sum(axis=1), None
    P = np.empty((K, D, D))
    for k in range(K):
        try:
            L = linalg.cholesky(cov[k], lower=True)
        except linalg.LinAlgError as e:
            raise IllDefined(str(e))
        P[k] = linalg.solve_triangular(L, np.eye(D), lower=True).T
    logdet = np.array([np.log(np.diag(P[k])).sum() for k in range(K)])
    b = np.einsum("kd,kde->ke", mu, P)
    return P, logdet, b


def weighted_log_prob(X, w, mu, cov, covariance_type):
    n, D = X.shape
    K = w.size
    P, logdet, b = precisions(mu, cov, covariance_type)
    q = np.empty((n, K))
    for k in range(K):
        y = X @ P[k] - b[k] if covariance_type == "full" else (X - mu[k]) * P[k]
        q[:, k] = (y * y).sum(axis=1)
    return (-0.5 * (D * np.log(2 * np.pi) + q) + logdet[None, :]) + np.log(w)[None, :]


def e_step(X, w, mu, cov, covariance_type):
    """(responsibilities, labels, mean log-likelihood)."""
    lp = weighted_log_prob(X, w, mu, cov, covariance_type)
    m = lp.max(axis=1)
    e = np.exp(lp - m[:, None])
    s, comp = np.zeros(X.shape[0]), np.zeros(X.shape[0])
    for k in range(lp.shape[1]):                         # k ascending, Kahan's compensation
        y = e[:, k] - comp
        t = s + y
        comp = (t - s) - y
        s = t
    lse = m + np.log(s)
    blocks = [lse[b0:b0 + 256].sum() for b0 in range(0, X.shape[0], 256)]
    per = -(-len(blocks) // 256)                         # 256 runs of consecutive blocks, each ascending, then the runs ascending
    tot = 0.0
    for t in range(256):
        run = 0.0
        for v in blocks[t * per:(t + 1) * per]:
            run = run + v
        tot = tot + run
    return e / s[:, None], lp.argmax(axis=1).astype(np.int32), tot / X.shape[0]


def fit_from_labels(X, labels, K, covariance_type, max_iter, tol, reg_covar=1e-6):
    """One run from given start labels: dict of weights, means, covariances, lower_bound, n_iter, converged."""
    X = np.asarray(X, dtype=np.float64)
    resp = np.zeros((X.shape[0], K))
    resp[np.arange(X.shape[0]), labels] = 1.0
    w, mu, cov = m_step(X, resp, reg_covar, covariance_type)
    prev, lb, conv, it = -np.inf, -np.inf, False, 0
    for it in range(1, max_iter + 1):
        resp, _, lb = e_step(X, w, mu, cov, covariance_type)
        w, mu, cov = m_step(X, resp, reg_covar, covariance_type)
        precisions(mu, cov, covariance_type)    # raises where the device flags
        if abs(lb - prev) < tol:
            conv = True
            break
        prev = lb
    return {"weights": w, "means": mu, "covariances": cov, "lower_bound": lb, "n_iter": it, "converged": conv}


def kmeans_labels(X, K, n_init, seed):
    """The start labels of sklearn's GaussianMixture(init_params="kmeans", n_init, random_state=seed): KMeans(K, n_init=1) per
    run on ONE shared RandomState."""
    from sklearn.cluster import KMeans

    if K == 1:
        return [np.zeros(X.shape[0], dtype=np.int64) for _ in range(n_init)]
    rs = np.random.RandomState(seed)
    return [KMeans(K, n_init=1, random_state=rs).fit(X).labels_ for _ in range(n_init)]


def fit(X, K, covariance_type, n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0):
    """Every run and the best (a later run replaces it only on a strictly larger lower bound), with the labels and
    responsibilities of one more E-step under the best run's parameters."""
    X = np.asarray(X, dtype=np.float64)
    runs = [fit_from_labels(X, lab, K, covariance_type, max_iter, tol, reg_covar) for lab in kmeans_labels(X, K, n_init, seed)]
    best = 0
    for r in range(1, n_init):
        if runs[r]["lower_bound"] > runs[best]["lower_bound"]:
            best = r
    b = runs[best]
    resp, labels, loglik = e_step(X, b["weights"], b["means"], b["covariances"], covariance_type)
    return {"runs": runs, "best": best, "labels": labels, "proba": resp, "loglik": loglik}


def sklearn_fit(X, K, covariance_type, n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0):
    import warnings

    from sklearn.mixture import GaussianMixture

    gm = GaussianMixture(n_components=K, covariance_type=covariance_type, n_init=n_init, max_iter=max_iter, tol=tol,
                         reg_covar=reg_covar, init_params="kmeans", random_state=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        labels = gm.fit_predict(np.asarray(X, dtype=np.float64))
    return gm, labels


def distance(a, b):
    """The largest difference relative to the reference array's largest entry."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def parameter_distance(weights, means, covariances, gm):
    return max(distance(weights, gm.weights_), distance(means, gm.means_), distance(covariances, gm.covariances_))


def ambiguous_cells(gm, X, gap=1e-6):
    """Cells whose two largest weighted log-probabilities under sklearn's parameters are closer than ``gap``."""
    if gm.n_components == 1:
        return np.zeros(X.shape[0], dtype=bool)
    lp = gm._estimate_weighted_log_prob(np.asarray(X, dtype=np.float64))
    top = np.sort(lp, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) < gap


def three_domain_recipe(seed, n=3000, d=4):
    """Three domains of unequal size, split at x = 0.6 and 0.8; three cell types of which a domain holds one at 0.8 and the
    others at 0.1 each; an embedding whose type centres are 3 normal(3, d).  (xy, X, domain).  With equal thirds the
    stability rule prefers 4 (a labelling and its refinement score a high Fowlkes-Mallows index); with one large and two
    small domains K = 2 merges the small ones, s(2) rises and the rule returns the planted 3 (seeds 0 and 1, sklearn as the
    fitter, (2, 5), three runs: stabilities 0.80 / 0.86 / 0.83 / 0.76 at seed 1)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(size=(n, 2))
    domain = (xy[:, 0] > 0.6).astype(np.int64) + (xy[:, 0] > 0.8)
    u = rng.uniform(size=n)
    kind = np.where(u < 0.8, domain, np.where(u < 0.9, (domain + 1) % 3, (domain + 2) % 3))
    X = 3.0 * rng.normal(size=(3, d))[kind] + rng.normal(size=(n, d))
    return xy, X, domain
