"""numpy restatement of spatialcore_amd/csrc/sc_threshold.hip: metagene scores, the KS cutoff and the one-dimensional
Gaussian mixture of classify_by_threshold, with the kernels' arithmetic choices.

Summation order ("block order"): workgroup b owns the 2048 consecutive points from 2048 b; its thread t adds the points
2048 b + 256 j + t, j = 0 .. 7, in that order; the 256 thread values are added as the fixed tree value[t] += value[t + h],
h = 128 .. 1; the workgroups are added in index order.  The library is built with -ffp-contract=off and every operation
outside exp / log / erf / erfc is an IEEE add, multiply, divide, square root or conversion, so everything that does not
pass through one of those four functions equals the device bit for bit.

 - metagene: the mean over the features is numpy's pairwise row sum (``row_sum``); arithmetic_mean, median and minimum
   compute in the input type; the two geometric means in fp64, rounded to the input type once.
 - KS: fp64; background mean and population standard deviation in two passes, block order; Phi as scipy's ndtr.
 - GMM: the k-means labels of every run come from tests/kmeans_restated.py (seeding + lloyd in the kernels' order);
   the EM is sklearn 1.7.2's in fp64 with block-order sums and a ONE-pass variance around the current mean c:
   sum r (x - m)^2 = B - 2 (m - c) A + (m - c)^2 S0, A = sum r (x - c), B = sum r (x - c)^2.  sklearn takes a second
   pass around the new mean m; the initialisation here does too.

``perturbed(rng)`` moves every exp / log / erf / erfc result by -1, 0 or +1 ulp at random: the model of a math library
that differs from numpy's in the last place, from which the device tolerances are measured.

Test helper only: not used by the package."""

import contextlib

import numpy as np
from scipy import special

import kmeans_restated as kr

TPB, PT = 256, 8
BLK = TPB * PT
LOG_2PI = float(np.log(2 * np.pi))
EPS10 = 10 * np.finfo(np.float64).eps
METHODS = ("shifted_geometric_mean", "geometric_mean", "arithmetic_mean", "median", "minimum")

_RNG = None


@contextlib.contextmanager
def perturbed(rng):
    global _RNG
    _RNG = rng
    try:
        yield
    finally:
        _RNG = None


def _lib(fn, x):
    y = np.asarray(fn(x), dtype=np.float64)
    if _RNG is None:
        return y
    step = _RNG.integers(-1, 2, size=y.shape)
    return np.where(step == 0, y, np.nextafter(y, np.where(step > 0, np.inf, -np.inf)))


def _exp(x): return _lib(np.exp, x)
def _log(x): return _lib(np.log, x)


def ndtr(a):
    """scipy's ndtr: 0.5 + 0.5 erf(x) for |x| < 1, else 0.5 erfc(|x|) mirrored; x = a / sqrt 2."""
    x = np.asarray(a, dtype=np.float64) * 0.70710678118654752440
    z = np.abs(x)
    y = 0.5 * _lib(special.erfc, z)
    return np.where(z < 1.0, 0.5 + 0.5 * _lib(special.erf, x), np.where(x > 0.0, 1.0 - y, y))


def block_sum(v):
    """Sum over axis 0 in block order."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[0]
    nb = max(1, -(-n // BLK))
    pad = np.zeros((nb * BLK,) + v.shape[1:])
    pad[:n] = v
    a = kr._seq(pad.reshape((nb, PT, TPB) + v.shape[1:]), axis=1)
    h = TPB // 2
    while h >= 1:
        a = a[:, :h] + a[:, h:2 * h]
        h //= 2
    return kr._seq(a[:, 0], axis=0)


def row_sum(A):
    """numpy's pairwise sum of every (contiguous) row of A, fewer than 128 columns, in A's type."""
    n, f = A.shape
    if f < 8:
        res = np.zeros(n, dtype=A.dtype)
        for i in range(f):
            res = res + A[:, i]
        return res
    r = [A[:, i].copy() for i in range(8)]
    i = 8
    while i < f - f % 8:
        for k in range(8):
            r[k] = r[k] + A[:, i + k]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(i, f):
        res = res + A[:, k]
    return res


def metagene(features, method, pseudocount=0.1):
    """sc_metagene_score: valid, score (input type, NaN where not valid), min / max / mean, the three counts."""
    F = np.ascontiguousarray(features)
    T = F.dtype.type
    n, f = F.shape
    valid = np.all(np.isfinite(F), axis=1)
    Fv = F[valid]
    if method in ("shifted_geometric_mean", "geometric_mean"):
        shift = pseudocount if method == "shifted_geometric_mean" else 1e-10
        with np.errstate(invalid="ignore", divide="ignore"):
            m = row_sum(_log(Fv.astype(np.float64) + shift)) / float(f)
        e = _exp(m)
        sv = (e - pseudocount if method == "shifted_geometric_mean" else e).astype(T)
    elif method == "arithmetic_mean":
        sv = (row_sum(Fv).astype(np.float64) / float(f)).astype(T)
    elif method == "median":
        s = np.sort(Fv, axis=1)
        sv = s[:, f // 2] if f % 2 else (s[:, f // 2 - 1] + s[:, f // 2]) / T(2)
    elif method == "minimum":
        sv = Fv.min(axis=1)
    else:
        raise ValueError(method)
    score = np.full(n, np.nan, dtype=T)
    score[valid] = sv
    full = np.where(valid, score, T(0)).astype(np.float64)      # rows that are not valid add nothing
    nv = int(valid.sum())
    return {"valid": valid, "score": score, "min": float(sv.min()) if nv else np.inf,
            "max": float(sv.max()) if nv else -np.inf, "mean": float(block_sum(full)) / nv if nv else np.nan,
            "n_valid": nv, "n_below": int((sv < T(1e-6)).sum()), "n_negative": int(np.any(Fv < 0, axis=1).sum())}


def ks_background(scores, q):
    """sc_ks_prepare: the sorted fp64 scores, background mean and population standard deviation."""
    s = np.sort(np.asarray(scores).astype(np.float64))
    m = min(max(int(s.size * q), 10), s.size)
    mean = float(block_sum(s[:m])) / m
    d = s[:m] - mean
    return s, mean, float(np.sqrt(float(block_sum(d * d)) / m))


def ks_deviation(sorted_scores, mean, sd):
    s = sorted_scores
    return np.arange(1, s.size + 1) / float(s.size) - ndtr((s - mean) / sd)


def ks(scores, q=0.5):
    """threshold_ks with the device's arithmetic and the host's two fallbacks as numpy takes them on the scores' type.
    Returns threshold, deviation scores (fp64), labels, params (with the argmax, D and which fallbacks fired)."""
    x = np.asarray(scores)
    T = x.dtype.type
    s, mean, sd = ks_background(x, q)
    st = s.astype(T)                                  # exact: the sorted scores in their own type
    fallback = ""
    if sd < 1e-10:
        q25, q75 = np.percentile(st, [25, 75])
        iqr = q75 - q25
        if iqr > 1e-10:
            sd, fallback = float(iqr / 1.35), "iqr"
        else:
            sd, fallback = float(max((st[-1] - st[0]) * 0.1, 1e-6)), "range"
    D = ks_deviation(s, mean, sd)
    i = int(np.argmax(D))
    thr = float(s[i])
    p90 = thr <= mean
    if p90:
        thr = float(np.percentile(st, 90))
    rng = max(float(s[-1]) - thr, 1e-10)
    x64 = x.astype(np.float64)
    dev = np.clip((x64 - thr) / rng, 0.0, 1.0)
    return thr, dev, (x64 >= thr).astype(np.int32), {
        "background_mean": mean, "background_std": sd, "argmax": i, "D": float(D[i]), "std_fallback": fallback,
        "p90_fallback": bool(p90), "sorted": s}


def kmeans_run_labels(scores, K, draws, max_iter=300):
    """labels_ of KMeans(K, n_init=1).fit(scores[:, None]) for every run of ``draws`` (n_init, 1 + (K - 1) L), with
    sc_kmeans_fit's summation orders for a call with these n_init runs."""
    X = np.ascontiguousarray(np.asarray(scores).reshape(-1, 1))
    tol = float(np.mean(np.var(X, axis=0)) * 1e-4)
    Xc = X - X.mean(axis=0)
    R = draws.shape[0]
    nb = kr.workgroups(X.shape[0], 1, K, R)
    out = np.empty((R, X.shape[0]), dtype=np.int32)
    for r in range(R):
        seeds = kr.seeding(Xc, K, draws[r])
        out[r] = kr.lloyd(Xc, Xc[seeds], max_iter, tol, nb)[0]
    return out


def _derived(w, var):
    p = 1.0 / np.sqrt(var)
    return p, _log(p), _log(w)


def weighted_log_prob(x, w, mu, var, derived=None):
    p, lp, lw = derived if derived is not None else _derived(w, var)
    y = x[:, None] * p[None, :] - (mu * p)[None, :]
    return (-0.5 * (LOG_2PI + y * y) + lp[None, :]) + lw[None, :]


def log_sum_exp(wl):
    m = wl.max(axis=1)
    s = np.zeros(wl.shape[0])
    for k in range(wl.shape[1]):
        s = s + _exp(wl[:, k] - m)
    return _log(s) + m


def em_run(x, labels, K, max_iter=100, tol=1e-3, reg=1e-6, trace=None):
    """One run of sc_gmm_fit from its k-means labels: weights, means, variances, lower bound, n_iter, converged.
    trace: a list that receives every iteration's change of the lower bound."""
    x = np.asarray(x).astype(np.float64)
    n = x.size
    onehot = (labels[:, None] == np.arange(K)[None, :]).astype(np.float64)
    nk = block_sum(onehot) + EPS10
    mu = block_sum(onehot * x[:, None]) / nk
    d = x[:, None] - mu[None, :]
    var = block_sum(onehot * (d * d)) / nk + reg
    w = nk / float(n)
    derived = _derived(w, var)
    lb, n_iter, converged = -np.inf, 0, False
    for _ in range(max_iter):
        wl = weighted_log_prob(x, w, mu, var, derived)
        lse = log_sum_exp(wl)
        resp = _exp(wl - lse[:, None])
        d = x[:, None] - mu[None, :]
        S0, S1 = block_sum(resp), block_sum(resp * x[:, None])
        A, B = block_sum(resp * d), block_sum(resp * (d * d))
        nk = S0 + EPS10
        m = S1 / nk
        dm = m - mu
        var = ((B - (2.0 * dm) * A) + (dm * dm) * S0) / nk + reg
        mu = m
        tot = 0.0
        for k in range(K):
            tot = tot + nk[k]
        w = nk / tot
        derived = _derived(w, var)
        new = float(block_sum(lse)) / n
        change, lb = new - lb, new
        n_iter += 1
        if trace is not None:
            trace.append(change)
        if abs(change) < tol:
            converged = True
            break
    return w, mu, var, lb, n_iter, converged


def gmm_fit(scores, K, draws, max_iter=100, tol=1e-3, reg=1e-6, km_labels=None, km_max_iter=300):
    """sc_gmm_fit: every run's parameters and the best run (strictly larger lower bound)."""
    x = np.asarray(scores)
    R = draws.shape[0]
    if km_labels is None:
        km_labels = kmeans_run_labels(x, K, draws, km_max_iter)
    out = {"weights": np.empty((R, K)), "means": np.empty((R, K)), "variances": np.empty((R, K)),
           "lower_bound": np.empty(R), "n_iter": np.empty(R, dtype=np.int32), "converged": np.empty(R, dtype=bool),
           "km_labels": km_labels, "changes": []}
    best = 0
    for r in range(R):
        trace = []
        w, mu, var, lb, n_iter, conv = em_run(x, km_labels[r], K, max_iter, tol, reg, trace)
        out["weights"][r], out["means"][r], out["variances"][r] = w, mu, var
        out["lower_bound"][r], out["n_iter"][r], out["converged"][r] = lb, n_iter, conv
        out["changes"].append(trace)
        if lb > out["lower_bound"][best]:
            best = r
    out["best"] = best
    return out


def gmm_posterior(scores, w, mu, var, high, cutoff):
    """sc_gmm_posterior: P(high) = the responsibilities of the components ``high`` added in order; labels."""
    x = np.asarray(scores).astype(np.float64)
    w, mu, var = (np.asarray(a, dtype=np.float64) for a in (w, mu, var))
    p = 1.0 / np.sqrt(var)
    wl = weighted_log_prob(x, w, mu, var, (p, np.log(p), np.log(w)))     # the host forms these: numpy's own log
    lse = log_sum_exp(wl)
    prob = np.zeros(x.size)
    for k in high:
        prob = prob + _exp(wl[:, k] - lse)
    return prob, (prob > cutoff).astype(np.int32)


def gmm_threshold(w, mu, var, K):
    """threshold_gmm's cutoff from fitted parameters (TH:283-328): for K = 2 the first sign change of P(high) - 0.5 on a
    1000-point grid between the two means (their midpoint without one); for K >= 3 the midpoint of the two lowest
    means.  Returns threshold, the components summed into P(high) in order, the argsort of the means."""
    order = np.argsort(mu)
    if K == 2:
        hi = int(np.argmax(mu))
        lo = 1 - hi
        grid = np.linspace(mu[lo], mu[hi], 1000)
        prob, _ = gmm_posterior(grid, w, mu, var, [hi], 0.5)
        cross = np.where(np.diff(np.sign(prob - 0.5)))[0]
        thr = float(grid[cross[0]]) if len(cross) else float((mu[lo] + mu[hi]) / 2)
        return thr, [hi], order
    return float((mu[order[0]] + mu[order[1]]) / 2), [int(k) for k in order[1:]], order


# ---- tests/golden/ref_threshold.npz (scripts/make_threshold_golden.py) -------------------------------------------------
def golden_cases(z):
    """One dict per full-call case of the golden file: name, feature matrix in the case's type (NaN / Inf cells
    injected where the case has them), the call's arguments and the case's scalars (flags, measured deviations)."""
    out = []
    for name, key, dtype, metagene_method, threshold_method, with_bad in z["cases"]:
        M = z[f"input_{key}"].copy()
        if with_bad == "1":
            M[z["bad_nan_cells"][:, 0], z["bad_nan_cells"][:, 1]] = np.nan
            M[z["bad_inf_cells"][:, 0], z["bad_inf_cells"][:, 1]] = np.inf
        stat = dict(zip(z[f"{name}_stat_names"].tolist(), z[f"{name}_stat_values"].tolist()))
        kwargs = {"metagene_method": str(metagene_method), "threshold_method": str(threshold_method),
                  "n_components": int(stat["n_components"]), "max_cells": int(stat["max_cells"])}
        out.append({"name": str(name), "features": np.ascontiguousarray(M.astype(dtype)), "kwargs": kwargs, "stat": stat})
    return out


def reference_tolerance(dev, ulp):
    """Tolerance against the reference's recorded output: 4 x the deviation the generator measured between this
    restatement and the reference.  Where that deviation is exactly 0 the restatement IS the reference's computation,
    the comparison is the one against the restatement, and its tolerance (16 x the one-ulp spread) applies."""
    return 4.0 * dev if dev > 0 else 16.0 * ulp


def sorted_parameters(w, mu, var):
    """weights | means | variances with the components ordered by mean (the winner's component order is noise)."""
    o = np.argsort(mu)
    return np.concatenate([np.asarray(w)[o], np.asarray(mu)[o], np.asarray(var)[o]])


class RestatedContext:
    """The threshold methods of spatialcore_amd._lib.Context answered by this restatement: lets the CPU tests drive the
    package's Python layer (validation, fallbacks, side effects) end to end without a device."""

    def metagene_score(self, features, method, pseudocount=0.1):
        return metagene(features, method, pseudocount)

    def ks_prepare(self, scores, background_quantile, ranks=(), return_sorted=False):
        s, mean, sd = ks_background(scores, background_quantile)
        self._sorted = s
        return {"bg_mean": mean, "bg_std": sd, "order": s[np.asarray(ranks, dtype=np.int64)],
                "sorted": s if return_sorted else None}

    def ks_argmax(self, bg_mean, bg_std):
        D = ks_deviation(self._sorted, bg_mean, bg_std)
        i = int(np.argmax(D))
        return i, float(self._sorted[i]), float(D[i])

    def ks_classify(self, scores, threshold, max_score):
        x = np.asarray(scores).astype(np.float64)
        dev = np.clip((x - threshold) / max(max_score - threshold, 1e-10), 0.0, 1.0)
        lab = (x >= threshold).astype(np.int32)
        return dev, lab, int(lab.sum())

    def gmm_fit(self, scores, n_components, n_init, km_max_iter, km_tol, x_mean, uniforms, max_iter=100, tol=1e-3,
                reg_covar=1e-6, return_km_labels=False):
        return gmm_fit(scores, n_components, np.asarray(uniforms).reshape(n_init, -1), max_iter, tol, reg_covar,
                       km_max_iter=km_max_iter)

    def gmm_posterior(self, scores, weights, means, variances, high, cutoff):
        prob, lab = gmm_posterior(scores, weights, means, variances, list(high), cutoff)
        return prob, lab, int(lab.sum())
