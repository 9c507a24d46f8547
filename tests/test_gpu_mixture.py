"""sc_mixture_fit / sc_mixture_predict and cluster.gaussian_mixture on the device against sklearn 1.7.2's GaussianMixture and
tests/mixture_restated.py.

Protocol of the parity tests: the device, the restatement and sklearn start from the same k-means labels
(KMeans(K, n_init=1, random_state=RandomState(0)), which the device replays itself), run with tol = 0 and the same max_iter,
and the largest difference of weights, means and covariances relative to each array's largest entry is compared with
MARGIN, against sklearn and against the restatement, after max_iter 5 and 30."""
import functools
import hashlib
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import hops_restated as H
import mixture_restated as R
from conftest import make_adata

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Ten times the largest parameter distance measured on the MI355X over every case of this file (2.91e-13, device against
# sklearn at (4096, 4, 64) "diag" after 30 iterations; "full" reaches 6.8e-14 there); the loosest allowed is 1e-9.
# RESTATEMENT_MEASURED: device against restatement, parameters and lower bound: at most 6.7e-14 after 5 and after 30
# iterations ((1200, 256, 2) "full"); responsibilities: at most 1.2e-14 after 5 and 2.2e-12 after 30 iterations (both at
# (4096, 4, 64) "full", 64 overlapping components in 4 dimensions), held to the same MARGIN.
MARGIN = 3e-12
SHAPES = [(257, 1, 2), (1000, 3, 2), (1031, 17, 5), (2049, 64, 3), (1500, 65, 3), (1200, 255, 2), (1200, 256, 2), (4096, 4, 64)]
TYPES = ("full", "diag")


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


@functools.lru_cache(maxsize=None)
def _input(n, D, K, dtype="float64", rare=False):
    sep = 4.0 if K == 64 else 2.0
    weights = None
    if rare:
        weights = np.full(K, (1.0 - 0.01) / (K - 1))
        weights[K - 1] = 0.01
    X, z = R.planted(n, D, K, sep, seed=n + D, weights=weights, dtype=np.dtype(dtype))
    X.setflags(write=False)
    return X, z


@functools.lru_cache(maxsize=None)
def _sklearn(n, D, K, ct, max_iter, tol=0.0, n_init=1, dtype="float64", rare=False):
    X, _ = _input(n, D, K, dtype, rare)
    return R.sklearn_fit(X, K, ct, n_init=n_init, max_iter=max_iter, tol=tol, seed=0)


@functools.lru_cache(maxsize=None)
def _device(n, D, K, ct, max_iter, tol=0.0, n_init=1, dtype="float64", rare=False):
    from spatialcore_amd.cluster.mixture import _fit

    X, _ = _input(n, D, K, dtype, rare)
    return _fit(_ctx(), X, K, ct, n_init, max_iter, tol, 1e-6, 0, True)


def _best(fit):
    b = fit["best"]
    return fit["weights"][b], fit["means"][b], fit["covariances"][b]


def _check_against_sklearn(n, D, K, ct, max_iter, **kw):
    fit = _device(n, D, K, ct, max_iter, **kw)
    gm, labels = _sklearn(n, D, K, ct, max_iter, **kw)
    d = R.parameter_distance(*_best(fit), gm)
    print(f"mixture parity n={n} D={D} K={K} {ct} max_iter={max_iter} {kw}: device - sklearn {d:.3e}")
    assert d <= MARGIN
    # labels: equal except where sklearn's own two best log-probabilities are closer than 1e-6; at most 1 % such cells
    X, _ = _input(n, D, K, kw.get("dtype", "float64"), kw.get("rare", False))
    out = R.ambiguous_cells(gm, X)
    assert out.mean() <= 0.01
    assert np.array_equal(fit["labels"][~out], labels[~out])
    return d


# ---- 1, 2. parity of the parameters and the labels ---------------------------------------------------------------------------
@pytest.mark.parametrize("ct", TYPES)
@pytest.mark.parametrize("n,D,K", SHAPES)
def test_device_against_sklearn(n, D, K, ct):
    """One past an MFMA tile (17), the block edge (64, 65), the cap (255, 256; 600 cells per component > D) and the K cap.
    Measured on the MI355X: see MARGIN."""
    for max_iter in (5, 30):
        _check_against_sklearn(n, D, K, ct, max_iter)


@functools.lru_cache(maxsize=None)
def _restated(n, D, K, ct, max_iter):
    X, _ = _input(n, D, K)
    return R.fit(X, K, ct, max_iter=max_iter, tol=0.0, seed=0)


@pytest.mark.parametrize("max_iter", (5, 30))
@pytest.mark.parametrize("ct", TYPES)
@pytest.mark.parametrize("n,D,K", SHAPES)
def test_device_against_restatement(n, D, K, ct, max_iter):
    """Parameters, lower bound and responsibilities after 5 and after 30 iterations.  Measured on the MI355X: see
    RESTATEMENT_MEASURED above."""
    fit = _device(n, D, K, ct, max_iter)
    want = _restated(n, D, K, ct, max_iter)
    run = want["runs"][0]
    d = max(R.distance(fit["weights"][0], run["weights"]), R.distance(fit["means"][0], run["means"]),
            R.distance(fit["covariances"][0], run["covariances"]), abs(fit["lower_bound"][0] - run["lower_bound"]) / abs(run["lower_bound"]))
    dp = R.distance(fit["proba"], want["proba"])
    print(f"mixture parity n={n} D={D} K={K} {ct} max_iter={max_iter}: device - restatement {d:.3e}, responsibilities {dp:.3e}")
    assert d <= MARGIN
    assert fit["n_iter"][0] == run["n_iter"] == max_iter and not fit["converged"][0]
    assert dp <= MARGIN


@pytest.mark.parametrize("ct", TYPES)
@pytest.mark.parametrize("delta", (-1, 0, 1, None))
def test_slice_edges(ct, delta):
    """n at the M-step slice length S - 1, S, S + 1 and 2 S + 1."""
    from spatialcore_amd import _lib

    S = _lib.mixture_slice_rows(1000, 6, 3, ct)
    n = 2 * S + 1 if delta is None else S + delta
    assert _lib.mixture_slice_rows(n, 6, 3, ct) == S
    _check_against_sklearn(n, 6, 3, ct, 5)


@pytest.mark.parametrize("ct", TYPES)
def test_float32_input(ct):
    """float32 values are widened first: the fit is that of the widened matrix, and sklearn's on it."""
    fit = _device(1031, 17, 5, ct, 5, dtype="float32")
    _check_against_sklearn(1031, 17, 5, ct, 5, dtype="float32")
    from spatialcore_amd.cluster.mixture import _fit

    X, _ = _input(1031, 17, 5, "float32")
    wide = _fit(_ctx(), X.astype(np.float64), 5, ct, 1, 5, 0.0, 1e-6, 0, True)
    for k in ("weights", "means", "covariances", "lower_bound", "labels", "proba"):
        assert fit[k].tobytes() == wide[k].tobytes()


@pytest.mark.parametrize("ct", TYPES)
def test_rare_component(ct):
    """A component the recipe gives 1 % of the cells."""
    _check_against_sklearn(3000, 6, 4, ct, 30, rare=True)


@pytest.mark.parametrize("ct", TYPES)
def test_stop_rule_and_best_run(ct):
    """sklearn's default tol: n_iter, converged and the best of three runs equal sklearn's."""
    fit = _device(1031, 17, 5, ct, 100, tol=1e-3, n_init=3)
    X, _ = _input(1031, 17, 5)
    gms = [R.fit_from_labels(X, lab, 5, ct, 100, 1e-3) for lab in R.kmeans_labels(X, 5, 3, 0)]
    lbs = [g["lower_bound"] for g in gms]
    gm, labels = _sklearn(1031, 17, 5, ct, 100, tol=1e-3, n_init=3)
    best = int(np.argmax(lbs))
    assert fit["best"] == best
    assert [int(v) for v in fit["n_iter"]] == [g["n_iter"] for g in gms]
    assert [bool(v) for v in fit["converged"]] == [g["converged"] for g in gms]
    assert fit["n_iter"][best] == gm.n_iter_ and bool(fit["converged"][best]) == gm.converged_
    assert abs(fit["lower_bound"][best] - gm.lower_bound_) <= MARGIN * abs(gm.lower_bound_)
    assert R.parameter_distance(*_best(fit), gm) <= MARGIN


# ---- 3. consistency ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", TYPES)
@pytest.mark.parametrize("n,D,K", [(1031, 17, 5), (1500, 65, 3), (4096, 4, 64)])
def test_predict_returns_the_fits_bytes(n, D, K, ct):
    fit = _device(n, D, K, ct, 5)
    X, _ = _input(n, D, K)
    labels, proba, loglik = _ctx().mixture_predict(X, ct, *_best(fit), return_proba=True)
    assert labels.tobytes() == fit["labels"].tobytes()
    assert proba.tobytes() == fit["proba"].tobytes()
    assert loglik == fit["loglik"]
    rows = np.array([math.fsum(row) for row in proba])      # the exact sum, correctly rounded: no summation error of the test's own
    print(f"mixture rows n={n} D={D} K={K} {ct}: |sum - 1| <= {np.max(np.abs(rows - 1.0)) / np.finfo(np.float64).eps:.1f} ulp")
    assert np.max(np.abs(rows - 1.0)) <= 4 * np.finfo(np.float64).eps
    # other cells: the log-likelihood against sklearn's score_samples under the same parameters
    gm, _ = _sklearn(n, D, K, ct, 5)
    other, _ = R.planted(777, D, K, 2.0, seed=99)
    gm2 = _with_parameters(gm, ct, *_best(fit))
    _, _, ll = _ctx().mixture_predict(other, ct, *_best(fit))
    want = gm2.score_samples(other).mean()
    print(f"mixture loglik n={n} D={D} K={K} {ct}: {abs(ll - want) / abs(want):.3e}")
    assert abs(ll - want) <= MARGIN * abs(want)


def _with_parameters(gm, ct, w, mu, cov):
    import copy

    from sklearn.mixture._gaussian_mixture import _compute_precision_cholesky

    g = copy.deepcopy(gm)
    g.weights_, g.means_, g.covariances_ = w, mu, cov
    g.precisions_cholesky_ = _compute_precision_cholesky(cov, ct)
    return g


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------
_CHILD = """
import hashlib, sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import mixture_restated as R
from spatialcore_amd import _lib
from spatialcore_amd.cluster.mixture import _fit
for ct in ("full", "diag"):
    X, _ = R.planted(2049, 65, 3, 2.0, seed=5)
    f = _fit(_lib.default_context(0), X, 3, ct, 2, 8, 0.0, 1e-6, 0, True)
    h = hashlib.sha256()
    for k in ("labels", "proba", "weights", "means", "covariances", "lower_bound"):
        h.update(f[k].tobytes())
    print("digest", ct, h.hexdigest())
"""


def _digests():
    from spatialcore_amd.cluster.mixture import _fit

    lines = []
    for ct in TYPES:
        X, _ = R.planted(2049, 65, 3, 2.0, seed=5)
        f = _fit(_ctx(), X, 3, ct, 2, 8, 0.0, 1e-6, 0, True)
        h = hashlib.sha256()
        for k in ("labels", "proba", "weights", "means", "covariances", "lower_bound"):
            h.update(f[k].tobytes())
        lines.append(f"digest {ct} {h.hexdigest()}")
    return lines


def test_two_calls_and_a_child_on_four_hardware_queues_give_the_same_bytes(tmp_path):
    first = _digests()
    assert _digests() == first
    script = tmp_path / "mixture_child.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    run = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert [line for line in run.stdout.splitlines() if line.startswith("digest ")] == first


# ---- 5. one component --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", TYPES)
def test_one_component(ct):
    from spatialcore_amd.cluster.mixture import _fit

    X, _ = R.planted(1500, 9, 3, 2.0, seed=3)
    f = _fit(_ctx(), X, 1, ct, 1, 5, 1e-3, 1e-6, 0, True)
    cov = np.cov(X.T, bias=True) + 1e-6 * np.eye(9)
    assert R.distance(f["means"][0, 0], X.mean(0)) <= MARGIN
    assert R.distance(f["covariances"][0, 0], cov if ct == "full" else np.diag(cov)) <= MARGIN
    assert not f["labels"].any() and np.all(f["proba"] == 1.0) and f["weights"][0, 0] == 1.0


# ---- 6. ill-defined covariance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", TYPES)
def test_ill_defined_covariance_is_refused_and_the_context_stays_usable(ct):
    """reg_covar = 0 with one component's 40 cells identical: refused by the flag, as sklearn refuses it."""
    from spatialcore_amd import _lib
    from spatialcore_amd.cluster import gaussian_mixture

    rng = np.random.default_rng(0)
    X = np.vstack([np.zeros((40, 8)), rng.normal(50.0, 1.0, size=(400, 8))])   # the identical cells' mean is exact
    ctx = _ctx()
    km_tol = float(np.mean(np.var(X, axis=0)) * 1e-4)
    from spatialcore_amd.spatial.neighborhoods import kmeans_draws

    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        ctx.mixture_fit(X, 2, ct, 1, 300, km_tol, X.mean(0), kmeans_draws(0, 1, 2), 20, 1e-3, 0.0)
    # the entry point itself: the code it returns, not only what the binding makes of it
    import ctypes

    P, K, D = ctypes.c_void_p, 2, 8
    Xc = np.ascontiguousarray(X)
    xm, u = np.ascontiguousarray(X.mean(0)), np.ascontiguousarray(kmeans_draws(0, 1, K))
    full = ct == "full"
    w, mu, cov = np.empty(K), np.empty((K, D)), np.empty((K, D, D) if full else (K, D))
    lb, it, cv, lab = np.empty(1), np.empty(1, np.int32), np.empty(1, np.int32), np.empty(440, np.int32)
    best, ll = ctypes.c_int32(0), ctypes.c_double(0.0)
    ptr = lambda a: a.ctypes.data_as(P)   # noqa: E731
    rc = ctx._lib.sc_mixture_fit(ctx._h, ptr(Xc), _lib.SC_F64, 440, D, K, _lib.MIX_COVARIANCES[ct], 1, 300, km_tol, ptr(xm), ptr(u), 20,
                                 1e-3, 0.0, ptr(w), ptr(mu), ptr(cov), ptr(lb), ptr(it), ptr(cv), ctypes.byref(best), ptr(lab), None,
                                 ctypes.byref(ll))
    assert rc == _lib.SC_ERR_ILLDEFINED == 6
    assert b"not positive definite" in ctx._lib.sc_last_error()
    ad = make_adata(np.zeros((440, 2)), np.zeros((440, 2)))
    ad.obsm["X_cellcharter"] = X
    with pytest.raises(ValueError, match="increase reg_covar"):
        gaussian_mixture(ad, 2, covariance_type=ct, reg_covar=0.0)
    gaussian_mixture(ad, 2, covariance_type=ct)          # the same context, a valid call
    assert sorted(ad.uns["spatial_cluster"]["sizes"].tolist()) == [40, 400]


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------
def test_domains_end_to_end():
    """aggregate_neighbors(n_layers=3) then gaussian_mixture(2) on the planted two-domain recipe of hops_restated: the labels
    are sklearn's on the same features (rule of test 2), so the ARI against the planted domains is at least sklearn's."""
    from spatialcore_amd.cluster import gaussian_mixture, predict_gaussian_mixture
    from spatialcore_amd.spatial import aggregate_neighbors

    xy, X, domain = H.domain_recipe(0)
    ad = make_adata(xy, np.zeros((4000, 2)))
    ad.obsm["X_pca"] = X
    aggregate_neighbors(ad, n_layers=3, n_neighbors=6)
    F = np.asarray(ad.obsm["X_cellcharter"], dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gaussian_mixture(ad, 2, proba_key="X_domain_proba")
    gm, labels = R.sklearn_fit(F, 2, "full", seed=0)
    got = np.asarray(ad.obs["spatial_cluster"].cat.codes)
    out = R.ambiguous_cells(gm, F)
    assert out.mean() <= 0.01 and np.array_equal(got[~out], labels[~out])
    assert H.ari(got, domain) >= H.ari(labels, domain)
    entry = ad.uns["spatial_cluster"]
    assert abs(entry["bic"] - gm.bic(F)) <= 1e-9 * abs(gm.bic(F)) and abs(entry["aic"] - gm.aic(F)) <= 1e-9 * abs(gm.aic(F))
    assert list(ad.obs["spatial_cluster"].cat.categories) == ["0", "1"] and ad.obs["spatial_cluster"].cat.ordered
    assert ad.obsm["X_domain_proba"].shape == (4000, 2)
    other = make_adata(xy, np.zeros((4000, 2)))
    other.obsm["X_cellcharter"] = ad.obsm["X_cellcharter"]
    predict_gaussian_mixture(other, ad)
    assert np.array_equal(np.asarray(other.obs["spatial_cluster"].cat.codes), got)
    assert other.uns["spatial_cluster"]["loglik"] == entry["loglik"]


def test_autok_chooses_the_three_planted_domains():
    """gaussian_mixture_autok((2, 5), max_runs=3) on three planted domains (mixture_restated.three_domain_recipe, seed 1)
    chooses 3, as the restated rule does with sklearn's fits (random_state + r) at K = 1 .. 6 -- checked on the CPU first:
    stabilities 0.80 / 0.86 / 0.83 / 0.76 -- and agrees with it in the similarities, the stabilities and the best run's
    labels."""
    from spatialcore_amd.cluster import gaussian_mixture_autok
    from spatialcore_amd.cluster.mixture import autok_rule

    xy, X, domain = R.three_domain_recipe(1)
    F = H.features(H.knn_union(xy, 6), X, [1, 2, 3], ["mean"])
    ad = make_adata(xy, np.zeros((3000, 2)))
    ad.obsm["X_cellcharter"] = F
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gaussian_mixture_autok(ad, (2, 5), max_runs=3)
    fits = {K: [R.sklearn_fit(F, K, "full", seed=r) for r in range(3)] for K in range(1, 7)}
    best, stability, sim = autok_rule({K: [f[1] for f in fits[K]] for K in fits}, 2, 5)
    got = ad.uns["spatial_cluster_autok"]
    assert best == 3 and got["best_k"] == 3 and got["n_clusters"].tolist() == [2, 3, 4, 5]
    assert np.max(np.abs(got["stability"] - [stability[K] for K in (2, 3, 4, 5)])) <= 1e-9
    assert np.max(np.abs(got["similarity"] - [sim[K] for K in (1, 2, 3, 4, 5)])) <= 1e-9
    lbs = [f[0].lower_bound_ for f in fits[3]]
    assert np.max(np.abs(got["lower_bound"][2] - lbs)) <= MARGIN * np.max(np.abs(lbs))
    run = int(np.argmax(lbs))
    assert ad.uns["spatial_cluster"]["params"]["random_state"] == run
    gm, labels = fits[3][run]
    out = R.ambiguous_cells(gm, F)
    assert out.mean() <= 0.01 and np.array_equal(np.asarray(ad.obs["spatial_cluster"].cat.codes)[~out], labels[~out])
    assert H.ari(np.asarray(ad.obs["spatial_cluster"].cat.codes), domain) >= 0.9
