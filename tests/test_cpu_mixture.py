"""cluster.gaussian_mixture without a device: the numpy restatement of the device's arithmetic (tests/mixture_restated.py)
against sklearn 1.7.2's GaussianMixture, the stop rule, the Fowlkes-Mallows helper, the autoK rule, BIC / AIC and every
argument check of the three public functions (all made before a context exists)."""
import numpy as np
import pytest

import mixture_restated as R
from conftest import make_adata
from spatialcore_amd import _lib
from spatialcore_amd.cluster import gaussian_mixture, gaussian_mixture_autok, predict_gaussian_mixture
from spatialcore_amd.cluster import mixture as M

# (n, D, K, sep, correlated columns appended)
SHAPES = [(3000, 12, 4, 3.0, 0), (2500, 40, 5, 1.5, 0), (1500, 64, 3, 1.5, 0), (2000, 8, 3, 0.6, 8), (2000, 24, 4, 0.8, 24)]
# Ten times the largest distance measured (7.2e-14, at (1500, 64, 3) "full", max_iter 5); the loosest allowed is 1e-9.
MARGIN = 7.2e-13


@pytest.mark.parametrize("ct", ("full", "diag"))
@pytest.mark.parametrize("n,D,K,sep,corr", SHAPES)
def test_restatement_against_sklearn(n, D, K, sep, corr, ct):
    """Same k-means labels (KMeans(K, n_init=1, random_state=RandomState(0))), tol = 0, max_iter 5 and 30.  Measured: at
    most 7.2e-14 over the twenty cases ("full" up to 7.2e-14, "diag" up to 4.2e-14: sklearn's one-pass diagonal variance
    against the two-pass one here)."""
    X, _ = R.planted(n, D, K, sep, seed=1, correlated=corr)
    lab = R.kmeans_labels(X, K, 1, 0)[0]
    for max_iter in (5, 30):
        run = R.fit_from_labels(X, lab, K, ct, max_iter, 0.0)
        gm, _ = R.sklearn_fit(X, K, ct, max_iter=max_iter, tol=0.0, seed=0)
        d = R.parameter_distance(run["weights"], run["means"], run["covariances"], gm)
        print(f"restatement - sklearn n={n} D={D + corr} K={K} {ct} max_iter={max_iter}: {d:.3e}")
        assert d <= MARGIN
        assert not R.ambiguous_cells(gm, X).any()


@pytest.mark.parametrize("ct", ("full", "diag"))
def test_stop_rule_and_best_run(ct):
    X, _ = R.planted(2000, 8, 3, 0.6, seed=1, correlated=8)
    got = R.fit(X, 3, ct, n_init=3, seed=0)
    gm, labels = R.sklearn_fit(X, 3, ct, n_init=3, seed=0)
    best = got["runs"][got["best"]]
    assert best["n_iter"] == gm.n_iter_ and best["converged"] == gm.converged_
    assert abs(best["lower_bound"] - gm.lower_bound_) <= MARGIN * abs(gm.lower_bound_)
    assert R.parameter_distance(best["weights"], best["means"], best["covariances"], gm) <= 1e-9
    assert np.array_equal(got["labels"], labels)
    # each run alone, as sklearn runs it from the same labels
    from sklearn.mixture import GaussianMixture

    rs = np.random.RandomState(0)
    for run in got["runs"]:
        one = GaussianMixture(3, covariance_type=ct, n_init=1, random_state=rs).fit(X)
        assert (run["n_iter"], run["converged"]) == (one.n_iter_, one.converged_)


def test_fowlkes_mallows_against_sklearn():
    from sklearn.metrics import fowlkes_mallows_score

    rng = np.random.default_rng(0)
    a = rng.integers(0, 4, size=5000)
    cases = [(a, a), (a, rng.integers(0, 7, size=5000)), (a, np.where(rng.random(5000) < 0.1, rng.integers(0, 4, size=5000), a)),
             (np.zeros(50, dtype=int), np.zeros(50, dtype=int)), (np.zeros(5000, dtype=int), a), (a, (a + 1) % 4),
             (np.arange(6), np.arange(6))]
    for x, y in cases:
        assert abs(M.fowlkes_mallows(x, y) - fowlkes_mallows_score(x, y)) <= 1e-12
    assert M.fowlkes_mallows(a, a) == 1.0
    with pytest.raises(ValueError, match="same non-zero length"):
        M.fowlkes_mallows([0, 1], [0])
    with pytest.raises(ValueError, match="non-negative"):
        M.fowlkes_mallows([0, -1], [0, 1])


def test_autok_rule_on_hand_made_labellings():
    """Labellings at K = 1 .. 5 for (lo, hi) = (2, 4).  Two runs per K."""
    n = 120
    base = np.arange(n)
    one = np.zeros(n, dtype=int)
    two = base // 60
    three = base // 40
    # K = 4, 5: the halves of K = 2 split differently in the two runs -> unstable
    four_a, four_b = base // 30, (base // 60) * 2 + base % 2
    five_a, five_b = np.minimum(base // 24, 4), base % 5
    tables = {1: [one, one], 2: [two, two], 3: [three, three], 4: [four_a, four_b], 5: [five_a, five_b]}
    best, stability, sim = M.autok_rule(tables, 2, 4)
    assert set(stability) == {2, 3, 4} and set(sim) == {1, 2, 3, 4}
    for K in (1, 2, 3, 4):
        want = np.mean([M.fowlkes_mallows(a, b) for a in tables[K] for b in tables[K + 1]])
        assert sim[K] == want
    for K in (2, 3, 4):
        assert stability[K] == (sim[K - 1] + sim[K]) / 2
    assert best == max(stability, key=lambda K: (stability[K], -K))
    # the ends are used: changing the labellings at lo - 1 or at hi + 1 changes the stabilities at lo and at hi
    other = dict(tables)
    other[1] = [base % 2, base % 2]
    other[5] = [five_b, five_b]
    _, stab2, _ = M.autok_rule(other, 2, 4)
    assert stab2[2] != stability[2] and stab2[4] != stability[4] and stab2[3] == stability[3]
    # ties go to the smaller K: identical nested labellings at every K give the same similarity pattern
    same = {K: [two, two] for K in range(1, 6)}
    assert M.autok_rule(same, 2, 4)[0] == 2
    tie = {1: [three], 2: [three], 3: [three], 4: [three], 5: [one]}
    best, stab, _ = M.autok_rule(tie, 2, 4)
    assert stab[2] == stab[3] == 1.0 and stab[4] < 1.0 and best == 2


def test_bic_and_aic_against_sklearn():
    X, _ = R.planted(1500, 12, 3, 2.0, seed=2)
    for ct in ("full", "diag"):
        got = R.fit(X, 3, ct, seed=0)
        gm, _ = R.sklearn_fit(X, 3, ct, seed=0)
        assert M.n_parameters(3, 12, ct) == gm._n_parameters()
        bic, aic = M.information_criteria(got["loglik"], 1500, 3, 12, ct)
        assert abs(bic - gm.bic(X)) <= 1e-9 * abs(gm.bic(X)) and abs(aic - gm.aic(X)) <= 1e-9 * abs(gm.aic(X))


def test_slice_rows_rule():
    assert _lib.mixture_slice_rows(1000, 64, 3) == 1024 and _lib.mixture_slice_rows(2049, 256, 64) == 1024
    assert _lib.mixture_slice_rows(10 ** 6, 64, 20) == 2464          # 409 slices of 20 x 32 KiB fit 256 MiB
    assert _lib.mixture_slice_rows(10 ** 6, 200, 20) == 25024        # ten blocks per component: 40 slices
    assert _lib.mixture_slice_rows(10 ** 6, 200, 20, "diag") == 1024
    for n, D, K in ((10 ** 6, 256, 64), (10 ** 7, 200, 20), (5000, 1, 1)):
        S = _lib.mixture_slice_rows(n, D, K)
        nb = (D + 63) // 64
        assert -(-n // S) * K * (nb * (nb + 1) // 2) * 64 * 64 * 8 <= max(1 << 28, K * (nb * (nb + 1) // 2) * 64 * 64 * 8)


# ---- argument checks: all before a context is made ---------------------------------------------------------------------------
def _adata(n=50, D=4, dtype=np.float64):
    ad = make_adata(np.zeros((n, 2)), np.zeros((n, 2)))
    ad.obsm["X_cellcharter"] = np.random.default_rng(0).normal(size=(n, D)).astype(dtype)
    return ad


@pytest.fixture
def no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a context was requested before the arguments were checked")

    monkeypatch.setattr(_lib, "default_context", boom)


@pytest.mark.parametrize("kw,match", [
    (dict(n_clusters=0), "n_clusters must be an integer in 1 .. 64"),
    (dict(n_clusters=65), "n_clusters must be an integer in 1 .. 64"),
    (dict(n_clusters=2.0), "n_clusters must be an integer"),
    (dict(n_clusters=True), "n_clusters must be an integer"),
    (dict(n_clusters=51), "cannot exceed the number of cells"),
    (dict(covariance_type="tied"), "'tied' is not supported"),
    (dict(covariance_type="spherical"), "'spherical' is not supported"),
    (dict(covariance_type="banana"), "must be 'full' or 'diag'"),
    (dict(n_init=0), "n_init must be an integer in 1 .. 10"),
    (dict(n_init=11), "n_init must be an integer in 1 .. 10"),
    (dict(max_iter=0), "max_iter must be an integer >= 1"),
    (dict(tol=-1e-3), "tol must be a finite number >= 0"),
    (dict(tol=float("nan")), "tol must be a finite number >= 0"),
    (dict(reg_covar=-1.0), "reg_covar must be a finite number >= 0"),
    (dict(reg_covar=float("inf")), "reg_covar must be a finite number >= 0"),
    (dict(random_state=-1), "random_state must be an integer"),
    (dict(random_state=None), "random_state must be an integer"),
    (dict(use_rep="X_missing"), "obsm\\['X_missing'\\] not found"),
    (dict(use_rep=""), "use_rep must be a non-empty string"),
    (dict(key_added=""), "key_added must be a non-empty string"),
    (dict(proba_key=3), "proba_key must be a non-empty string"),
])
def test_gaussian_mixture_refuses(kw, match, no_context):
    args = dict(n_clusters=3)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        gaussian_mixture(_adata(), **args)


def test_gaussian_mixture_refuses_the_representation(no_context):
    ad = _adata()
    ad.obsm["X_cellcharter"] = np.zeros((50, 257))
    with pytest.raises(ValueError, match="257 columns, need 1 .. 256"):
        gaussian_mixture(ad, 2)
    ad.obsm["X_cellcharter"] = np.zeros((50, 4), dtype=np.int64)
    with pytest.raises(ValueError, match="float32 or float64"):
        gaussian_mixture(ad, 2)
    bad = np.zeros((50, 4))
    bad[49, 3] = np.nan
    ad.obsm["X_cellcharter"] = bad
    with pytest.raises(ValueError, match="non-finite"):
        gaussian_mixture(ad, 2)


@pytest.mark.parametrize("kw,match", [
    (dict(n_clusters=(1, 4)), "n_clusters must be \\(lo, hi\\)"),
    (dict(n_clusters=(4, 3)), "n_clusters must be \\(lo, hi\\)"),
    (dict(n_clusters=5), "n_clusters must be \\(lo, hi\\)"),
    (dict(n_clusters=(2, 64)), "n_clusters must be \\(lo, hi\\)"),
    (dict(n_clusters=(2, 3.5)), "n_clusters must be \\(lo, hi\\)"),
    (dict(max_runs=0), "max_runs must be an integer in 1 .. 100"),
    (dict(n_clusters=(2, 50)), "cannot exceed the number of cells"),
    (dict(covariance_type="tied"), "'tied' is not supported"),
    (dict(max_iter=0), "max_iter must be an integer >= 1"),
    (dict(tol=-1.0), "tol must be a finite number"),
    (dict(random_state=2 ** 32 - 2), "random_state \\+ max_runs"),
    (dict(use_rep="nope"), "not found"),
    (dict(key_added=None), "key_added must be a non-empty string"),
])
def test_gaussian_mixture_autok_refuses(kw, match, no_context):
    args = dict(n_clusters=(2, 4))
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        gaussian_mixture_autok(_adata(), **args)


def _model(ct="full", K=2, D=4):
    cov = np.tile(np.eye(D), (K, 1, 1)) if ct == "full" else np.ones((K, D))
    return {"params": {"covariance_type": ct, "use_rep": "X_cellcharter", "key_added": "spatial_cluster"},
            "weights": np.full(K, 1.0 / K), "means": np.zeros((K, D)), "covariances": cov}


def test_predict_gaussian_mixture_refuses(no_context):
    ad = _adata()
    with pytest.raises(ValueError, match="model must be the uns entry"):
        predict_gaussian_mixture(ad, {"weights": [1.0]})
    with pytest.raises(ValueError, match="model.uns\\['spatial_cluster'\\] not found"):
        predict_gaussian_mixture(ad, _adata())
    m = _model()
    m["params"]["covariance_type"] = "tied"
    with pytest.raises(ValueError, match="covariance_type must be 'full' or 'diag'"):
        predict_gaussian_mixture(ad, m)
    m = _model()
    m["covariances"] = np.ones((2, 4))
    with pytest.raises(ValueError, match="does not fit 'full'"):
        predict_gaussian_mixture(ad, m)
    m = _model()
    m["means"] = np.zeros((3, 4))
    with pytest.raises(ValueError, match="weights must be \\(K,\\) and means \\(K, D\\)"):
        predict_gaussian_mixture(ad, m)
    m = _model()
    m["weights"] = np.array([1.0, 0.0])
    with pytest.raises(ValueError, match="weights must be finite and > 0"):
        predict_gaussian_mixture(ad, m)
    m = _model("diag")
    m["covariances"][1, 3] = np.inf
    with pytest.raises(ValueError, match="means and covariances finite"):
        predict_gaussian_mixture(ad, m)
    with pytest.raises(ValueError, match="has 4 columns, the mixture was fitted on 5"):
        predict_gaussian_mixture(ad, _model(D=5))
    with pytest.raises(ValueError, match="obsm\\['X_other'\\] not found"):
        predict_gaussian_mixture(ad, _model(), use_rep="X_other")
    with pytest.raises(ValueError, match="key_added must be a non-empty string"):
        predict_gaussian_mixture(ad, _model(), key_added="")
    with pytest.raises(ValueError, match="proba_key must be a non-empty string"):
        predict_gaussian_mixture(ad, _model(), proba_key="")


def test_error_code_maps_to_sklearns_message(monkeypatch):
    class Lib:
        @staticmethod
        def sc_last_error():
            return b"sc_mixture_fit: the covariance of component 1 is not positive definite"

    monkeypatch.setattr(_lib, "load_library", lambda: Lib)
    with pytest.raises(ValueError, match="ill-defined empirical covariance.*increase reg_covar"):
        _lib._check(_lib.SC_ERR_ILLDEFINED)
