"""The inputs of tests/test_gpu_threshold_edges.py are what those tests say they are -- against numpy, scipy and sklearn
alone, no GPU.  Per GMM input the three rules scripts/make_threshold_golden.py applies to its own cases: the restated
k-means labels of every run equal sklearn's, no change of the lower bound comes within 1e-9 of tol, and n_iter and
converged do not move under the one-ulp perturbations.  For the KS argmax the generator's ks_gap rule; for the K = 8
posteriors its cap on undecided cells."""
import warnings

import numpy as np
import pytest

import threshold_edge_inputs as ei
import threshold_restated as tr
from test_cpu_threshold import adata_of

TYPES = [np.float32, np.float64]


# ---- metagene ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("F", ei.FEATURE_COUNTS)
def test_restated_scores_are_numpys_at_every_feature_count(F, dtype):
    """arithmetic_mean, median and minimum of the restatement equal numpy's own on the edge matrix: with ties, signed
    zeros, and every shape of the pairwise sum (no loop, one pass, several, with and without a tail)."""
    for M in (ei.edge_features(300, F, dtype, F), ei.negative_features(300, F, dtype, 7 + F)):
        v = np.all(np.isfinite(M), axis=1)
        assert v.sum() == 298
        assert np.array_equal(tr.row_sum(M[v]), M[v].sum(axis=1))
        for method, fn in (("arithmetic_mean", np.mean), ("median", np.median), ("minimum", np.min)):
            r = tr.metagene(M, method)
            assert r["score"].dtype == M.dtype and np.array_equal(r["score"][v], fn(M[v], axis=1)), method
            assert (r["min"], r["max"], r["mean"]) == ei.stats_of_scores(r["score"], r["valid"])


def test_feature_counts_cover_every_shape_of_the_row_sum():
    passes = {F: (F - F % 8) // 8 - 1 for F in ei.FEATURE_COUNTS if F >= 8}      # rounds of the 8-accumulator loop
    assert min(ei.FEATURE_COUNTS) < 8 and max(ei.FEATURE_COUNTS) == 64
    assert {F for F, p in passes.items() if p == 0} == {8, 9, 15}
    assert {F for F, p in passes.items() if p == 1} == {16, 17}
    assert {F for F, p in passes.items() if p > 1} == {24, 33, 63, 64}
    assert {F for F in passes if F % 8} == {9, 15, 17, 33, 63}                    # the tail


@pytest.mark.parametrize("F", [8, 9, 17, 64])
def test_edge_matrix_has_the_ties_and_zeros_it_promises(F):
    M = ei.edge_features(300, F, np.float64, F)
    rows = np.arange(300)
    tied = M[(rows % 4 == 1) & np.all(np.isfinite(M), axis=1)]
    assert 70 <= tied.shape[0] <= 75                                              # a quarter of the rows
    assert np.array_equal(tied, np.round(tied, 1))
    s = np.sort(tied, axis=1)
    at_median = (s[:, F // 2] == s[:, F // 2 - 1]) | (s[:, F // 2] == s[:, min(F // 2 + 1, F - 1)])
    assert at_median.mean() > 0.2                                                 # ties AT the selected rank
    z = M[rows % 16 == 2]
    assert (z[:, 0] == 0).all() and np.signbit(z[:, 0]).all() and (z[:, F - 1] == 0).all() and not np.signbit(z[:, F - 1]).any()
    assert np.isnan(M[100, F - 1]) and np.isposinf(M[299, 0])


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("F", [9, 17, 33])
def test_negative_matrix_puts_negatives_where_the_counts_see_them(F, dtype):
    M = ei.negative_features(300, F, dtype, 7 + F)
    v = np.all(np.isfinite(M), axis=1)
    share = np.any(M[v] < 0, axis=1).mean()
    assert 0.28 < share < 0.38                                                    # about a third of the valid rows
    assert (M[~v] < 0).any(axis=1).all()                                          # rows that must NOT be counted
    for method in ei.EXACT_METHODS:
        r = tr.metagene(M, method)
        assert r["n_negative"] == int(np.any(M[v] < 0, axis=1).sum()) > 90
        assert r["n_below"] > int((r["score"][v] == 0).sum()) and (r["score"][v] < 0).sum() >= 30
        assert r["min"] < -2.0 and r["n_below"] == int((r["score"][v] < dtype(1e-6)).sum())
    assert tr.metagene(M, "minimum")["mean"] < 0


@pytest.mark.parametrize("dtype", TYPES)
def test_invalid_blocks_are_invalid(dtype):
    M = ei.invalid_block_features(dtype)
    v = np.all(np.isfinite(M), axis=1)
    assert M.shape[0] == 4097 and not v[2048:4096].any() and v[4096] and v[:2048].sum() == 2047
    bad = M[2048:4096]
    assert np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any()
    assert (np.isfinite(bad).sum(axis=1) == M.shape[1] - 1).all()                 # one bad cell per row, in turning columns
    r = tr.metagene(M, "minimum")
    assert r["n_valid"] == 2048 and r["n_negative"] == 0
    A = ei.all_invalid_features(dtype)
    r = tr.metagene(A, "arithmetic_mean")
    assert not r["valid"].any() and np.isnan(r["score"]).all()
    assert (r["min"], r["max"]) == (np.inf, -np.inf) and np.isnan(r["mean"])
    assert (r["n_valid"], r["n_below"], r["n_negative"]) == (0, 0, 0)


# ---- KS ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
def test_key_scores_hold_every_kind_of_key(dtype):
    x = ei.ks_key_scores(dtype)
    fi = np.finfo(dtype)
    assert x.dtype == dtype and 2900 < x.size < 3100 and np.isfinite(x).all()
    assert (x < 0).sum() > 1000 and (x > 0).sum() > 1000
    zero = x == 0
    assert (zero & np.signbit(x)).sum() >= 20 and (zero & ~np.signbit(x)).sum() >= 20   # (rounding adds a few)
    sub = (x != 0) & (np.abs(x) < fi.tiny)
    assert (sub & (x < 0)).sum() == 60 and (sub & (x > 0)).sum() == 60
    assert x.max() == fi.max and x.min() == -fi.max
    values, counts = np.unique(x, return_counts=True)
    assert counts.max() >= 20 and (counts >= 5).sum() >= 30                      # runs of equal values
    x64 = ei.ks_key_scores(np.float64)
    near = np.sort(x64)
    gaps = np.diff(near)
    close = (gaps > 0) & (gaps < 2.0 ** -45 * np.abs(near[1:])) & (np.abs(near[1:]) > 1e-3)
    assert close.sum() >= 100                                                     # neighbours a few fp64 ulps apart ...
    if dtype == np.float32:                                                       # ... that float32 makes one key
        assert np.unique(x).size < np.unique(x64).size - 100
    s = np.sort(x.astype(np.float64))
    assert np.array_equal(np.sort(ei.ks_key_scores(dtype, extremes=False).astype(np.float64)), s[1:-1])


@pytest.mark.parametrize("dtype", TYPES)
def test_key_scores_keep_the_argmax_apart(dtype):
    """ks_gap: the two largest D at distinct scores differ by more than the tolerance of D (mixed-sign input without
    the two extremes, whose squares are not finite in fp64)."""
    x = ei.ks_key_scores(dtype, extremes=False)
    gap, tol, p = ei.ks_gap(x, 0.5)
    print(f"{x.dtype}: argmax {p['argmax']}, D {p['D']:.6g}, gap {gap:.3g}, tolerance {tol:.3g}")
    assert gap > tol and gap > 1e-12
    assert p["sorted"][p["argmax"]] < 0                                           # D peaks among the negative keys
    with np.errstate(over="ignore", invalid="ignore"):
        _, mean, sd = tr.ks_background(ei.ks_key_scores(np.float64), 0.5)
    assert np.isfinite(mean) and np.isposinf(sd)                                  # why the argmax leaves the extremes out


def test_background_counts():
    for n, q, m in ei.BACKGROUND_CASES:
        assert ei.background_count(n, q) == m
        x = ei.background_scores(n, np.float64)
        s, mean, sd = tr.ks_background(x, q)
        assert mean == float(tr.block_sum(s[:m])) / m
        assert abs(mean - s[:m].mean()) < 1e-12 and abs(sd - s[:m].std()) < 1e-12
        assert (s[:m] < 0).any() and (x > 0).any()
    assert [m for _, _, m in ei.BACKGROUND_CASES[:3]] == [tr.BLK - 1, tr.BLK, tr.BLK + 1]


def test_rank_requests_and_classify_inputs():
    r = ei.rank_requests(3000)
    assert r.size == 64 and r[0] == 0 and r[1] == 2999 and r[2] == r[3] and r.min() >= 0 and r.max() < 3000
    for dtype in TYPES:
        for n in (255, 256, 257, 4097):
            x, thr = ei.classify_scores(n, dtype)
            assert (x.astype(np.float64) == thr).sum() >= 5 and thr < 0 and (x < 0).sum() > n // 3
            lab = tr.RestatedContext().ks_classify(x, thr, float(x.max()))[1]
            assert lab.sum() == (x >= dtype(thr)).sum() and 0 < lab.sum() < n


# ---- GMM ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ei.GMM_CASES))
def test_gmm_input_passes_the_generators_guards(name):
    c = ei.gmm_case(name)
    _, K, n_init, seed, max_iter, dtype = ei.GMM_CASES[name]
    want = c["want"]
    assert c["x"].dtype == dtype and want["km_labels"].shape == (n_init, c["x"].size)
    assert np.array_equal(want["km_labels"], ei.sklearn_kmeans_labels(c["x"], K, n_init, seed))
    assert all((np.bincount(lab, minlength=K) > 0).all() for lab in want["km_labels"])
    margin = ei.change_margin(want)
    print(f"{name}: n_iter {want['n_iter'].tolist()}, converged {want['converged'].astype(int).tolist()}, "
          f"change margin {margin:.3g}, best {want['best']}")
    assert margin > 1e-9
    for t in range(ei.N_PERTURB):
        with tr.perturbed(np.random.default_rng(500 + t)):
            g = tr.gmm_fit(c["x"], K, c["draws"], max_iter=max_iter, km_labels=want["km_labels"])
        assert np.array_equal(g["n_iter"], want["n_iter"]) and np.array_equal(g["converged"], want["converged"])
    assert np.isfinite(want["lower_bound"]).all()


def test_gmm_inputs_pin_what_they_are_named_for():
    w = ei.gmm_case("k8_mixed_stop_f64")["want"]
    assert (w["n_iter"] == 6).all() and w["converged"].sum() == 5                 # five stop converged, five do not
    assert np.array_equal(ei.gmm_case("k8_mixed_stop_f32")["want"]["converged"], w["converged"])
    for name, n in (("k8_block_2048", tr.BLK), ("k8_block_2049", tr.BLK + 1)):
        assert ei.gmm_case(name)["x"].size == n and ei.gmm_case(name)["want"]["converged"].all()
    w = ei.gmm_case("k8_three_groups")["want"]
    assert w["n_iter"].tolist() == [7, 7, 6] and ei.gmm_case("k8_three_groups")["x"].size == 2 * tr.BLK + 1
    assert ei.gmm_case("k5_one_run")["want"]["lower_bound"].shape == (1,)
    c = ei.gmm_case("k4_many_runs")
    groups = ei.equal_label_groups(c["want"]["km_labels"])
    assert c["n_init"] == 33 and len(groups) >= 3
    for g in groups:                                                              # equal labels: equal to the last bit
        for k in ("weights", "means", "variances", "lower_bound", "n_iter", "converged"):
            assert all(c["want"][k][r].tobytes() == c["want"][k][g[0]].tobytes() for r in g), k
    best = [g for g in groups if c["want"]["best"] in g]
    assert best and c["want"]["best"] == best[0][0]                               # the first of equal runs wins
    for name in ("zero_inflated_k3", "zero_inflated_k8_f32"):
        var = ei.gmm_case(name)["want"]["variances"]
        assert ((var == ei.REG_COVAR).sum(axis=1) == 1).all()                     # one collapsed component in every run


@pytest.mark.parametrize("dtype", TYPES)
def test_without_reg_covar_the_zero_inflated_fit_ends_unconverged(dtype):
    """K = 8, max_iter = 5: every run's lower bound is NaN, with and without the one-ulp perturbations.  (K = 3 is no
    fair input at 5 iterations: there the variance reaches 0 in iteration 5 or 6 according to which responsibilities
    underflow, and the perturbations move that.)"""
    x = ei.zero_inflated(3000, 9).astype(dtype)
    draws = ei.kmeans_draws(9, 10, 8)
    with np.errstate(all="ignore"):
        f = tr.gmm_fit(x, 8, draws, max_iter=5, reg=0.0)
        fits = [f]
        for t in range(ei.N_PERTURB):
            with tr.perturbed(np.random.default_rng(500 + t)):
                fits.append(tr.gmm_fit(x, 8, draws, max_iter=5, reg=0.0, km_labels=f["km_labels"]))
    for g in fits:
        assert not np.isfinite(g["lower_bound"]).any() and not g["converged"].any() and (g["n_iter"] == 5).all()
        assert g["best"] == 0      # sklearn's rule too: the first run is taken while the maximum is -inf; nothing exceeds NaN


# ---- posteriors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257])
def test_k8_posterior_leaves_no_cell_undecided(n):
    x, w, mu, var, high = ei.k8_posterior_setup()
    assert len(high) == 7 and int(np.argmin(mu)) not in high and np.all(np.diff(mu[high]) > 0)
    base = tr.gmm_posterior(x[:n], w, mu, var, high, 0.3)
    tol = 16 * ei.spread(lambda: [tr.gmm_posterior(x[:n], w, mu, var, high, 0.3)[0]], [base[0]])[0]
    undecided = int((np.abs(base[0] - 0.3) <= tol).sum())
    print(f"n={n}: tolerance {tol:.3g}, undecided {undecided}, high {int(base[1].sum())}")
    assert tol > 0 and undecided <= 0.001 * n and 0 < base[1].sum() < n


def test_k8_posterior_orders_and_far_scores():
    x, w, mu, var, high = ei.k8_posterior_setup()
    a = tr.gmm_posterior(x[:300], w, mu, var, high, 0.3)[0]
    b = tr.gmm_posterior(x[:300], w, mu, var, high[::-1], 0.3)[0]
    assert (a != b).sum() >= 10 and np.max(np.abs(a - b)) < 1e-15                 # the order of the additions shows
    far = ei.far_scores(mu, var)
    wl = np.sort(tr.weighted_log_prob(far, w, mu, var), axis=1)
    assert (wl[:, -1] - wl[:, -2] > ei.EXP_UNDERFLOW + 100).all() and np.isfinite(tr.log_sum_exp(wl)).all()
    R = ei.responsibilities(far, w, mu, var)
    assert np.isin(R, (0.0, 1.0)).all() and (R.sum(axis=1) == 1).all()
    assert (np.abs(far[:, None] - mu[None, :]).min(axis=1) > 40 * np.sqrt(var.max())).all()
    one = tr.gmm_posterior(x[:257], [1.0], [0.5], [2.0], [0], 0.3)                # K = 1
    assert (one[0] == 1.0).all() and one[1].all()


# ---- the public function -------------------------------------------------------------------------------------------------
def test_public_inputs_run_on_the_restatement(monkeypatch):
    from spatialcore_amd import _lib
    from spatialcore_amd.stats import classify_by_threshold

    monkeypatch.setattr(_lib, "default_context", lambda device=0: tr.RestatedContext())
    M = ei.public_ks_matrix()
    assert M.dtype == np.float32 and M.shape[1] == 17 and (M < 0).any(axis=1).mean() > 0.6
    a = adata_of(M)
    classify_by_threshold(a, list(a.var_names), metagene_method="arithmetic_mean", threshold_method="ks", plot=False)
    hi = a.obs["threshold_cluster"].to_numpy() == 1
    assert 0 < hi.sum() < 0.4 * 600 and (a.obs["threshold_score"].to_numpy() < 0).sum() > 100
    prm = a.uns["threshold_params"]
    assert prm["background_mean"] < 0 < prm["threshold"]       # (the reference's 90th-percentile fallback, in float32)
    M = ei.public_gmm_matrix()
    assert M.dtype == np.float64 and M.shape[1] == 33
    b = adata_of(M)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        classify_by_threshold(b, list(b.var_names), metagene_method="median", threshold_method="gmm", n_components=4,
                              plot=False)
    prm = b.uns["threshold_params"]
    assert prm["n_components"] == 4 and len(prm["gmm_means"]) == 4 and prm["gmm_converged"]
    assert 0.6 < (b.obs["threshold_cluster"].to_numpy() == 1).mean() < 0.9        # every level but the lowest
