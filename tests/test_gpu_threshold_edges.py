"""GPU tests of sc_threshold.hip at the edges of its own constants, against the numpy restatement
(tests/threshold_restated.py) on the inputs of tests/threshold_edge_inputs.py; tests/test_cpu_threshold_edges.py shows
that each input is a fair test.

Contract, as tests/test_gpu_threshold.py: bit for bit wherever no exp / log / erf / erfc enters; 16 x
the restatement's own one-ulp spread where one does.  Two floors follow from a final rounding that the ulp model cannot
see: 2^-52 on the KS deviation D (a difference of two numbers <= 1), and one float32 ulp of the score on float32
geometric means (the fp64 value is rounded to float32 once: a last-place difference in fp64 can cross that boundary
although the measured spread is 0).  "Bit for bit" compares values: the sign of a zero is not part of the contract
(numpy's own sort and minimum do not fix it).  Every toleranced assertion prints its deviation and its tolerance."""
import warnings

import numpy as np
import pytest

import threshold_edge_inputs as ei
import threshold_restated as tr
from test_cpu_threshold import adata_of
from test_gpu_threshold import _assert_fit, _ctx, _draws, _fit_both
from threshold_edge_inputs import spread

pytestmark = pytest.mark.gpu

TYPES = [np.float32, np.float64]


# ---- metagene ----------------------------------------------------------------------------------------------------------
def _check_metagene(M, methods=tr.METHODS, what=""):
    """One sc_metagene_score call per method against the restatement, and the statistics against the device's own scores."""
    ctx = _ctx()
    for method in methods:
        got, want = ctx.metagene_score(M, method, 0.1), tr.metagene(M, method, 0.1)
        v = want["valid"]
        assert got["score"].dtype == M.dtype
        assert np.array_equal(got["valid"], v) and np.isnan(got["score"][~v]).all(), (what, method)
        for k in ("n_valid", "n_negative"):
            assert got[k] == want[k], (what, method, k)
        mn, mx, mean = ei.stats_of_scores(got["score"], got["valid"])            # exact functions of the scores written
        assert (got["min"], got["max"]) == (mn, mx), (what, method)
        assert got["mean"] == mean or (np.isnan(mean) and np.isnan(got["mean"])), (what, method)
        assert got["n_below"] == int((got["score"][v] < M.dtype.type(1e-6)).sum()), (what, method)
        if method in ei.EXACT_METHODS:
            assert np.array_equal(got["score"][v], want["score"][v]), (what, method)
            assert got["n_below"] == want["n_below"], (what, method)
            assert (got["min"], got["max"]) == (want["min"], want["max"]), (what, method)
            assert got["mean"] == want["mean"] or (np.isnan(want["mean"]) and np.isnan(got["mean"])), (what, method)
        elif v.any():
            base = want["score"][v].astype(float)
            tol = 16 * spread(lambda: [tr.metagene(M, method, 0.1)["score"][v]], [base])[0]
            floor = np.spacing(np.abs(want["score"][v])).astype(float) if M.dtype == np.float32 else 0.0
            d = np.abs(got["score"][v].astype(float) - base)
            print(f"{what} {method} {M.dtype}: score dev {d.max():.3g} (16 x spread {tol:.3g}, float32 ulp {np.max(floor):.3g})")
            assert np.all(d <= tol + floor), (what, method)
    return got


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("F", ei.FEATURE_COUNTS)
def test_metagene_at_every_shape_of_the_row_sum(F, dtype):
    """F below, at and above 8 and 16, with and without a tail, up to TH_FMAX; ties and signed zeros in the rows."""
    _check_metagene(ei.edge_features(300, F, dtype, F), what=f"F={F}")


@pytest.mark.parametrize("dtype", TYPES)
def test_metagene_f17_across_workgroups(dtype):
    _check_metagene(ei.edge_features(4097, 17, dtype, 4097), what="n=4097 F=17")


def test_metagene_refuses_65_features_and_takes_64():
    with pytest.raises(ValueError, match="need 1 <= n_features <= 64, got 65"):
        _ctx().metagene_score(np.ones((10, 65)), "median")
    got = _ctx().metagene_score(np.arange(640.0).reshape(10, 64), "median")
    assert np.array_equal(got["score"], np.median(np.arange(640.0).reshape(10, 64), axis=1))


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("F", [9, 17, 33])
def test_metagene_negative_features(F, dtype):
    """n_negative, n_below and negative min / mean: a third of the rows hold a negative value."""
    M = ei.negative_features(300, F, dtype, 7 + F)
    got = _check_metagene(M, methods=ei.EXACT_METHODS, what=f"negative F={F}")
    assert got["n_negative"] > 90 and got["min"] < -2.0 and got["mean"] < 0     # (the last method: minimum)


@pytest.mark.parametrize("dtype", TYPES)
def test_metagene_workgroup_without_a_valid_row(dtype):
    """n = 4097: the second workgroup's partial is (0, +inf, -inf); the third holds one row."""
    M = ei.invalid_block_features(dtype)
    got = _check_metagene(M, what="invalid block")
    assert got["n_valid"] == 2048 and not got["valid"][2048:4096].any() and got["valid"][4096]


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n", [2048, 2049])
def test_metagene_at_the_workgroup_edge(n, dtype):
    _check_metagene(ei.edge_features(n, 3, dtype, n), what=f"n={n}")


@pytest.mark.parametrize("dtype", TYPES)
def test_metagene_without_any_valid_row(dtype):
    M = ei.all_invalid_features(dtype)
    for method in tr.METHODS:
        got = _ctx().metagene_score(M, method, 0.1)
        assert not got["valid"].any() and np.isnan(got["score"]).all(), method
        assert (got["min"], got["max"]) == (np.inf, -np.inf) and np.isnan(got["mean"]), method
        assert (got["n_valid"], got["n_below"], got["n_negative"]) == (0, 0, 0), method
    _check_metagene(M, what="all invalid")


# ---- KS ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
def test_ks_sort_of_mixed_keys(dtype):
    """Both branches of ordered_bits: signs, zeros of both signs, subnormals, the largest finite values, runs of equal keys."""
    x = ei.ks_key_scores(dtype)
    ranks = ei.rank_requests(x.size)
    with np.errstate(over="ignore", invalid="ignore"):           # float64: the square of the largest value is +inf
        s, mean, sd = tr.ks_background(x, 0.5)
    prep = _ctx().ks_prepare(x, 0.5, ranks=ranks, return_sorted=True)
    assert np.array_equal(prep["sorted"], s)
    zeros = prep["sorted"] == 0
    assert zeros.sum() >= 40 and (np.diff(np.signbit(prep["sorted"][zeros]).astype(int)) <= 0).all()   # -0.0 sorts before +0.0
    assert np.array_equal(prep["order"], s[ranks])               # 64 order statistics, with repeats and both ends
    assert prep["bg_mean"] == mean and prep["bg_std"] == sd and (np.isfinite(sd) or dtype == np.float64)
    none = _ctx().ks_prepare(x, 0.5)                             # n_ranks = 0
    assert none["order"].size == 0 and none["sorted"] is None and (none["bg_mean"], none["bg_std"]) == (mean, sd)


@pytest.mark.parametrize("dtype", TYPES)
def test_ks_argmax_of_mixed_keys(dtype):
    """The existing rule on the mixed-sign input (without the two extremes: their squares overflow the fp64 moments)."""
    x = ei.ks_key_scores(dtype, extremes=False)
    gap, tol_D, p = ei.ks_gap(x, 0.5)
    ctx = _ctx()
    prep = ctx.ks_prepare(x, 0.5, return_sorted=True)
    assert np.array_equal(prep["sorted"], p["sorted"])
    assert (prep["bg_mean"], prep["bg_std"]) == (p["background_mean"], p["background_std"])
    i, score, D = ctx.ks_argmax(prep["bg_mean"], prep["bg_std"])
    print(f"{x.dtype}: argmax {i} (restated {p['argmax']}), D dev {abs(D - p['D']):.3g} (tolerance {tol_D:.3g}), gap {gap:.3g}")
    assert gap > tol_D
    assert i == p["argmax"] and score == p["sorted"][i] and score < 0 and abs(D - p["D"]) <= tol_D


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n,q,m", ei.BACKGROUND_CASES)
def test_ks_background_count(n, q, m, dtype):
    """m = 2047, 2048, 2049: k_th_sum ends inside a workgroup, at its end, one point into the next; n = 10: m = n."""
    assert ei.background_count(n, q) == m
    x = ei.background_scores(n, dtype)
    s, mean, sd = tr.ks_background(x, q)
    prep = _ctx().ks_prepare(x, q, ranks=[0, n - 1], return_sorted=True)
    assert np.array_equal(prep["sorted"], s) and np.array_equal(prep["order"], s[[0, n - 1]])
    assert (prep["bg_mean"], prep["bg_std"]) == (mean, sd)


def test_ks_prepare_refusals():
    ctx = _ctx()
    x = ei.background_scores(100, np.float64)
    with pytest.raises(ValueError, match="at most 64 order statistics"):
        ctx.ks_prepare(x, 0.5, ranks=np.zeros(65, dtype=np.int64))
    with pytest.raises(ValueError, match=r"rank 100 outside \[0, n\)"):
        ctx.ks_prepare(x, 0.5, ranks=[0, 100])
    with pytest.raises(ValueError, match=r"rank -1 outside \[0, n\)"):
        ctx.ks_prepare(x, 0.5, ranks=[-1])
    with pytest.raises(ValueError, match="need 10 <= n <= 2\\^31 - 1, got 9"):
        ctx.ks_prepare(x[:9], 0.5)
    for q in (0.0, 1.0):
        with pytest.raises(ValueError, match=r"background_quantile must be in \(0, 1\)"):
            ctx.ks_prepare(x, q)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n", [255, 256, 257, 4097])
def test_ks_classify_at_tile_edges(n, dtype):
    """A threshold that several (negative) scores equal: labels use >=; n_high adds up across workgroups."""
    x, thr = ei.classify_scores(n, dtype)
    top = float(x.max())
    dev, lab, n_high = _ctx().ks_classify(x, thr, top)
    w_dev, w_lab, w_high = tr.RestatedContext().ks_classify(x, thr, top)
    assert np.array_equal(dev, w_dev) and np.array_equal(lab, w_lab) and n_high == w_high == int(lab.sum())
    at = x.astype(np.float64) == thr
    assert at.sum() >= 5 and lab[at].all() and (dev[at] == 0).all() and not lab[x.astype(np.float64) < thr].any()


# ---- GMM ---------------------------------------------------------------------------------------------------------------
def _fit_case(name):
    _, K, n_init, seed, max_iter, dtype = ei.GMM_CASES[name]
    c = ei.gmm_case(name)
    got, want, draws = _fit_both(c["x"], K, seed, max_iter=max_iter, n_init=n_init)
    assert np.array_equal(draws, c["draws"])
    for k in ("km_labels", "n_iter", "converged", "lower_bound"):                # the shared restated fit is this one
        assert np.array_equal(want[k], c["want"][k]), k
    _assert_fit(got, want, c["x"], K, draws, max_iter=max_iter, what=name)
    return got, want


@pytest.mark.parametrize("name", ["k8_mixed_stop_f64", "k8_mixed_stop_f32"])
def test_gmm_k8_runs_stop_converged_and_unconverged_together(name):
    """GMM_KMAX components (33 partials, a full sp[5][8]); at max_iter = 6 five runs converge and five do not."""
    got, want = _fit_case(name)
    assert (got["n_iter"] == 6).all() and got["converged"].sum() == 5 and want["converged"].sum() == 5


@pytest.mark.parametrize("name", ["k8_block_2048", "k8_block_2049"])
def test_gmm_k8_at_the_workgroup_edge(name):
    _fit_case(name)


def test_gmm_k8_finished_runs_are_skipped():
    """Three runs over three workgroups that stop after 7, 7 and 6 iterations: k_gmm_pass and k_gmm_stage2 pass over the
    finished run, whose parameters must stay those of its own last M-step."""
    got, want = _fit_case("k8_three_groups")
    assert want["n_iter"].tolist() == [7, 7, 6] and len(set(want["n_iter"].tolist())) > 1


def test_gmm_one_run():
    got, want = _fit_case("k5_one_run")
    assert got["best"] == 0 and got["lower_bound"].shape == (1,)


def test_gmm_33_runs_equal_labels_give_equal_runs():
    """More runs than the package ever asks for.  Runs with identical k-means labels are identical in every output, to
    the last bit, and the best run is the first of its group."""
    got, want = _fit_case("k4_many_runs")
    groups = ei.equal_label_groups(got["km_labels"])
    assert len(groups) >= 3
    for g in groups:
        for k in ("weights", "means", "variances", "lower_bound", "n_iter", "converged"):
            assert all(got[k][r].tobytes() == got[k][g[0]].tobytes() for r in g), (k, g)
    first = {r: g[0] for g in groups for r in g}
    assert any(want["best"] in g for g in groups)
    assert got["best"] == first.get(got["best"], got["best"])


@pytest.mark.parametrize("name", ["zero_inflated_k3", "zero_inflated_k8_f32"])
def test_gmm_zero_inflated_component_collapses_to_reg_covar(name):
    got, want = _fit_case(name)
    collapsed = want["variances"] == ei.REG_COVAR
    assert (collapsed.sum(axis=1) == 1).all()
    assert np.array_equal(got["variances"] == ei.REG_COVAR, collapsed)
    assert (got["means"][collapsed] == 0).all()


@pytest.mark.parametrize("dtype", TYPES)
def test_gmm_without_reg_covar_ends_unconverged(dtype):
    """reg_covar = 0 (legal through the ABI), K = 8: the variance of the component at zero reaches 0 within five
    iterations, the lower bound is NaN from then on and |NaN| < tol is false: every run stops at max_iter, unconverged,
    and the first run stays the best (sklearn's rule as well: it takes the first run while its maximum is -inf, and
    nothing exceeds NaN).  The CPU file shows that the one-ulp perturbations do not move this outcome."""
    K = 8
    x = ei.zero_inflated(3000, 9).astype(dtype)
    X = x.reshape(-1, 1)
    draws = _draws(9, K)
    with np.errstate(all="ignore"):
        want = tr.gmm_fit(x, K, draws, max_iter=5, reg=0.0)
    got = _ctx().gmm_fit(x, K, 10, 300, float(np.mean(np.var(X, axis=0)) * 1e-4), X.mean(axis=0), draws, 5, 1e-3, 0.0,
                         return_km_labels=True)
    assert np.array_equal(got["km_labels"], want["km_labels"])
    assert not np.isfinite(want["lower_bound"]).any() and not np.isfinite(got["lower_bound"]).any()
    assert not got["converged"].any() and (got["n_iter"] == 5).all()
    assert got["best"] == want["best"] == 0


def test_gmm_fit_refusals():
    ctx = _ctx()
    x = ei.mixture(300, 3, 1)

    def fit(x=x, K=3, n_init=10, max_iter=100, tol=1e-3, reg=1e-6, draws=None):
        draws = _draws(0, K, max(n_init, 1)) if draws is None else draws
        return ctx.gmm_fit(x, K, n_init, 300, 1e-4, [x.mean()], draws, max_iter, tol, reg)

    with pytest.raises(ValueError, match=r"need 2 <= K <= min\(8, n\) \(K = 9, n = 300\)"):
        fit(K=9)
    with pytest.raises(ValueError, match=r"need 2 <= K <= min\(8, n\) \(K = 4, n = 3\)"):
        fit(x=x[:3], K=4)
    with pytest.raises(ValueError, match="need 1 <= n_init <= 1024"):
        fit(n_init=0, draws=np.zeros(0))
    with pytest.raises(ValueError, match="need 1 <= n_init <= 1024"):
        fit(n_init=1025)
    with pytest.raises(ValueError, match="max_iter >= 1"):
        fit(max_iter=0)
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError, match="km_tol, tol and reg_covar must be finite and >= 0"):
            fit(tol=bad)
        with pytest.raises(ValueError, match="km_tol, tol and reg_covar must be finite and >= 0"):
            fit(reg=bad)
    assert np.isfinite(fit()["lower_bound"]).all()               # the context is as usable as before


# ---- posteriors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n", [255, 256, 257])
def test_posterior_of_one_component_is_one(n, dtype):
    x = ei.mixture(n, 3, n).astype(dtype)
    prob, lab, n_high = _ctx().gmm_posterior(x, [1.0], [0.5], [2.0], [0], 0.3)
    assert (prob == 1.0).all() and lab.all() and n_high == n
    prob, lab, n_high = _ctx().gmm_posterior(x, [0.25], [0.5], [2.0], [0], 0.999)      # (weights need not add up to 1)
    assert (prob == 1.0).all() and lab.all() and n_high == n


@pytest.mark.parametrize("n", [255, 256, 257])
def test_posterior_k8_seven_high_components(n):
    x, w, mu, var, high = ei.k8_posterior_setup()
    x = x[:n]
    base = tr.gmm_posterior(x, w, mu, var, high, 0.3)
    tol = 16 * spread(lambda: [tr.gmm_posterior(x, w, mu, var, high, 0.3)[0]], [base[0]])[0]
    prob, lab, n_high = _ctx().gmm_posterior(x, w, mu, var, high, 0.3)
    d = float(np.max(np.abs(prob - base[0])))
    decided = np.abs(base[0] - 0.3) > tol
    print(f"n={n}: P(high) dev {d:.3g} (tolerance {tol:.3g}), undecided {int((~decided).sum())}")
    assert d <= tol and (~decided).sum() <= 0.001 * n
    assert np.array_equal(lab[decided], base[1][decided]) and n_high == int(lab.sum())
    assert np.array_equal(lab, (prob > 0.3).astype(np.int32))


def test_posterior_adds_the_components_in_the_given_order():
    x, w, mu, var, high = ei.k8_posterior_setup()
    x = x[:300]
    ctx = _ctx()
    orders = (high, high[::-1])
    base = [tr.gmm_posterior(x, w, mu, var, o, 0.3)[0] for o in orders]
    assert (base[0] != base[1]).sum() >= 10
    got = [ctx.gmm_posterior(x, w, mu, var, o, 0.3)[0] for o in orders]
    for o, g, b in zip(("ascending", "descending"), got, base):
        tol = 16 * spread(lambda: [tr.gmm_posterior(x, w, mu, var, orders[0] if o == "ascending" else orders[1], 0.3)[0]], [b])[0]
        print(f"{o}: P(high) dev {np.max(np.abs(g - b)):.3g} (tolerance {tol:.3g})")
        assert np.max(np.abs(g - b)) <= tol
    # responsibilities that are exact (0 or 1) leave the order of the additions as the only difference: compare both
    # orders on the far scores, where the device owes the restatement's bits
    far = ei.far_scores(mu, var)
    for o in orders:
        assert np.array_equal(ctx.gmm_posterior(far, w, mu, var, o, 0.3)[0], tr.gmm_posterior(far, w, mu, var, o, 0.3)[0])


@pytest.mark.parametrize("dtype", TYPES)
def test_posterior_of_far_scores_is_exact(dtype):
    """Scores so far out that every responsibility but one underflows: each is exactly 0 or 1, they add up to 1, and
    the log-sum-exp behind them stayed finite (a non-finite one would make them NaN)."""
    _, w, mu, var, _ = ei.k8_posterior_setup()
    far = ei.far_scores(mu, var).astype(dtype)
    ctx = _ctx()
    want = ei.responsibilities(far, w, mu, var)
    got = np.stack([ctx.gmm_posterior(far, w, mu, var, [k], 0.5)[0] for k in range(8)], axis=1)
    assert np.isin(want, (0.0, 1.0)).all() and np.array_equal(got, want) and (got.sum(axis=1) == 1).all()
    prob, lab, n_high = ctx.gmm_posterior(far, w, mu, var, list(range(8)), 0.5)
    assert (prob == 1.0).all() and n_high == far.size


def test_posterior_refusals():
    x, w, mu, var, high = ei.k8_posterior_setup()
    ctx = _ctx()
    with pytest.raises(ValueError, match="need 1 <= n_high <= K, got 0"):
        ctx.gmm_posterior(x[:10], w, mu, var, [], 0.3)
    with pytest.raises(ValueError, match="need 1 <= n_high <= K, got 3"):
        ctx.gmm_posterior(x[:10], w[:2] / w[:2].sum(), mu[:2], var[:2], [0, 1, 1], 0.3)
    with pytest.raises(ValueError, match="need 1 <= K <= 8, got 9"):
        ctx.gmm_posterior(x[:10], np.full(9, 1 / 9), np.arange(9.0), np.ones(9), [1], 0.3)


# ---- the public function -------------------------------------------------------------------------------------------------
def _both_calls(monkeypatch, M, **kw):
    from spatialcore_amd import _lib
    from spatialcore_amd.stats import classify_by_threshold

    dev, twin = adata_of(M), adata_of(M)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        classify_by_threshold(dev, list(dev.var_names), plot=False, **kw)
        monkeypatch.setattr(_lib, "default_context", lambda device=0: tr.RestatedContext())
        classify_by_threshold(twin, list(twin.var_names), plot=False, **kw)
        monkeypatch.undo()
    return dev, twin


def test_classify_by_threshold_17_markers_with_negative_values(monkeypatch):
    """arithmetic_mean + KS on float32: sums, sqrt, divide and erfc's argmax only -- every column bit for bit."""
    dev, twin = _both_calls(monkeypatch, ei.public_ks_matrix(), metagene_method="arithmetic_mean", threshold_method="ks")
    for col in ("threshold_score", "threshold_probability", "threshold_cluster"):
        assert np.array_equal(dev.obs[col].to_numpy(), twin.obs[col].to_numpy()), col
    a, b = dev.uns["threshold_params"], twin.uns["threshold_params"]
    for k in ("threshold", "background_mean", "background_std", "n_high", "n_low", "n_invalid"):
        assert a[k] == b[k], k
    assert (dev.obs["threshold_score"].to_numpy() < 0).sum() > 100 and 0 < a["n_high"] < 240


def test_classify_by_threshold_33_markers_four_components(monkeypatch):
    """median + GMM with n_components = 4, which the Python layer accepts: the scores bit for bit; P(high), the fitted
    parameters and the threshold within 16 x the spread of the restated chain; labels wherever P is decided."""
    M = ei.public_gmm_matrix()
    kw = dict(metagene_method="median", threshold_method="gmm", n_components=4)
    dev, twin = _both_calls(monkeypatch, M, **kw)
    assert np.array_equal(dev.obs["threshold_score"].to_numpy(), twin.obs["threshold_score"].to_numpy())
    c = ei.gmm_case("public_k4")
    assert np.array_equal(c["x"], twin.obs["threshold_score"].to_numpy())

    def chain():
        f = tr.gmm_fit(c["x"], 4, c["draws"], km_labels=c["want"]["km_labels"])
        b = f["best"]
        w, mu, var = f["weights"][b], f["means"][b], f["variances"][b]
        thr, high, _ = tr.gmm_threshold(w, mu, var, 4)
        return [tr.gmm_posterior(c["x"], w, mu, var, high, 0.3)[0], np.array(thr), tr.sorted_parameters(w, mu, var)]

    base = chain()
    assert np.array_equal(base[0], twin.obs["threshold_probability"].to_numpy())
    tol = [16 * t for t in spread(chain, base)]
    a, b = dev.uns["threshold_params"], twin.uns["threshold_params"]
    got_par = tr.sorted_parameters(a["gmm_weights"], a["gmm_means"], np.square(a["gmm_stds"]))
    tol_par = tol[2] + 4 * np.finfo(float).eps * base[2].max()                  # (params hold stds: squared again)
    d = float(np.max(np.abs(dev.obs["threshold_probability"].to_numpy() - base[0])))
    print(f"P(high) dev {d:.3g} (tolerance {tol[0]:.3g}), parameters dev {np.max(np.abs(got_par - base[2])):.3g} "
          f"(tolerance {tol_par:.3g}), threshold dev {abs(a['threshold'] - float(base[1])):.3g}")
    assert d <= tol[0] and np.max(np.abs(got_par - base[2])) <= tol_par
    lowest = np.sort(a["gmm_means"])[:2]                                         # K >= 3: an exact function of the means
    assert a["threshold"] == float((lowest[0] + lowest[1]) / 2) and float(base[1]) == b["threshold"]
    assert a["n_components"] == 4 and a["gmm_n_iter"] == b["gmm_n_iter"] and a["gmm_converged"] and b["gmm_converged"]
    decided = np.abs(base[0] - 0.3) > tol[0]
    assert (~decided).sum() <= 0.001 * c["x"].size
    assert np.array_equal(dev.obs["threshold_cluster"].to_numpy()[decided], twin.obs["threshold_cluster"].to_numpy()[decided])
    assert abs(a["n_high"] - b["n_high"]) <= (~decided).sum()
