"""GPU tests of classify_by_threshold and the entry points under it (sc_metagene_score, sc_ks_*, sc_gmm_*) against
the numpy restatement of the kernels (tests/threshold_restated.py) and the reference's recorded results
(tests/golden/ref_threshold.npz).

Contract.  Bit for bit against the restatement: the mask, minimum / median / arithmetic_mean scores,
the sort, the background moments, the k-means labels of every run, n_iter and every integer count.  Where exp / log /
erf / erfc enter, the device may differ from the restatement by 16 x the spread the restatement itself shows when
every result of those functions is moved by one random ulp (measured here on the test's own input, or read from the
golden file for the golden inputs); against the reference by 4 x the restatement-against-reference deviation the
generator recorded.  Labels must agree wherever the recorded margin exceeds that tolerance."""
import warnings

import numpy as np
import pytest

import threshold_restated as tr
from conftest import load_golden, make_adata, synth
from test_cpu_threshold import CASES, _check_case, adata_of
from threshold_edge_inputs import spread     # N_PERTURB one-ulp perturbations of exp / log / erf / erfc

pytestmark = pytest.mark.gpu

G = load_golden("ref_threshold.npz")
GOLDEN_CASES = {c["name"]: c for c in tr.golden_cases(G)}


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


def _draws(seed, K, n_init=10):
    from spatialcore_amd.spatial.neighborhoods import kmeans_draws

    return kmeans_draws(seed, n_init, K)


def features(n, F, dtype, seed):
    """Log-normal markers with dropout zeros; a row with a NaN, a row with +Inf, an all-zero column (F >= 2)."""
    rng = np.random.default_rng(seed)
    M = rng.lognormal(0.0, 1.0, (n, F)) * (rng.random((n, F)) > 0.25)
    if F >= 2:
        M[:, 0] = 0.0
    M[n // 3, F - 1] = np.nan
    M[n - 1, 0] = np.inf
    return M.astype(dtype)


# ---- metagene --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [100, 257, 4097])        # one tile and less; one past a 256-thread tile; one past two 2048-point groups
def test_metagene_matches_restatement(n, dtype):
    ctx = _ctx()
    for F in (1, 2, 3, 8):
        M = features(n, F, dtype, seed=n + F)
        for method in tr.METHODS:
            got, want = ctx.metagene_score(M, method, 0.1), tr.metagene(M, method, 0.1)
            assert got["score"].dtype == M.dtype
            assert np.array_equal(got["valid"], want["valid"]) and got["valid"].sum() == n - 2
            assert np.isnan(got["score"][~got["valid"]]).all()
            for k in ("n_valid", "n_below", "n_negative"):
                assert got[k] == want[k], (F, method, k)
            v = want["valid"]
            if method in ("minimum", "median", "arithmetic_mean"):
                assert np.array_equal(got["score"][v], want["score"][v]), (F, method)
                assert (got["min"], got["max"], got["mean"]) == (want["min"], want["max"], want["mean"]), (F, method)
            else:
                base = [want["score"][v], np.array([want["min"], want["max"], want["mean"]])]
                tol = spread(lambda: (lambda r: [r["score"][v], np.array([r["min"], r["max"], r["mean"]])])(
                    tr.metagene(M, method, 0.1)), base)
                d = np.max(np.abs(got["score"][v].astype(float) - want["score"][v].astype(float)))
                ds = np.max(np.abs(np.array([got["min"], got["max"], got["mean"]]) - base[1]))
                print(f"n={n} F={F} {method} {M.dtype}: score dev {d:.3g} (spread {tol[0]:.3g}), stats dev {ds:.3g} (spread {tol[1]:.3g})")
                assert d <= 16 * tol[0] and ds <= 16 * tol[1], (F, method)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_metagene_matches_reference_golden(dt):
    ctx = _ctx()
    for F in (1, 2, 3, 8):
        M, ref = G[f"mg_{F}_{dt}_features"], G[f"mg_{F}_{dt}_scores"]
        for k, method in enumerate(tr.METHODS):
            got = ctx.metagene_score(M, method, 0.1)
            v = np.all(np.isfinite(M), axis=1)
            assert np.array_equal(got["valid"], v)
            d = float(np.max(np.abs(got["score"][v].astype(float) - ref[k].astype(float))))
            tol = tr.reference_tolerance(float(G[f"mg_{F}_{dt}_dev"][k]), float(G[f"mg_{F}_{dt}_ulp"][k]))
            print(f"F={F} {dt} {method}: dev {d:.3g} tolerance {tol:.3g}")
            if method in ("minimum", "median"):
                assert np.array_equal(got["score"][v], ref[k])
            else:
                assert d <= tol, (F, method)


def test_metagene_rejects_bad_arguments():
    ctx = _ctx()
    with pytest.raises(ValueError, match="n_features"):
        ctx.metagene_score(np.ones((10, 65)), "minimum")
    with pytest.raises(ValueError):
        ctx.metagene_score(np.ones((10, 2)), "mode")


# ---- KS ----------------------------------------------------------------------------------------------------------------
def _ks_inputs():
    rng = np.random.default_rng(11)

    def mix(n):
        return np.where(rng.random(n) < 0.45, rng.normal(2.3, 0.08, n), rng.uniform(0.0, 2.0, n))

    zi = np.where(rng.random(1000) < 0.62, 0.0, rng.poisson(3.0, 1000) + 1.0)
    return {
        "n100_q05": (mix(100), 0.05),                       # the API's floor; max(int(100 * 0.05), 10) = 10 binds
        "n4097": (mix(4097), 0.5),                          # sorted array and D cross three workgroups
        "ties": (np.round(mix(600), 1), 0.5),               # runs of equal scores, one of them across the argmax
        "zero_inflated": (zi, 0.5),                         # zero background variance: IQR and 90th-percentile fallbacks
        "constant": (np.full(300, 0.7), 0.5),               # range < 1e-10 everywhere
    }


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["n100_q05", "n4097", "ties", "zero_inflated", "constant"])
def test_ks_matches_restatement(name, dtype):
    from spatialcore_amd.stats import classify as cl

    x, q = _ks_inputs()[name]
    x = x.astype(dtype)
    ctx = _ctx()
    s, mean, sd = tr.ks_background(x, q)
    prep = ctx.ks_prepare(x, q, ranks=[0, x.size - 1, x.size // 2], return_sorted=True)
    assert np.array_equal(prep["sorted"], s)                                   # the sort, bit for bit
    assert np.array_equal(prep["order"], s[[0, x.size - 1, x.size // 2]])
    assert (prep["bg_mean"], prep["bg_std"]) == (mean, sd)                     # sums in block order, IEEE sqrt and divide
    thr, dev, lab, p = tr.ks(x, q)
    i, score, D = ctx.ks_argmax(p["background_mean"], p["background_std"])
    # D is a difference of two numbers of magnitude <= 1, each rounded to the grid of 2^-53 there: an ulp of erf / erfc
    # that the perturbation happens to round away can still move D by one step of that grid
    tol_D = 16 * spread(lambda: [np.array(tr.ks(x, q)[3]["D"])], [np.array(p["D"])])[0] + 2.0 ** -52
    print(f"{name} {x.dtype}: argmax {i} (restated {p['argmax']}), D dev {abs(D - p['D']):.3g} (tolerance {tol_D:.3g}), "
          f"fallbacks [{p['std_fallback']}, p90={p['p90_fallback']}]")
    assert i == p["argmax"] and score == s[i] and abs(D - p["D"]) <= tol_D
    if name == "ties":
        assert s[i] == s[i - 1] or s[i] == s[min(i + 1, x.size - 1)]           # the argmax sits in a run of equal scores
    if name == "zero_inflated":
        assert p["std_fallback"] == "iqr" and p["p90_fallback"]
    if name == "constant":
        assert p["std_fallback"] == "range" and lab.all() and not dev.any()
    g_thr, g_dev, g_lab, g_high, g_prm = cl._threshold_ks(ctx, x, q)
    assert g_thr == thr and np.array_equal(g_dev, dev) and np.array_equal(g_lab, lab) and g_high == lab.sum()
    assert (g_prm["background_mean"], g_prm["background_std"]) == (p["background_mean"], p["background_std"])


def test_ks_argmax_takes_the_first_of_equal_deviations():
    """Two exactly equal largest D in different workgroups: h scores far below the background (Phi = 0) and h scores AT
    its mean (Phi = 0.5 exactly) give D[h - 1] = h / n - 0 = 0.5 and D[n - 1] = 1 - 0.5 = 0.5.  numpy's argmax answers
    with the first; h = 2049 puts index 2048 in the second workgroup and index 4097 in the third."""
    ctx = _ctx()
    h = 2049
    x = np.concatenate([np.full(h, 1.0), np.full(h, -1000.0)])
    ctx.ks_prepare(x, 0.5)
    D = tr.ks_deviation(np.sort(x), 1.0, 1.0)
    assert D[h - 1] == D[2 * h - 1] == 0.5 == D.max() and int(np.argmax(D)) == h - 1
    assert ctx.ks_argmax(1.0, 1.0) == (h - 1, -1000.0, 0.5)
    # saturated Phi: D = (i + 1) / n - 1 rises to exactly 0 at the last index
    assert ctx.ks_argmax(-5000.0, 1e-3) == (2 * h - 1, 1.0, 0.0)


def test_ks_needs_prepare_and_valid_moments():
    from spatialcore_amd import _lib

    with _lib.Context(0) as fresh:
        with pytest.raises(_lib.SpatialCoreHipError, match="sc_ks_prepare first"):
            fresh.ks_argmax(0.0, 1.0)
        fresh.ks_prepare(np.arange(100.0), 0.5)
        with pytest.raises(ValueError, match="standard deviation"):
            fresh.ks_argmax(0.0, 0.0)


# ---- GMM ---------------------------------------------------------------------------------------------------------------
def trimodal(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    return np.where(u < 0.45, np.abs(rng.normal(0.2, 0.15, n)),
                    np.where(u < 0.8, rng.normal(1.4, 0.45, n), rng.normal(3.2, 0.7, n)))


def bimodal(n, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.35, rng.normal(3.0, 0.6, n), np.abs(rng.normal(0.4, 0.3, n)))


def _fit_both(x, K, seed, max_iter=100, n_init=10):
    X = x.reshape(-1, 1)
    draws = _draws(seed, K, n_init)
    got = _ctx().gmm_fit(x, K, n_init, 300, float(np.mean(np.var(X, axis=0)) * 1e-4), X.mean(axis=0), draws, max_iter,
                         return_km_labels=True)
    want = tr.gmm_fit(x, K, draws, max_iter=max_iter)
    return got, want, draws


def _assert_fit(got, want, x, K, draws, max_iter=100, what=""):
    assert np.array_equal(got["km_labels"], want["km_labels"])                 # every run's k-means labels
    assert np.array_equal(got["n_iter"], want["n_iter"]) and np.array_equal(got["converged"], want["converged"])
    base = [want["weights"], want["means"], want["variances"], want["lower_bound"]]
    tol = spread(lambda: (lambda f: [f["weights"], f["means"], f["variances"], f["lower_bound"]])(
        tr.gmm_fit(x, K, draws, max_iter=max_iter, km_labels=want["km_labels"])), base)
    for k, t, b in zip(("weights", "means", "variances", "lower_bound"), tol, base):
        d = float(np.max(np.abs(got[k] - b)))
        print(f"{what} {k}: dev {d:.3g}, one-ulp spread {t:.3g}")
        assert d <= 16 * t, k
    # the best run: the first of the largest lower bounds, unless two runs are closer than the tolerance
    lb = want["lower_bound"]
    if lb.size == 1:
        assert got["best"] == want["best"] == 0
    elif np.sort(lb)[-1] - np.sort(lb)[-2] > 32 * tol[3]:
        assert got["best"] == want["best"]
    else:
        assert lb[want["best"]] - lb[got["best"]] <= 32 * tol[3]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", [2, 3])
def test_gmm_small_matches_restatement(K, dtype):
    """Case A: n = 300, one workgroup.  The K = 3 input has runs that stop after 7, 8 and 9 iterations (fp64)."""
    x = trimodal(300, 19).astype(dtype)
    got, want, draws = _fit_both(x, K, 19)
    if K == 3 and dtype == np.float64:
        assert sorted(set(want["n_iter"].tolist())) == [7, 8, 9]
    assert want["converged"].all()
    _assert_fit(got, want, x, K, draws, what=f"A K={K} {x.dtype}")


def test_gmm_across_workgroups_matches_restatement():
    """Case B: n = 4097 -- three workgroups, the last with one point."""
    x = bimodal(4097, 5)
    got, want, draws = _fit_both(x, 2, 5)
    _assert_fit(got, want, x, 2, draws, what="B")


def test_gmm_fit_on_a_sample_scores_every_cell():
    """Case C: max_cells = 150 of n = 400 -- the fit on the sample, the posteriors on all cells."""
    from spatialcore_amd.stats import classify as cl

    x = bimodal(400, 8)
    fit_scores = x[cl.sample_indices(400, 150, 42)]
    thr, prob, lab, n_high, prm = cl._threshold_gmm(_ctx(), fit_scores, x, 0.3, 2, 42)

    def restated():
        f = tr.gmm_fit(fit_scores, 2, _draws(42, 2))
        b = f["best"]
        w, mu, var = f["weights"][b], f["means"][b], f["variances"][b]
        t, high, _ = tr.gmm_threshold(w, mu, var, 2)
        return [tr.gmm_posterior(x, w, mu, var, high, 0.3)[0], np.array(t), tr.sorted_parameters(w, mu, var)]

    base = restated()
    tol = spread(restated, base)
    d = float(np.max(np.abs(prob - base[0])))
    got_par = tr.sorted_parameters(prm["gmm_weights"], prm["gmm_means"], np.square(prm["gmm_stds"]))
    print(f"C: P(high) dev {d:.3g} (spread {tol[0]:.3g}), parameters dev {np.max(np.abs(got_par - base[2])):.3g} (spread {tol[2]:.3g})")
    assert prob.shape == (400,) and d <= 16 * tol[0]
    assert np.max(np.abs(got_par - base[2])) <= 16 * tol[2] + 4 * np.finfo(float).eps * base[2].max()   # (params hold stds: squared again)
    step = abs(base[2][3] - base[2][2]) / 999.0
    assert abs(thr - float(base[1])) <= step
    decided = np.abs(base[0] - 0.3) > 16 * tol[0]
    assert np.array_equal(lab[decided], (base[0] > 0.3)[decided]) and n_high == lab.sum()
    assert (~decided).sum() <= 0.001 * 400


def test_gmm_max_iter_through_the_abi():
    """Case D: max_iter = 2 -- runs that would need more stop unconverged, with the parameters of their second M-step."""
    x = trimodal(300, 19)
    got, want, draws = _fit_both(x, 3, 19, max_iter=2)
    assert (want["n_iter"] == 2).all() and not want["converged"].any()
    _assert_fit(got, want, x, 3, draws, max_iter=2, what="D")


def test_gmm_is_reproducible():
    x = bimodal(4097, 5).astype(np.float32)
    a, _, _ = _fit_both(x, 2, 5)
    X = x.reshape(-1, 1)
    b = _ctx().gmm_fit(x, 2, 10, 300, float(np.mean(np.var(X, axis=0)) * 1e-4), X.mean(axis=0), _draws(5, 2),
                       return_km_labels=True)
    for k in ("weights", "means", "variances", "lower_bound", "n_iter", "converged", "km_labels"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best"] == b["best"]
    w, mu, var = (a[k][a["best"]] for k in ("weights", "means", "variances"))
    p1 = _ctx().gmm_posterior(x, w, mu, var, [int(np.argmax(mu))], 0.3)
    p2 = _ctx().gmm_posterior(x, w, mu, var, [int(np.argmax(mu))], 0.3)
    assert p1[0].tobytes() == p2[0].tobytes() and p1[1].tobytes() == p2[1].tobytes() and p1[2] == p2[2]


def test_gmm_rejects_bad_arguments():
    x = bimodal(300, 1)
    ctx = _ctx()
    with pytest.raises(ValueError, match="2 <= K"):
        ctx.gmm_fit(x, 9, 10, 300, 1e-4, [x.mean()], _draws(0, 9))
    with pytest.raises(ValueError, match="positive weight and variance"):
        ctx.gmm_posterior(x, [0.5, 0.5], [0.0, 1.0], [1.0, 0.0], [1], 0.3)
    with pytest.raises(ValueError, match="outside"):
        ctx.gmm_posterior(x, [0.5, 0.5], [0.0, 1.0], [1.0, 1.0], [2], 0.3)


# ---- the public function -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_classify_by_threshold_matches_reference(name):
    from spatialcore_amd.stats import classify_by_threshold

    case = dict(GOLDEN_CASES[name], golden=G)
    a = adata_of(case["features"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        classify_by_threshold(a, list(a.var_names), plot=False, **case["kwargs"])
    prm, stat = a.uns["threshold_params"], case["stat"]
    v = np.all(np.isfinite(case["features"]), axis=1)
    print(f"{name}: threshold dev {abs(prm['threshold'] - stat['threshold']):.3g} (restatement's {stat['dev_threshold']:.3g}), "
          f"probability dev {np.max(np.abs(a.obs['threshold_probability'].to_numpy()[v] - G[f'{name}_probability'][v])):.3g} "
          f"(restatement's {stat['dev_probability']:.3g}, one-ulp spread {stat['ulp_probability']:.3g})")
    _check_case(case, a, stat)


def test_vignette_chain_local_moran_to_domains(monkeypatch):
    """local_morans_i -> classify_by_threshold("local_morans_I:g0") -> make_spatial_domains on this package alone, and
    the classification against the restatement on the same local Moran values."""
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import local_morans_i, make_spatial_domains
    from spatialcore_amd.stats import classify_by_threshold

    coords, X = synth(600, 4, 21, dtype=np.float32)
    ad = make_adata(coords, X)
    local_morans_i(ad, genes=["g0", "g2"], n_neighbors=6, n_permutations=10, seed=0)
    assert ad.uns["local_morans_params"]["genes"] == ["g0", "g2"]
    kw = dict(metagene_method="arithmetic_mean", threshold_method="ks", column_prefix="x", plot=False)
    classify_by_threshold(ad, ["local_morans_I:g0"], **kw)
    hi = ad.obs["x_cluster"].to_numpy() == 1
    assert 0 < hi.sum() < 600
    twin = ad.copy()
    monkeypatch.setattr(_lib, "default_context", lambda device=0: tr.RestatedContext())
    classify_by_threshold(twin, ["local_morans_I:g0"], **kw)
    monkeypatch.undo()
    for col in ("x_score", "x_probability", "x_cluster"):        # KS: nothing but sums, sqrt, divide and erfc's argmax
        assert np.array_equal(ad.obs[col].to_numpy(), twin.obs[col].to_numpy()), col
    assert ad.uns["x_params"]["threshold"] == twin.uns["x_params"]["threshold"]
    ad.obs["hot"] = ad.obs["x_cluster"] == 1                   # the vignette's step: a boolean column for the filter
    make_spatial_domains(ad, "hot", cell_dist_um=25.0, shrink_margin_um=10.0, min_target_cells_domain=2,
                         domain_prefix="hot")
    dom = ad.obs["spatial_domain"]
    assert dom.notna().any() and set(dom[hi & dom.notna()].map(lambda s: s.split("_")[0])) == {"hot"}
    ops = [o["function"] for o in ad.uns["spatialcore_metadata"]["operations"]]
    assert ops[-3:] == ["local_morans_i", "classify_by_threshold", "make_spatial_domains"]
