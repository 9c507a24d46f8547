"""Generate tests/golden/ref_threshold.npz from the reference's own classify_by_threshold / _thresholding (numpy, scipy,
sklearn's GaussianMixture).

Build container only: needs the reference's source tree (REF_SRC), sklearn and matplotlib.  The reference modules are
imported with inert stand-ins for the absent ``anndata`` (the technique of scripts/make_niche_golden.py); only data is
written, with allow_pickle=False on the reading side.

Per case the file holds the inputs, the reference's outputs, the deviation of tests/threshold_restated.py from the
reference for every compared quantity (``*_dev``: the device-against-reference tolerance is 4 x that), the spread of
the restatement under one-ulp perturbation of every exp / log / erf / erfc result (``*_ulp``: the device-against-
restatement tolerance is 16 x that) and the stability flags.  A case that fails a flag is REFUSED (the script stops):
 - GMM: the restatement's k-means labels equal sklearn's for all ten runs (recorded by wrapping KMeans.fit); the
   smallest | |change| - tol | over all runs and iterations exceeds 1e-9 (so n_iter cannot flip); every run whose lower
   bound is within 1e-5 of the best has mean-sorted parameters within 1e-4 of the best's (optimum_stable); the cells
   whose |P(high) - cutoff| is within the tolerance are at most 0.1 % of the case;
 - KS: the two largest D at distinct scores differ by more than the tolerance (ks_gap); the cells within the tolerance
   of the threshold are at most 0.1 %.

Usage:  python scripts/make_threshold_golden.py
"""

from __future__ import annotations

import importlib
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "ref_threshold.npz")
REF_SRC = "/root/reference/src"
N_PERTURB = 6

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from spatialcore_amd._adata import SimpleAnnData  # noqa: E402
from spatialcore_amd.spatial.neighborhoods import kmeans_draws  # noqa: E402
from spatialcore_amd.stats.classify import sample_indices  # noqa: E402
import threshold_restated as tr  # noqa: E402


class Refused(RuntimeError):
    pass


def import_reference():
    ad = types.ModuleType("anndata")
    ad.AnnData = SimpleAnnData
    sys.modules["anndata"] = ad
    for name, sub in (("spatialcore", ""), ("spatialcore.core", "core"), ("spatialcore.stats", "stats")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF_SRC, "spatialcore", sub)]
        sys.modules[name] = pkg
    return (importlib.import_module("spatialcore.stats.classify"),
            importlib.import_module("spatialcore.stats._thresholding"))


KM_LABELS = []


def install_kmeans_recorder():
    from sklearn.cluster import KMeans

    orig = KMeans.fit

    def fit(self, X, y=None, sample_weight=None):
        out = orig(self, X, y, sample_weight)
        KM_LABELS.append(self.labels_.copy())
        return out

    KMeans.fit = fit


def per_run_sklearn(x, K, km_labels):
    """sklearn's own EM from each run's recorded k-means labels: lower bound, n_iter, parameters of every run."""
    from sklearn.mixture import GaussianMixture

    class FromLabels(GaussianMixture):
        def _initialize_parameters(self, X, random_state):
            resp = np.zeros((X.shape[0], self.n_components), dtype=X.dtype)
            resp[np.arange(X.shape[0]), self._labels] = 1
            self._initialize(X, resp)

    runs = []
    for lab in km_labels:
        g = FromLabels(n_components=K, n_init=1, covariance_type="full")
        g._labels = lab
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g.fit(x.reshape(-1, 1))
        o = np.argsort(g.means_.ravel())
        runs.append({"lb": float(g.lower_bound_), "n_iter": int(g.n_iter_),
                     "par": np.concatenate([g.weights_[o], g.means_.ravel()[o], g.covariances_.ravel()[o]]).astype(float)})
    return runs


def spread(fn, base):
    """Largest deviation of fn() from base over N_PERTURB one-ulp perturbations of the math library."""
    worst = [0.0] * len(base)
    for t in range(N_PERTURB):
        with tr.perturbed(np.random.default_rng(1000 + t)):
            got = fn()
        for i, (a, b) in enumerate(zip(got, base)):
            worst[i] = max(worst[i], float(np.max(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float)))))
    return worst


def adata_of(columns, dtype=np.float64):
    n = len(next(iter(columns.values())))
    X = np.column_stack([np.asarray(v, dtype=dtype) for v in columns.values()])
    return SimpleAnnData(X, obs=pd.DataFrame(index=pd.RangeIndex(n).astype(str)), var_names=list(columns))


def sorted_par(w, mu, var):
    o = np.argsort(mu)
    return np.concatenate([np.asarray(w)[o], np.asarray(mu)[o], np.asarray(var)[o]])


def main():
    import sklearn

    cl, th = import_reference()
    install_kmeans_recorder()
    rng = np.random.default_rng(20260101)
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}

    # ---- metagene: every method, F in {1, 2, 3, 8}, both types; NaN / Inf rows in the F = 3 matrix ----------------
    n_mg = 100
    for F in (1, 2, 3, 8):
        M = rng.lognormal(0.0, 1.0, (n_mg, F)) * (rng.random((n_mg, F)) > 0.25)   # dropout zeros
        if F == 3:
            M[[5, 77], 1] = np.nan
            M[[60, 61, 99], 2] = np.inf
        for dt in ("f32", "f64"):
            Md = M.astype(np.float32 if dt == "f32" else np.float64)
            out[f"mg_{F}_{dt}_features"] = Md
            valid = np.all(np.isfinite(Md), axis=1)
            ref_scores, devs_mg, ulps_mg = [], [], []
            for method in tr.METHODS:
                ref = th.compute_metagene_score(Md[valid], method, 0.1)
                base = tr.metagene(Md, method, 0.1)
                assert np.array_equal(base["valid"], valid)
                name = f"mg_{F}_{dt}_{method}"
                ref_scores.append(ref)
                got = base["score"][valid]
                dev = float(np.max(np.abs(got.astype(float) - ref.astype(float))))
                if method in ("minimum", "median") and dev != 0.0:
                    raise Refused(f"{name}: the restatement is not bit-exact ({dev})")
                devs_mg.append(dev)
                ulps_mg.append(spread(lambda: [tr.metagene(Md, method, 0.1)["score"][valid]], [got])[0])
                print(f"{name}: dev {dev:.3g} ulp {ulps_mg[-1]:.3g}")
            # rows in the order of threshold_restated.METHODS; the valid cells only
            out[f"mg_{F}_{dt}_scores"] = np.stack(ref_scores)
            out[f"mg_{F}_{dt}_dev"] = np.array(devs_mg)
            out[f"mg_{F}_{dt}_ulp"] = np.array(ulps_mg)

    # ---- full calls -----------------------------------------------------------------------------------------------
    def lognorm_scores(n):
        """A wide background below a tight expressing population: D peaks above the background mean."""
        bg = rng.uniform(0.0, 2.0, n)
        sig = rng.normal(2.3, 0.08, n)
        return np.where(rng.random(n) < 0.45, sig, bg)

    def zero_inflated(n):
        c = rng.poisson(3.0, n).astype(float) + 1.0
        return np.where(rng.random(n) < 0.62, 0.0, c)

    def bimodal3(n):
        hi = rng.random(n) < 0.35
        base = np.where(hi[:, None], rng.lognormal(1.2, 0.35, (n, 3)), rng.lognormal(-1.5, 0.5, (n, 3)))
        return base

    def trimodal(n):
        u = rng.random(n)
        return np.where(u < 0.5, np.abs(rng.normal(0.1, 0.08, n)), np.where(u < 0.8, rng.normal(1.5, 0.3, n), rng.normal(4.5, 0.5, n)))

    n = 500
    inputs = {"lognorm": lognorm_scores(n)[:, None], "zeroinfl": zero_inflated(n)[:, None], "b3": bimodal3(n),
              "tri": trimodal(n)[:, None]}
    for key, M in inputs.items():
        out[f"input_{key}"] = M
    bad = {"nan": np.array([[3, 0], [250, 0], [499, 0]]), "inf": np.array([[40, 2], [41, 2]])}   # (cell, column)
    ks, am = dict(threshold_method="ks"), dict(metagene_method="arithmetic_mean")
    cases = [  # name, input, dtype, NaN / Inf cells, kwargs
        ("ks_lognorm_f64", "lognorm", np.float64, False, dict(**ks, **am)),
        ("ks_lognorm_f32", "lognorm", np.float32, False, dict(**ks, **am)),
        ("ks_zeroinfl_f64", "zeroinfl", np.float64, False, dict(**ks, **am)),
        ("ks_zeroinfl_f32", "zeroinfl", np.float32, False, dict(**ks, metagene_method="minimum")),
        ("gmm_k2_all_f64", "b3", np.float64, False, dict()),
        ("gmm_k2_sub_f32", "b3", np.float32, False, dict(max_cells=200)),
        ("gmm_k2_nan_f64", "b3", np.float64, True, dict(metagene_method="median")),
        ("gmm_k3_all_f32", "tri", np.float32, False, dict(n_components=3, **am)),
        ("gmm_k3_sub_f64", "tri", np.float64, False, dict(n_components=3, max_cells=250, **am)),
    ]
    table = []   # name, input, dtype, metagene method, threshold method, NaN / Inf cells injected
    for name, key, dtype, with_bad, kw in cases:
        M = inputs[key].copy()
        if with_bad:
            M[bad["nan"][:, 0], bad["nan"][:, 1]] = np.nan
            M[bad["inf"][:, 0], bad["inf"][:, 1]] = np.inf
        feats = [f"m{j}" for j in range(M.shape[1])]
        a = adata_of(dict(zip(feats, M.T)), dtype)
        KM_LABELS.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cl.classify_by_threshold(a, feats, plot=False, **kw)
        prm = a.uns["threshold_params"]
        method = kw.get("metagene_method", "shifted_geometric_mean")
        table.append([name, key, np.dtype(dtype).name, method, kw.get("threshold_method", "gmm"), str(int(with_bad))])
        stat = {"n_components": kw.get("n_components", 2), "max_cells": kw.get("max_cells", 20000)}
        out[f"{name}_score"] = a.obs["threshold_score"].to_numpy().astype(dtype)   # exact: the scores are of this type
        out[f"{name}_probability"] = a.obs["threshold_probability"].to_numpy()
        out[f"{name}_cluster"] = a.obs["threshold_cluster"].to_numpy().astype(np.int64)
        stat["threshold"] = prm["threshold"]
        for k in ("n_high", "n_low", "n_invalid", "n_total"):
            stat[k] = prm[k]

        mg = tr.metagene(np.ascontiguousarray(a.X), method, 0.1)
        valid, scores = mg["valid"], mg["score"][mg["valid"]]
        ref_prob = out[f"{name}_probability"][valid]
        ref_lab = out[f"{name}_cluster"][valid]
        n_valid = scores.size
        if kw.get("threshold_method") == "ks":
            thr, dev, lab, p = tr.ks(scores, 0.5)
            devs = {"threshold": abs(thr - prm["threshold"]), "background_mean": abs(p["background_mean"] - prm["background_mean"]),
                    "background_std": abs(p["background_std"] - prm["background_std"]),
                    "probability": float(np.max(np.abs(dev - ref_prob)))}
            base = [np.array(thr), np.array(p["D"]), dev]
            ulp = spread(lambda: (lambda r: [np.array(r[0]), np.array(r[3]["D"]), r[1]])(tr.ks(scores, 0.5)), base)
            D = tr.ks_deviation(p["sorted"], p["background_mean"], p["background_std"])
            top = np.max(D)
            others = D[p["sorted"] != p["sorted"][p["argmax"]]]
            gap = float(top - np.max(others)) if others.size else np.inf
            tol_thr = 4 * devs["threshold"]
            # (tolerance 0: restatement and reference share one threshold, a score equal to it is decided alike)
            near = int(np.count_nonzero(np.abs(scores.astype(float) - prm["threshold"]) <= tol_thr)) if tol_thr > 0 else 0
            if not p["p90_fallback"] and gap <= max(16 * ulp[1], 1e-12):
                raise Refused(f"{name}: ks_gap {gap:.3g} within the tolerance")
            if near > 0.001 * n_valid:
                raise Refused(f"{name}: {near} cells within {tol_thr:.3g} of the threshold")
            for k in ("background_mean", "background_std", "background_quantile"):
                stat[k] = prm[k]
            stat.update(ks_gap=gap, iqr_fallback=float(p["std_fallback"] == "iqr"), p90_fallback=float(p["p90_fallback"]),
                        excluded_share=near / n_valid, ulp_threshold=ulp[0], ulp_D=ulp[1], ulp_probability=ulp[2])
            mism = int(np.count_nonzero(lab != ref_lab))
            print(f"{name}: thr {thr:.6g} (ref {prm['threshold']:.6g}) fallbacks [{p['std_fallback']}, p90={p['p90_fallback']}] "
                  f"gap {gap:.3g} label mismatches {mism} devs {devs} ulp {ulp}")
        else:
            K = kw.get("n_components", 2)
            max_cells = kw.get("max_cells", 20000)
            fit_scores = scores[sample_indices(n_valid, max_cells, 42)] if max_cells < n_valid else scores
            km_ref = np.stack(KM_LABELS[:10])
            if len(KM_LABELS) != 10:
                raise Refused(f"{name}: {len(KM_LABELS)} KMeans fits recorded")
            draws = kmeans_draws(42, 10, K)
            km = tr.kmeans_run_labels(fit_scores, K, draws)
            if not np.array_equal(km, km_ref):
                raise Refused(f"{name}: k-means labels differ from sklearn's in runs "
                              f"{np.flatnonzero((km != km_ref).any(axis=1)).tolist()}")
            fit = tr.gmm_fit(fit_scores, K, draws, km_labels=km)
            b = fit["best"]
            w, mu, var = fit["weights"][b], fit["means"][b], fit["variances"][b]
            thr, high, order = tr.gmm_threshold(w, mu, var, K)
            prob, lab = tr.gmm_posterior(scores, w, mu, var, high, 0.3)
            runs = per_run_sklearn(fit_scores, K, km_ref)
            margin = min(abs(abs(c) - 1e-3) for t in fit["changes"] for c in t if np.isfinite(c))
            if margin <= 1e-9:
                raise Refused(f"{name}: a change of the lower bound is within 1e-9 of tol")
            if [r["n_iter"] for r in runs] != fit["n_iter"].tolist():
                raise Refused(f"{name}: n_iter differs from sklearn's: {[r['n_iter'] for r in runs]} vs {fit['n_iter'].tolist()}")
            lbs = np.array([r["lb"] for r in runs])
            rb = int(np.argmax(lbs))
            stable = all(np.max(np.abs(r["par"] - runs[rb]["par"])) < 1e-4 for r in runs if lbs[rb] - r["lb"] < 1e-5)
            if not stable:
                raise Refused(f"{name}: runs at the best lower bound disagree on the parameters")
            ref_par = sorted_par(prm["gmm_weights"], prm["gmm_means"], np.square(prm["gmm_stds"]))
            got_par = sorted_par(w, mu, var)
            grid_step = abs(ref_par[K + 1] - ref_par[K]) / 999.0 if K == 2 else 0.0
            devs = {"parameters": float(np.max(np.abs(got_par - ref_par))), "threshold": abs(thr - prm["threshold"]),
                    "probability": float(np.max(np.abs(prob - ref_prob))),
                    "lower_bound": float(np.max(np.abs(fit["lower_bound"] - lbs)))}

            def again():
                f = tr.gmm_fit(fit_scores, K, draws, km_labels=km)
                bb = f["best"]
                pr = tr.gmm_posterior(scores, w, mu, var, high, 0.3)[0]
                return [sorted_par(f["weights"][bb], f["means"][bb], f["variances"][bb]), f["lower_bound"], pr, f["n_iter"]]

            ulp = spread(again, [got_par, fit["lower_bound"], prob, fit["n_iter"]])
            if ulp[3] != 0:
                raise Refused(f"{name}: n_iter moves under one-ulp perturbation")
            tol_p = 4 * devs["probability"]
            margins = np.sort(np.abs(ref_prob - 0.3))
            near = int(np.count_nonzero(margins <= tol_p)) if tol_p > 0 else 0
            if near > 0.001 * n_valid:
                raise Refused(f"{name}: {near} cells within {tol_p:.3g} of the probability cutoff")
            out[f"{name}_km_labels"] = km_ref.astype(np.int8)
            out[f"{name}_ref_parameters"] = ref_par
            out[f"{name}_run_lower_bound"] = lbs
            out[f"{name}_run_n_iter"] = np.array([r["n_iter"] for r in runs], dtype=np.int32)
            out[f"{name}_prob_margin"] = margins[:64]
            stat.update(change_margin=margin, optimum_stable=float(stable), excluded_share=near / n_valid, grid_step=grid_step,
                        ulp_parameters=ulp[0], ulp_lower_bound=ulp[1], ulp_probability=ulp[2])
            mism = int(np.count_nonzero(lab != ref_lab))
            print(f"{name}: n_iter {fit['n_iter'].tolist()} best {b} thr {thr:.6g} (ref {prm['threshold']:.6g}, step {grid_step:.3g}) "
                  f"label mismatches {mism} change margin {margin:.3g} devs {devs} ulp {ulp[:3]}")
        for k, v in devs.items():
            stat[f"dev_{k}"] = float(v)
        # one (names, values) pair per case: tests/threshold_restated.py: case_stats
        out[f"{name}_stat_names"] = np.array(list(stat))
        out[f"{name}_stat_values"] = np.array([float(v) for v in stat.values()])
    out["cases"] = np.array(table)
    out["bad_nan_cells"], out["bad_inf_cells"] = bad["nan"], bad["inf"]
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
