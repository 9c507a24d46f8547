"""classify_by_threshold at 10^6 cells x 3 markers (float64), K = 2, the reference's defaults: wall time per stage
(metagene, sort / KS, mixture fit = k-means initialisation + EM, posteriors) with the mixture fitted on the reference's
max_cells=20000 sample and on every cell (max_cells=None), the context's kernel timers, and the kernel time of one EM
iteration against its compulsory bytes (all n_init runs share the pass: one 8-byte read per score per iteration).
One warm-up per stage, then the median of 5.  Writes profiles/threshold_1m.json.

Usage:  python scripts/threshold_probe.py"""
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.spatial.neighborhoods import kmeans_draws  # noqa: E402
from spatialcore_amd.stats import classify as cl  # noqa: E402
from spatialcore_amd.stats import classify_by_threshold  # noqa: E402

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes / s
REPS = 5

n, F, K = 1_000_000, 3, 2
rng = np.random.default_rng(0)
hi = rng.random(n) < 0.35
M = np.where(hi[:, None], rng.lognormal(1.2, 0.35, (n, F)), rng.lognormal(-1.5, 0.5, (n, F)))
ctx = _lib.default_context(0)


def timed(fn):
    fn()                                  # warm-up: code objects, allocations
    walls = []
    for _ in range(REPS):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        walls.append(time.perf_counter() - t0)
    return float(np.median(walls)), out


def kernel_ms(*ids):
    return sum(ctx.kernel_time(k)[0] for k in ids) / REPS, sum(ctx.kernel_time(k)[1] for k in ids) / REPS


out = {"workload": f"classify_by_threshold, {n} cells x {F} markers (float64), shifted_geometric_mean, "
                   f"GaussianMixture(n_components={K}, n_init=10), seed=42; KS with background_quantile=0.5",
       "stages": {}}

wall, mg = timed(lambda: ctx.metagene_score(M, "shifted_geometric_mean", 0.1))
scores = mg["score"][mg["valid"]]
out["stages"]["metagene"] = {"wall_s": wall}
wall, _ = timed(lambda: cl._threshold_ks(ctx, scores, 0.5))
out["stages"]["sort_and_ks"] = {"wall_s": wall}

for label, max_cells in (("max_cells_20000", 20000), ("max_cells_none", None)):
    fit_scores = scores if max_cells is None else scores[cl.sample_indices(scores.size, max_cells, 42)]
    X = fit_scores.reshape(-1, 1)
    km_tol, x_mean, draws = float(np.mean(np.var(X, axis=0)) * 1e-4), X.mean(axis=0), kmeans_draws(42, 10, K)
    ctx.gmm_fit(fit_scores, K, 10, 300, km_tol, x_mean, draws)
    ctx.reset_timers()
    wall, fit = timed(lambda: ctx.gmm_fit(fit_scores, K, 10, 300, km_tol, x_mean, draws))
    # (timed() runs REPS + 1 calls after the reset: scale the timers accordingly)
    scale = REPS / (REPS + 1)
    km_ms, _ = kernel_ms(_lib.K_KMEANS_SEED, _lib.K_KMEANS_LLOYD)
    em_ms, em_scopes = kernel_ms(_lib.K_GMM_EM)
    iters = int(fit["n_iter"].max())
    b = fit["best"]
    w, mu, var = fit["weights"][b], fit["means"][b], fit["variances"][b]
    pwall, _ = timed(lambda: ctx.gmm_posterior(scores, w, mu, var, [int(np.argmax(mu))], 0.3))
    a = SimpleAnnData(M, obs=pd.DataFrame(index=pd.RangeIndex(n).astype(str)), var_names=["a", "b", "c"])
    cwall, _ = timed(lambda: classify_by_threshold(a, ["a", "b", "c"], max_cells=max_cells, plot=False))
    pass_bytes = fit_scores.size * 8
    out["stages"][label] = {
        "cells_fitted": int(fit_scores.size),
        "gmm_fit_wall_s": wall,
        "kmeans_init_kernel_ms": km_ms * scale,
        "em_kernel_ms": em_ms * scale,
        "em_iterations_longest_run": iters, "n_iter_all_runs": fit["n_iter"].tolist(),
        "em_kernel_ms_per_timer_scope": em_ms / max(em_scopes, 1),
        "em_pass_compulsory_bytes": pass_bytes, "em_pass_hbm_floor_ms": pass_bytes / HBM_PEAK * 1e3,
        "posteriors_wall_s": pwall,
        "classify_by_threshold_wall_s": cwall,
    }

out["cpu_reference_s"] = {"GaussianMixture(2, n_init=10).fit, 1e6 scores": 8.3,
                          "GaussianMixture(2, n_init=10).fit, 20000 scores": "1.2-1.5",
                          "predict_proba, 1e6": 0.24, "threshold_ks, 1e6": 0.07}
out["cpu_reference_note"] = ("sklearn 1.7.2 / scipy on the CPU of the build container, not on the host of the GPU machine; "
                             "synthetic 3-marker metagene scores")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "threshold_1m.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
