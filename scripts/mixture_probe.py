"""gaussian_mixture at 10^6 cells of the bench's coordinates: X_pca (pca of the bench's synthetic counts, 50 components,
normalize=True, float64) truncated to d = 16 and d = 50, aggregate_neighbors(n_layers=3) on the k = 6 graph (D = 64 and
D = 200), K = 20, "full" and "diag".

Per (D, covariance type): the public call's wall time (max_iter = ITERS, tol = 0, so every call runs ITERS iterations; one
small warm-up call first), the time per EM iteration (from two calls through the binding that differ in max_iter only, so
that the k-means start and the transfers cancel), the E- and M-kernel times per iteration from SC_K_MIX_ESTEP /
SC_K_MIX_MSTEP, their fp64 rate against the data-sheet matrix peak (78.6 TFLOP/s; not measured here), the precision stage's
share (the M id of a sc_mixture_predict call holds it alone), and sklearn's GaussianMixture with the same settings on the
first 50,000 cells of the same host, scaled by the cell count.  Writes profiles/mixture_1m.json.

Usage:  python scripts/mixture_probe.py [n_cells [out.json]]"""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.cluster import gaussian_mixture  # noqa: E402
from spatialcore_amd.cluster.mixture import _fit  # noqa: E402
from spatialcore_amd.pca import pca  # noqa: E402
from spatialcore_amd.spatial import aggregate_neighbors  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mixture_1m.json")
G, K, ITERS, N_SKLEARN, PEAK = 500, 20, 10, 50_000, 78.6e12
ctx = _lib.default_context(0)


def say(*a):
    print(*a, flush=True)


t0 = time.perf_counter()
coords, dense = bench.synth_inputs(n, G, seed=42)
coords = np.ascontiguousarray(coords, dtype=np.float64)
ad = SimpleAnnData(dense, var_names=[f"g{i}" for i in range(G)])
pca(ad, n_comps=50, normalize=True, dtype="float64")
scores = np.ascontiguousarray(ad.obsm["X_pca"])
del dense, ad
say(f"input: {n} cells, X_pca {scores.shape} ({time.perf_counter() - t0:.1f} s)")


def kernel_ms():
    return {name: ctx.kernel_time(kid)[0] for name, kid in (("e", _lib.K_MIX_ESTEP), ("m", _lib.K_MIX_MSTEP))}


def flops(D, ct):
    """Useful fp64 operations of one iteration (multiply and add counted separately): E q = ||x P - b||^2 over the upper
    triangle of P, M the upper triangle of the covariance sum; "diag" 3 D and 4 D per (cell, component)."""
    if ct == "full":
        return {"e": n * K * D * (D + 1), "m": n * K * D * (D + 1)}
    return {"e": n * K * 3 * D, "m": n * K * 4 * D}


out = {"workload": f"{n} cells on bench.synth_inputs(seed=42)'s coordinates; X_pca = pca(50, normalize=True, float64) of its {G}-gene "
                   f"counts truncated to d; aggregate_neighbors(n_layers=3, n_neighbors=6); gaussian_mixture(K={K}, max_iter={ITERS}, tol=0)",
       "fp64_matrix_peak_flops": PEAK, "peak_is": "the data sheet's, not measured here", "runs": {}}
for d in (16, 50):
    a = SimpleAnnData(np.zeros((n, 1)), var_names=["g"], obsm={"spatial": coords, "X_pca": np.ascontiguousarray(scores[:, :d])})
    aggregate_neighbors(a, n_layers=3, n_neighbors=6)
    X = np.ascontiguousarray(a.obsm["X_cellcharter"], dtype=np.float64)
    D = X.shape[1]
    for ct in ("full", "diag"):
        entry = {"D": D, "slice_rows": _lib.mixture_slice_rows(n, D, K, ct)}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            small = SimpleAnnData(np.zeros((8192, 1)), var_names=["g"], obsm={"X_cellcharter": X[:8192]})
            gaussian_mixture(small, K, covariance_type=ct, max_iter=2, tol=0.0)      # code objects
            ctx.sync()
            t = time.perf_counter()
            gaussian_mixture(a, K, covariance_type=ct, max_iter=ITERS, tol=0.0)
            entry["public_call_s"] = time.perf_counter() - t
            ctx.reset_timers()
            t = time.perf_counter()
            _fit(ctx, X, K, ct, 1, 2, 0.0, 1e-6, 0, False)
            t_short = time.perf_counter() - t
            ms_short = kernel_ms()
            ctx.reset_timers()
            t = time.perf_counter()
            fit = _fit(ctx, X, K, ct, 1, ITERS, 0.0, 1e-6, 0, False)
            t_long = time.perf_counter() - t
            ms_long = kernel_ms()
        per = {k: (ms_long[k] - ms_short[k]) / (ITERS - 2) for k in ms_long}
        entry["iteration_s"] = (t_long - t_short) / (ITERS - 2)
        entry["e_kernels_ms_per_iteration"], entry["m_kernels_ms_per_iteration"] = per["e"], per["m"]
        f = flops(D, ct)
        entry["e_flops_per_s"], entry["m_flops_per_s"] = f["e"] / (per["e"] * 1e-3), f["m"] / (per["m"] * 1e-3)
        entry["e_share_of_peak"], entry["m_share_of_peak"] = entry["e_flops_per_s"] / PEAK, entry["m_flops_per_s"] / PEAK
        b = fit["best"]
        ctx.reset_timers()
        ctx.mixture_predict(X[:4096], ct, fit["weights"][b], fit["means"][b], fit["covariances"][b])
        entry["precision_stage_ms"] = kernel_ms()["m"]
        entry["precision_share_of_m"] = entry["precision_stage_ms"] / per["m"]
        entry["start_and_transfers_s"] = t_short - 2 * entry["iteration_s"]
        entry["lower_bound"] = float(fit["lower_bound"][b])
        m = min(N_SKLEARN, n)
        from sklearn.mixture import GaussianMixture

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = time.perf_counter()
            GaussianMixture(K, covariance_type=ct, max_iter=ITERS, tol=0.0, random_state=0).fit(X[:m])
            ts = time.perf_counter() - t
        entry["sklearn"] = {"cells": m, "s": ts, "scaled_to_n_s": ts * n / m, "scaling": "by the cell count"}
        say(f"D = {D} {ct}:", entry)
        out["runs"][f"D{D}_{ct}"] = entry
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:      # after every configuration: a run that is cut short keeps what it measured
            json.dump(out, fh, indent=1)
    del a, X
say("written", OUT)
