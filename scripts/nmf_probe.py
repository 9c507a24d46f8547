"""fit_nmf at 10^6 cells x 500 genes of the bench's synthetic counts, K = 20, 200 iterations (tol = 0), both losses.
Per loss: the public call's wall time; its parts measured on their own (canonical CSR on the host, the host's replay of
sklearn's init="random" -- 2 x 10^7 legacy RandomState normals --, the C entry: upload, column-sorted copy, iterations,
read-back); the HIP-event times per kernel family (sc_ctx_kernel_time); the compulsory bytes per iteration of the
formulation against the HBM peak.  Baseline: sklearn on this host at the first 10^5 cells for 20 iterations, per
iteration, scaled linearly to 10^6 cells (labelled as extrapolated).  Writes profiles/nmf_1m.json.

Usage:  python scripts/nmf_probe.py [n_cells [n_genes [baseline_cells]]]"""
import json
import os
import sys
import time
import warnings

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib, _sparse_input  # noqa: E402
from spatialcore_amd.nmf import factorize, fit_nmf  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 500
n_base = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
K, ITERS, BASE_ITERS = 20, 200, 20
HBM_PEAK = 8.0e12      # bytes / s, MI355X
ctx = _lib.default_context(0)


def say(*a):
    print(*a, flush=True)


t0 = time.perf_counter()
_, dense = bench.synth_inputs(n, G, seed=42)
X = sparse.csr_matrix(dense)
del dense
say(f"input: {n} x {G}, {X.nnz} stored entries ({time.perf_counter() - t0:.1f} s)")
names = [f"g{i}" for i in range(G)]
nnz = int(X.nnz)
# what one iteration has to move at least: both sorted copies of X once (int32 index + fp64 value), W read and written
# by the W pass, read by the sums over cells and once more by the H pass
compulsory = 2 * nnz * 12 + 4 * n * K * 8
gathered = 2 * nnz * K * 8        # the K-value rows fetched per stored entry: H^T rows (W pass), W rows (H pass)


def timed(fn, *a, **kw):
    ctx.sync()
    t = time.perf_counter()
    r = fn(*a, **kw)
    ctx.sync()
    return time.perf_counter() - t, r


def device(loss):
    ad = SimpleAnnData(X, var_names=names)
    fit_nmf(SimpleAnnData(X[:4096], var_names=names), K, beta_loss=loss, max_iter=2, tol=0.0)     # code objects, allocations
    wall, _ = timed(fit_nmf, ad, K, beta_loss=loss, max_iter=ITERS, tol=0.0, random_state=0)
    say(f"{loss}: public call {wall:.2f} s")
    t_csr, (Xc, _) = timed(_sparse_input.canonical_csr, X, np.arange(G), G, negative="negative", all_zero="all zero")   # as fit_nmf asks
    t_init, (W0, H0) = timed(factorize.random_init, factorize._scale(Xc, K), n, G, K, 0)
    ctx.reset_timers()
    t_entry, res = timed(ctx.nmf_fit, Xc.indptr, Xc.indices, Xc.data, G, W0, H0, loss, True, ITERS, 0.0)
    kern = {what: ctx.kernel_time(kid) for what, kid in (("setup", _lib.K_NMF_SETUP), ("w_pass", _lib.K_NMF_W),
                                                         ("h_pass", _lib.K_NMF_H), ("error", _lib.K_NMF_ERR))}
    np.testing.assert_array_equal(res["W"].astype(np.float32), ad.obsm["X_nmf"])      # the parts are the call
    per_iter_ms = (kern["w_pass"][0] + kern["h_pass"][0]) / ITERS
    return {
        "public_call_s": wall, "host_canonical_csr_s": t_csr, "host_random_init_s": t_init, "c_entry_s": t_entry,
        "c_entry_minus_kernels_s": t_entry - sum(v[0] for v in kern.values()) / 1e3,
        "kernel_ms": {k: v[0] for k, v in kern.items()}, "kernel_scopes": {k: v[1] for k, v in kern.items()},
        "per_iteration_kernel_ms": per_iter_ms, "w_pass_ms_per_iteration": kern["w_pass"][0] / ITERS,
        "h_pass_ms_per_iteration": kern["h_pass"][0] / ITERS,
        "compulsory_fraction_of_hbm_peak": compulsory / (per_iter_ms * 1e-3) / HBM_PEAK,
        "gathered_rows_bytes_per_s": gathered / (per_iter_ms * 1e-3),
        "n_iter": res["n_iter"], "reconstruction_err": res["reconstruction_err"], "error_at_init": float(res["error_trace"][0]),
    }, (W0, H0)


def baseline(loss, W0, H0):
    from sklearn.decomposition import NMF

    Xb = sparse.csr_matrix(X[:n_base], dtype=np.float64)
    m = NMF(n_components=K, init="custom", solver="mu", beta_loss=loss, max_iter=BASE_ITERS, tol=0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = time.perf_counter()
        m.fit_transform(Xb, W=W0[:n_base].copy(), H=H0.copy())
        dt = time.perf_counter() - t
    say(f"{loss}: sklearn {n_base} cells x {BASE_ITERS} iterations {dt:.1f} s")
    return {"cells": n_base, "iterations": BASE_ITERS, "fit_s": dt, "per_iteration_s": dt / BASE_ITERS,
            "per_iteration_s_extrapolated_to_n": dt / BASE_ITERS * n / n_base, "extrapolated": True}


out = {"workload": f"{n} cells x {G} genes of bench.synth_inputs(seed=42) (float32 counts), {nnz} stored entries, K = {K}, "
                   f"{ITERS} iterations, tol = 0, init='random' (random_state=0); one small warm-up call, then one timed call",
       "stored_entries": nnz, "compulsory_bytes_per_iteration": compulsory, "gathered_row_bytes_per_iteration": gathered,
       "hbm_peak_bytes_per_s": HBM_PEAK}
for loss in ("frobenius", "kullback-leibler"):
    out[loss], start = device(loss)
    out[loss]["sklearn_same_host"] = baseline(loss, *start)
    out[loss]["speedup_per_iteration_vs_extrapolated_sklearn"] = (
        out[loss]["sklearn_same_host"]["per_iteration_s_extrapolated_to_n"] / (out[loss]["per_iteration_kernel_ms"] * 1e-3))
out["device_mem_bytes"] = ctx.device_mem()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "nmf_1m.json"), "w") as f:
    json.dump(out, f, indent=1)
say(json.dumps(out, indent=1))
