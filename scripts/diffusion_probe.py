"""diffusion_map at 10^6 cells x 20 features of the tests' branching trajectory (tests/diffusion_restated.py: traj),
k = 15, n_comps = 15.  Records the public call's wall time; its parts measured on their own (the search, the graph build,
the eigensolver: Lanczos steps taken, per-step milliseconds split into the sparse product and the orthogonalisation);
device memory; two rooflines against the figures of the MI355X guide (the search against fp64 vector issue, 3 d
instructions per pair and n^2 pairs; the orthogonalisation against HBM, 4 j 8 n bytes at step j).  Baseline: sklearn's
kd_tree plus a numpy graph build plus scipy's eigsh on the first 10^5 cells on this host, scaled to 10^6 cells (the tree as
n log n, the rest linearly; labelled extrapolated).  Writes profiles/diffusion_1m.json.

Usage:  python scripts/diffusion_probe.py [n_cells [baseline_cells]]"""
import json
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diffusion_restated as R  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.diffusion import diffusion_map, maps  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
n_base = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
D, K, COMPS, TOL = 20, 15, 15, 1e-10
# MI355X figures: peak FP32 vector 157.3 TFLOPS = 7.86e13 lane-instructions / s (256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz);
# fp64 vector instructions are taken at half that rate (AMD's specification: 78.6 TFLOPS fp64 vector).  HBM 8.0 TB/s peak,
# 6.29 TB/s measured with a copy kernel.
FP32_LANE_INSTR = 157.3e12 / 2
FP64_LANE_INSTR = FP32_LANE_INSTR / 2
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
OUT = os.path.join(ROOT, "profiles", "diffusion_1m.json")
ctx = _lib.default_context(0)


def say(*a):
    print(*a, flush=True)


def timed(fn, *a, **kw):
    ctx.sync()
    t = time.perf_counter()
    r = fn(*a, **kw)
    ctx.sync()
    return time.perf_counter() - t, r


def adata(X):
    return SimpleAnnData(np.zeros((X.shape[0], 1)), obsm={"X_rep": X})


def write(out):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


X, _ = R.traj(n, D, 1)
say(f"input: {n} x {D}")
diffusion_map(adata(X[:4096]), "X_rep", n_neighbors=K, n_comps=COMPS)        # code objects, allocations
wall, ad = timed(diffusion_map, adata(X), "X_rep", n_neighbors=K, n_comps=COMPS, tol=TOL)
info = ad.uns["diffmap"]
say(f"public call {wall:.2f} s, {info['n_steps']} steps, worst residual {info['residuals'].max():.2e}")

ctx.reset_timers()
t_search, _ = timed(ctx.knn_dense, X, K, fetch=False)
t_graph, ginfo = timed(ctx.diffmap_graph)
mem_graph = ctx.device_mem()
cap = info["params"]["max_basis"]
t_eig, (lam, vecs, res, steps) = timed(maps._eigenpairs, ctx, n, COMPS, TOL, cap, 0)
kern = {what: ctx.kernel_time(kid) for what, kid in (("search", _lib.K_DIFF_KNN), ("graph", _lib.K_DIFF_GRAPH),
                                                     ("spmv", _lib.K_DIFF_SPMV), ("orthogonalisation", _lib.K_DIFF_ORTH))}
np.testing.assert_array_equal(lam, ad.uns["diffmap_evals"])          # the parts are the call
np.testing.assert_array_equal(vecs, ad.obsm["X_diffmap"])
dp = -(-D // 8) * 8
search_s, orth_s = kern["search"][0] * 1e-3, kern["orthogonalisation"][0] * 1e-3
orth_bytes = sum(4 * (j + 1) * 8 * n for j in range(steps))
out = {
    "workload": f"{n} cells x {D} features (tests/diffusion_restated.py traj, seed 1), n_neighbors = {K}, n_comps = {COMPS}, "
                f"tol = {TOL:g}; one small warm-up call, then one timed call",
    "public_call_s": wall, "n_steps": int(steps), "max_basis": int(cap), "worst_true_residual": float(res.max()),
    "eigenvalues": [float(v) for v in lam], "n_edges": int(ginfo["n_edges"]),
    "search_call_s": t_search, "graph_call_s": t_graph, "eigensolver_s": t_eig,
    "kernel_ms": {k: v[0] for k, v in kern.items()}, "kernel_scopes": {k: v[1] for k, v in kern.items()},
    "per_step_ms": {"spmv": kern["spmv"][0] / steps, "orthogonalisation": kern["orthogonalisation"][0] / steps},
    "device_mem_bytes": {"after_graph": int(mem_graph), "lanczos_basis": int((cap + 1) * n * 8)},
    "search_roofline": {
        "lane_instructions_3d_per_pair": 3.0 * D * n * n, "lane_instructions_issued_padded_d": 3.0 * dp * n * n,
        "fp64_lane_instructions_per_s_peak": FP64_LANE_INSTR, "fp32_vector_tflops_in_guide": 157.3,
        "fraction_of_fp64_issue_peak": 3.0 * D * n * n / search_s / FP64_LANE_INSTR,
        "fraction_of_fp64_issue_peak_padded_d": 3.0 * dp * n * n / search_s / FP64_LANE_INSTR},
    "orthogonalisation_roofline": {
        "bytes_4_j_8n_summed": orth_bytes, "bytes_per_s": orth_bytes / orth_s,
        "fraction_of_hbm_peak_8_0": orth_bytes / orth_s / HBM_PEAK, "fraction_of_hbm_copy_6_29": orth_bytes / orth_s / HBM_COPY},
}
write(out)
say(json.dumps(out, indent=1))

# ---- the same pipeline on the host, at n_base cells ---------------------------------------------------------------------
from scipy.sparse.linalg import eigsh  # noqa: E402
from sklearn.neighbors import NearestNeighbors  # noqa: E402

Xb = X[:n_base]
t = time.perf_counter()
ref = NearestNeighbors(n_neighbors=K + 1, algorithm="kd_tree", n_jobs=-1).fit(Xb).kneighbors(Xb, return_distance=False)
t_tree = time.perf_counter() - t
say(f"kd_tree at {n_base} cells: {t_tree:.1f} s")
idx = ref[:, 1:].astype(np.int32)
t = time.perf_counter()
d2 = R.pair_d2(Xb, np.repeat(np.arange(n_base), K), idx.ravel()).reshape(n_base, K)
indptr, indices = R.union_edges(idx)
T = R.transition(indptr, indices, R.kernel_weights(Xb, indptr, indices, R.scales(d2)))[0]
t_host_graph = time.perf_counter() - t
t = time.perf_counter()
lam_b, _ = eigsh(sparse.csr_matrix((T, indices, indptr), shape=(n_base, n_base)), k=COMPS, which="LA", tol=TOL, v0=np.ones(n_base))
t_eigsh = time.perf_counter() - t
say(f"numpy graph {t_host_graph:.1f} s, eigsh {t_eigsh:.1f} s")
scale = n / n_base
out["host_baseline"] = {
    "cells": n_base, "kd_tree_s": t_tree, "numpy_graph_s": t_host_graph, "eigsh_s": t_eigsh, "extrapolated": True,
    "total_s_extrapolated_to_n": (t_tree * scale * np.log(n) / np.log(n_base) + (t_host_graph + t_eigsh) * scale),
    "note": "kd_tree scaled as n log n, graph and eigsh linearly: a lower bound for the host at n cells",
}
out["speedup_vs_extrapolated_host"] = out["host_baseline"]["total_s_extrapolated_to_n"] / wall
write(out)
say(json.dumps(out["host_baseline"], indent=1))
