"""fit_spatial_nmf at 10^6 cells x 500 genes of the bench's synthetic counts, K = 20, 200 iterations (tol = 0), on the
kNN-union graphs of the bench's coordinates with k = 6 and k = 15, and, in the same job, fit_nmf (Frobenius) on the same
input.  Each is run three times after one small warm-up call.  Per run: the public call's wall time and the HIP-event
times of the kernel families it used (sc_ctx_kernel_time; the graph form runs under fit_nmf's ids: the W pass under
SC_K_NMF_W, the penalty inside SC_K_NMF_ERR).  Once per k: the host's time for the graph (the device search with its
read-back, and the union).  Derived: the W pass per iteration with and without the graph term, the penalty per check as
the difference of one evaluation with and without it, and the rate of the added gather (stored graph entries x K x 8
bytes per iteration) over the added W-pass time, against the guide's row-gather figure for a table of this size.
Writes profiles/spatial_nmf_1m.json.

Usage:  python scripts/spatial_nmf_probe.py [n_cells [n_genes [out.json]]]"""
import json
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.nmf import fit_nmf, fit_spatial_nmf  # noqa: E402
from spatialcore_amd.nmf.spatial import union_of_knn  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 500
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "spatial_nmf_1m.json")
K, ITERS, REPS, ALPHA = 20, 200, 3, 1.0
GUIDE_GATHER = (7.4e12, 7.9e12)   # bytes / s: uniformly random 1,152-byte rows of a 151 MB table (Infinity Cache), chip-wide
ctx = _lib.default_context(0)


def say(*a):
    print(*a, flush=True)


t0 = time.perf_counter()
coords, dense = bench.synth_inputs(n, G, seed=42)
X = sparse.csr_matrix(dense)
del dense
coords = np.ascontiguousarray(coords, dtype=np.float64)
names = [f"g{i}" for i in range(G)]
say(f"input: {n} x {G}, {X.nnz} stored entries ({time.perf_counter() - t0:.1f} s)")
FAMILIES = (("setup", _lib.K_NMF_SETUP), ("w_pass", _lib.K_NMF_W), ("h_pass", _lib.K_NMF_H), ("error", _lib.K_NMF_ERR),
            ("knn", _lib.K_KNN))


def adata(rows=None):
    if rows is None:
        return SimpleAnnData(X, var_names=names, obsm={"spatial": coords})
    return SimpleAnnData(X[:rows], var_names=names, obsm={"spatial": coords[:rows]})


def timed(fn, *a, **kw):
    ctx.sync()
    ctx.reset_timers()
    t = time.perf_counter()
    r = fn(*a, **kw)
    ctx.sync()
    wall = time.perf_counter() - t
    kern = {what: ctx.kernel_time(kid) for what, kid in FAMILIES}
    return wall, {k: v[0] for k, v in kern.items()}, {k: v[1] for k, v in kern.items()}, r


def runs(fn, key, **kw):
    fn(adata(4096), K, max_iter=2, tol=0.0, **kw)      # code objects, allocations
    out = []
    for rep in range(REPS):
        wall, ms, scopes, ad = timed(fn, adata(), K, max_iter=ITERS, tol=0.0, random_state=0, **kw)
        info = ad.uns[key]
        evals = scopes["error"]
        out.append({"public_call_s": wall, "kernel_ms": ms, "kernel_scopes": scopes,
                    "w_pass_ms_per_iteration": ms["w_pass"] / ITERS, "h_pass_ms_per_iteration": ms["h_pass"] / ITERS,
                    "error_evaluations": evals, "error_ms_per_evaluation": ms["error"] / evals,
                    "n_iter": info["n_iter"], "reconstruction_err": info["reconstruction_err"],
                    "penalty": info.get("penalty"), "graph": info.get("graph")})
        say(f"{key} {kw.get('n_neighbors', '')} run {rep}: {wall:.2f} s, W pass {ms['w_pass'] / ITERS:.3f} ms / iteration, "
            f"H pass {ms['h_pass'] / ITERS:.3f}, one evaluation {ms['error'] / evals:.2f} ms")
    return out


def median(rs, key):
    return float(np.median([r[key] for r in rs]))


def graph_host(k):
    t = time.perf_counter()
    lists = ctx.knn(coords, k)
    t_search = time.perf_counter() - t
    t = time.perf_counter()
    A = union_of_knn(lists, None, n)
    return {"search_and_read_back_s": t_search, "union_s": time.perf_counter() - t, "stored_entries": int(A.nnz)}


out = {"workload": f"{n} cells x {G} genes of bench.synth_inputs(seed=42) (float32 counts) on its coordinates, {int(X.nnz)} stored "
                   f"entries, K = {K}, {ITERS} iterations, tol = 0, init='random' (random_state=0), spatial_alpha = {ALPHA}; one "
                   f"small warm-up call, then {REPS} timed calls each; medians under 'summary'",
       "stored_entries": int(X.nnz), "guide_row_gather_bytes_per_s": list(GUIDE_GATHER), "all_figures": "measured"}
out["fit_nmf_frobenius"] = plain = runs(fit_nmf, "nmf", beta_loss="frobenius")
w_plain, e_plain = median(plain, "w_pass_ms_per_iteration"), median(plain, "error_ms_per_evaluation")
out["summary"] = {"fit_nmf_frobenius": {"public_call_s": median(plain, "public_call_s"), "w_pass_ms_per_iteration": w_plain,
                                        "h_pass_ms_per_iteration": median(plain, "h_pass_ms_per_iteration"),
                                        "error_ms_per_evaluation": e_plain}}
for k in (6, 15):
    host = graph_host(k)
    rs = runs(fit_spatial_nmf, "spatial_nmf", spatial_alpha=ALPHA, n_neighbors=k)
    out[f"fit_spatial_nmf_k{k}"] = rs
    w, e = median(rs, "w_pass_ms_per_iteration"), median(rs, "error_ms_per_evaluation")
    gather = host["stored_entries"] * K * 8
    added_ms = w - w_plain
    out["summary"][f"fit_spatial_nmf_k{k}"] = {
        "public_call_s": median(rs, "public_call_s"), "graph_host": host,
        "w_pass_ms_per_iteration": w, "w_pass_added_ms_per_iteration": added_ms,
        "h_pass_ms_per_iteration": median(rs, "h_pass_ms_per_iteration"),
        "error_ms_per_evaluation": e, "penalty_ms_per_check_by_difference": e - e_plain,
        "gathered_w_row_bytes_per_iteration": gather,
        "gather_bytes_per_s_over_added_time": gather / (added_ms * 1e-3) if added_ms > 0 else None,
        "fraction_of_guide_row_gather": [gather / (added_ms * 1e-3) / g for g in GUIDE_GATHER] if added_ms > 0 else None}
out["device_mem_bytes"] = ctx.device_mem()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
say(json.dumps(out["summary"], indent=1))
