"""aggregate_neighbors at 10^6 cells of the bench's coordinates: X_pca (pca of the bench's synthetic counts, 50 components,
normalize=True, float64) truncated to d = 16 and d = 50, on the kNN-union graphs with k = 6 and k = 15, L = 3.

Per (k, d): the public call's wall time (one small warm-up call, then REPS calls), and, from one walk through the C ABI
(sc_hop_begin / _next / _aggregate with sc_hop_times' HIP-event times), per hop: the expansion's count (the bound kernel
and the host's classing of the rows included), fill and sort, the aggregate kernel, the shell's size, and the aggregate's
gathered bytes (stored entries of the shell x d x 8) over its time -- beside the rates profiles/spatial_nmf_1m.json
records for the W gather of fit_spatial_nmf on the same graphs.  Once per k: the host's time for the graph, and the scipy
textbook (tests/hops_restated.py: shells_textbook, textbook) on the first 50,000 cells, scaled to n by the cell count.
Writes profiles/hops_1m.json.

Usage:  python scripts/hops_probe.py [n_cells [out.json]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import hops_restated as R  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd._spatial_graph import knn_union_graph  # noqa: E402
from spatialcore_amd.pca import pca  # noqa: E402
from spatialcore_amd.spatial import aggregate_neighbors  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "hops_1m.json")
G, L, REPS, N_TEXTBOOK = 500, 3, 3, 50_000
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


def adata(X, rows=None):
    rows = n if rows is None else rows
    return SimpleAnnData(np.zeros((rows, 1)), var_names=["g"], obsm={"spatial": coords[:rows], "X_pca": X[:rows]})


def walk(A, X):
    """One pass through the C ABI: per hop the phases of the expansion and one mean."""
    hops = []
    t = time.perf_counter()
    ctx.hop_begin(A.indptr, A.indices, n)
    begin_s = time.perf_counter() - t
    try:
        entries, longest = int(A.nnz), int(np.diff(A.indptr).max())
        for l in range(1, L + 1):
            hop = {"shell": l}
            if l > 1:
                t = time.perf_counter()
                entries, longest, _ = ctx.hop_next()
                hop["next_call_s"] = time.perf_counter() - t
                times = ctx.hop_times()
                hop.update({"count_ms": times["count"], "fill_ms": times["fill"], "sort_ms": times["sort"]})
            t = time.perf_counter()
            ctx.hop_aggregate(X, "mean")
            hop["aggregate_call_s"] = time.perf_counter() - t      # the first one uploads X; every one copies n x d back
            ms = ctx.hop_times()["aggregate"]
            gathered = entries * X.shape[1] * 8
            hop.update({"stored_entries": entries, "largest_row": longest, "aggregate_kernel_ms": ms, "gathered_bytes": gathered,
                        "gather_bytes_per_s": gathered / (ms * 1e-3)})
            hops.append(hop)
            say("   ", hop)
        mem = ctx.device_mem()
    finally:
        ctx.hop_end()
    return {"begin_call_s": begin_s, "hops": hops, "device_mem_bytes": mem}


def textbook_scaled(k, X):
    m = min(N_TEXTBOOK, n)
    A = R.knn_union(coords[:m], k)
    t = time.perf_counter()
    shells = R.shells_textbook(A, L)
    t_shells = time.perf_counter() - t
    t = time.perf_counter()
    for S in shells:
        R.textbook(S, X[:m])
    t_agg = time.perf_counter() - t
    return {"cells": m, "shells_s": t_shells, "aggregates_s": t_agg, "scaled_to_n_s": (t_shells + t_agg) * n / m,
            "scaling": "by the cell count: a kNN-union graph's shells grow with the cells, not with their density"}


try:
    with open(os.path.join(ROOT, "profiles", "spatial_nmf_1m.json")) as f:
        w_gather = {k: v.get("gather_bytes_per_s_over_added_time") for k, v in json.load(f)["summary"].items() if "spatial" in k}
except OSError:
    w_gather = None

out = {"workload": f"{n} cells on bench.synth_inputs(seed=42)'s coordinates; X_pca = pca(50, normalize=True, float64) of its {G}-gene counts, "
                   f"truncated to d; kNN-union graphs; aggregate_neighbors(n_layers={L}, aggregations='mean'); one small warm-up call, "
                   f"then {REPS} timed calls, the median under 'public_call_s'",
       "all_figures": "measured", "w_gather_bytes_per_s_of_fit_spatial_nmf": w_gather, "runs": {}}
for k in (6, 15):
    t = time.perf_counter()
    A = knn_union_graph(ctx, coords, [(None, None)], k, n)
    graph_s = time.perf_counter() - t
    entry = {"graph_host_s": graph_s, "stored_entries": int(A.nnz)}
    for d in (16, 50):
        X = np.ascontiguousarray(scores[:, :d])
        aggregate_neighbors(adata(X, 4096), n_layers=L, n_neighbors=k)      # code objects, allocations
        calls = []
        for _ in range(REPS):
            ctx.sync()
            t = time.perf_counter()
            res = aggregate_neighbors(adata(X), n_layers=L, n_neighbors=k)
            calls.append(time.perf_counter() - t)
        say(f"k = {k}, d = {d}: public call {np.median(calls):.2f} s, shells {res.uns['X_cellcharter']['shell_entries']}")
        entry[f"d{d}"] = {"public_call_s": float(np.median(calls)), "public_calls_s": calls,
                          "shell_entries": res.uns["X_cellcharter"]["shell_entries"], "shell_max": res.uns["X_cellcharter"]["shell_max"],
                          **walk(A, X)}
        del res
    entry["scipy_textbook_d16"] = textbook_scaled(k, scores[:, :16])
    say(f"k = {k}: scipy textbook {entry['scipy_textbook_d16']}")
    out["runs"][f"k{k}"] = entry
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
say("written", OUT)
