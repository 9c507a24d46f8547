"""The exact neighbour search at 10^6 cells of the bench's synthetic counts: pca (64 components, normalize=True), the scores
truncated to d = 20, 32, 40, 50, 64, k = 15.  Per d: sc_knn_dense (path 1) once and the certified Gram-form filter
(path 2) three times, with the `info` counts of every run and a digest of the lists (the two paths must agree); what
path 0 picks.  Then pca (50) -> neighbors -> louvain(graph="connectivities") and diffusion_map(graph="connectivities")
against the two calls with graph=None, each of which runs the same search and graph step again.

Every GPU step is a child process under its own time limit (the path 1 limits are sized from the 57 s on record at 50
features: three times the time scaled by d / 50); a step that fails or runs out of time ends the probe.  Writes
profiles/neighbors_1m.json (or the path given last).

Usage:  python scripts/neighbors_probe.py [n_cells [n_genes [parts [out.json]]]]     parts: search, pipeline or both"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIMS = (20, 32, 40, 50, 64)
NEIGHBORS = 15
FP64_MATRIX_PEAK = 78.6e12     # flop / s, MI355X data sheet


def say(*a):
    print(*a, flush=True)


def timed(ctx, fn, *a, **kw):
    ctx.sync()
    t = time.perf_counter()
    r = fn(*a, **kw)
    ctx.sync()
    return time.perf_counter() - t, r


def counts(n, G):
    import bench
    from scipy import sparse

    _, dense = bench.synth_inputs(n, G, seed=42)
    return sparse.csr_matrix(dense)


# ---- the steps (child processes) ------------------------------------------------------------------------------------------
def step_scores(n, G, path):
    from spatialcore_amd import SimpleAnnData, _lib
    from spatialcore_amd.pca import pca

    ctx = _lib.default_context(0)
    ad = SimpleAnnData(counts(n, G), var_names=[f"g{i}" for i in range(G)])
    t, _ = timed(ctx, pca, ad, max(DIMS), normalize=True)
    np.save(path, np.ascontiguousarray(ad.obsm["X_pca"], dtype=np.float64))
    return {"pca_s": t}


def step_search(scores, d, path, reps):
    from spatialcore_amd import _lib

    ctx = _lib.default_context(0)
    R = np.ascontiguousarray(np.load(scores)[:, :d])
    n = R.shape[0]
    ctx.knn_dense_gram(R[:4096], NEIGHBORS, path=path)      # code objects, allocations
    runs = []
    for _ in range(reps):
        ctx.reset_timers()
        t, (idx, d2, info) = timed(ctx, ctx.knn_dense_gram, R, NEIGHBORS, True, path)
        ms, _ = ctx.kernel_time(_lib.K_NEIGHBORS_GRAM if path == 2 else _lib.K_DIFF_KNN)
        digest = hashlib.sha1(idx.tobytes() + d2.tobytes()).hexdigest()
        runs.append({"call_s": t, "kernels_ms": ms, "info": info, "lists_sha1": digest})
        say(f"d={d} path={path}: {t:.2f} s (kernels {ms:.0f} ms), {info}")
    chosen = None
    if path == 2:      # what path 0 picks at this (n, d): one more call, whose info says which path ran
        t, (_, _, info) = timed(ctx, ctx.knn_dense_gram, R, NEIGHBORS, False, 0)
        chosen = {"path": info["path"], "call_s": t}
    return {"n": n, "d": d, "path": path, "runs": runs, "path_0_takes": chosen}


def step_pipeline(n, G):
    from spatialcore_amd import SimpleAnnData, _lib
    from spatialcore_amd.cluster import louvain
    from spatialcore_amd.diffusion import diffusion_map
    from spatialcore_amd.neighbors import neighbors
    from spatialcore_amd.pca import pca

    ctx = _lib.default_context(0)
    X = counts(n, G)
    names = [f"g{i}" for i in range(G)]
    ad = SimpleAnnData(X, var_names=names)
    t_pca, _ = timed(ctx, pca, ad, 50, normalize=True)
    small = SimpleAnnData(X[:4096], var_names=names)      # code objects, allocations
    small.obsm["X_pca"] = np.ascontiguousarray(ad.obsm["X_pca"][:4096])
    neighbors(small, NEIGHBORS)
    louvain(small, graph="connectivities")
    louvain(small, n_neighbors=NEIGHBORS)
    out = {"pca_s": t_pca}

    def attempt(name, fn, *a, **kw):
        try:
            t, _ = timed(ctx, fn, *a, **kw)
            out[name] = t
            say(f"{name}: {t:.2f} s")
        except (ValueError, RuntimeError) as e:
            # a property of the data (a disconnected graph, Lanczos out of basis) is recorded and the next stage runs; a failure
            # of the device or of its memory is not: it ends this process, and with it the probe, before anything else starts
            if isinstance(e, _lib.SpatialCoreHipError):
                raise
            out[name] = None
            out[name + "_error"] = str(e)[:200]
            say(f"{name}: {e}")

    attempt("neighbors_s", neighbors, ad, NEIGHBORS)
    out["search"] = ad.uns["neighbors"]["search"]
    attempt("louvain_on_stored_graph_s", louvain, ad, graph="connectivities")
    attempt("diffusion_map_on_stored_graph_s", diffusion_map, ad, graph="connectivities")
    other = SimpleAnnData(X, var_names=names)
    other.obsm["X_pca"] = ad.obsm["X_pca"]
    attempt("louvain_own_search_s", louvain, other, n_neighbors=NEIGHBORS)
    attempt("diffusion_map_own_search_s", diffusion_map, other, use_rep="X_pca", n_neighbors=NEIGHBORS)
    if out["louvain_on_stored_graph_s"] is not None and out["louvain_own_search_s"] is not None:
        out["louvain_labels_equal"] = bool(np.array_equal(np.asarray(ad.obs["louvain"].cat.codes),
                                                          np.asarray(other.obs["louvain"].cat.codes)))
    return out


# ---- the driver ---------------------------------------------------------------------------------------------------------
def child(limit, *args):
    """One step in a fresh process under its own time limit; its last output line is the step's JSON record."""
    say(f"--- step {' '.join(map(str, args))} (limit {limit} s)")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", *map(str, args)], stdout=subprocess.PIPE, timeout=limit,
                       check=True, text=True)
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    return json.loads(r.stdout.strip().splitlines()[-1])


def write(out, out_path):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    parts = sys.argv[3] if len(sys.argv) > 3 else "both"
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "neighbors_1m.json")
    scale = (n / 1e6) ** 2
    out = {"workload": f"{n} cells x {G} genes of bench.synth_inputs(seed=42) -> pca(64, normalize=True), scores truncated to d, "
                       f"k = {NEIGHBORS}; every step a fresh process: one warm-up call on 4096 rows, then the timed calls",
           "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "fp64_matrix_peak_source": "data sheet, not measured"}
    if os.path.exists(out_path):      # the two parts may be measured by two invocations
        with open(out_path) as f:
            old = json.load(f)
        if old.get("workload") == out["workload"]:
            out = old
    with tempfile.TemporaryDirectory() as tmp:
        if parts in ("search", "both"):
            scores = os.path.join(tmp, "scores.npy")
            out["pca_64_s"] = child(600, "scores", n, G, scores)["pca_s"]
            rows = []
            for d in DIMS:
                direct = child(int(60 + 3 * 57.2 * scale * d / 50), "search", scores, d, 1, 1)
                gram = child(int(60 + 3 * 57.2 * scale * d / 50), "search", scores, d, 2, 3)
                t1 = direct["runs"][0]["call_s"]
                t2 = [r["call_s"] for r in gram["runs"]]
                dp = -(-d // 8) * 8
                row = {"d": d, "padded_d": dp, "path_1_s": t1, "path_2_s": t2, "path_2_spread_s": max(t2) - min(t2),
                       "path_2_faster_by_s": t1 - max(t2), "path_1_info": direct["runs"][0]["info"],
                       "path_2_info": [r["info"] for r in gram["runs"]], "path_2_kernels_ms": [r["kernels_ms"] for r in gram["runs"]],
                       "lists_equal": all(r["lists_sha1"] == direct["runs"][0]["lists_sha1"] for r in gram["runs"]),
                       "path_0": gram["path_0_takes"],
                       "gram_flop": 2.0 * n * n * dp,
                       "path_2_fraction_of_fp64_matrix_peak": 2.0 * n * n * dp / (min(r["kernels_ms"] for r in gram["runs"]) * 1e-3)
                       / FP64_MATRIX_PEAK}
                row["path_0_picks_the_faster"] = row["path_0"]["path"] == (2 if max(t2) < t1 else 1)
                rows.append(row)
                say(json.dumps(row))
            out["search"] = rows
            write(out, out_path)
        if parts in ("pipeline", "both"):
            out["pipeline"] = child(int(300 + 400 * scale), "pipeline", n, G)
    write(out, out_path)
    say(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        a = sys.argv[3:]
        if sys.argv[2] == "scores":
            rec = step_scores(int(a[0]), int(a[1]), a[2])
        elif sys.argv[2] == "search":
            rec = step_search(a[0], int(a[1]), int(a[2]), int(a[3]))
        else:
            rec = step_pipeline(int(a[0]), int(a[1]))
        say(json.dumps(rec))
    else:
        main()
