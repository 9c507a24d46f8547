"""The UMAP steps at 10^6 cells of the bench's synthetic counts: pca (50 components, normalize=True) ->
neighbors(method="umap", 15) -> umap (200 epochs), the public calls timed by a host clock around calls that end in a device
synchronise.  Then, on the same neighbour lists, sc_fuzzy_graph beside sc_diffmap_graph (alternating, three times each);
the layout kernel's time at the first, the middle and the last epoch (one-epoch calls on the resident graph, the launch
that finds w_max measured by an empty range and taken off) and over all epochs in one call; the firings per epoch and the longest row; the achieved
interaction rate against the two bounds that apply.  As a CPU figure the numpy restatement (tests/umap_restated.py) is timed
at 50,000 cells on the same host, on the lists the device found, and scaled linearly; umap-learn is not installed.

`--tolerances` measures instead the largest difference between the device and the restatement over every input of
tests/test_gpu_umap.py ("tolerances") and of tests/test_gpu_umap_edges.py ("tolerances_edges"): the figures those files'
assertions are ten times of.

Every GPU step is a child process under its own time limit; a step that fails or runs out of time ends the probe.  Writes
profiles/umap_1m.json (or the path given last); the two modes fill two sections of the same file.

Usage:  python scripts/umap_probe.py [n_cells [n_genes [out.json]]]
        python scripts/umap_probe.py --tolerances [out.json]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEIGHBORS, EPOCHS, NEG, CPU_CELLS = 15, 200, 5, 50_000
# the two bounds of the layout kernel, per interaction (one attraction or one repulsion)
FP64_VECTOR_PEAK = 78.6e12 / 2      # fp64 vector instructions x lanes per second (data sheet: 78.6 Tflop/s with an FMA as two)
FP64_OPS_PER_INTERACTION = 120      # v_*_f64 instructions in k_um_epoch<2>'s ISA (612) over its five inlined interactions
LINE_BYTES = 128                    # a 16-byte position row costs one cache line
INFINITY_CACHE_GATHER = 8.6e12      # bytes / s, uniformly random rows of a table beyond an XCD's L2 (MI355X measurements)


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


def restated():
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import diffusion_restated as R
    import umap_restated as U

    return R, U


# ---- the steps (child processes) ------------------------------------------------------------------------------------------
def step_tolerances():
    from spatialcore_amd import _lib

    R, U = restated()
    ctx = _lib.default_context(0)
    normal = 1e-300
    out = {"sigma": 0.0, "w": 0.0, "layout_of_extent_10": 0.0, "cases": {}}

    def rel(got, ref):
        big = ref >= normal
        return float(np.max(np.abs(got[big] - ref[big]) / ref[big])) if big.any() else 0.0

    for name, (X, k) in U.fuzzy_recipes().items():
        idx, d2 = R.knn(X, k)
        g = U.fuzzy_graph(idx, d2)
        ctx.knn_dense(X, k, fetch=False)
        info = ctx.fuzzy_graph()
        _, _, w = ctx.diffmap_graph_get()
        rec = {"sigma": rel(info["sigma"], g["sigma"]), "w": rel(w, g["w"]), "rho_equal": bool(np.array_equal(info["rho"], g["rho"]))}
        out["cases"][name] = rec
        out["sigma"], out["w"] = max(out["sigma"], rec["sigma"]), max(out["w"], rec["w"])
        say(name, rec)
    for name, (graph, Y0, neg) in U.layout_recipes().items():
        ref, worst = Y0, 0.0
        for e1 in (1, 2, 3):
            ref = U.layout(*graph, ref, 10, e1 - 1, e1, neg=neg, seed=11)
            got = ctx.umap_layout(graph, Y0, U.A_DEFAULT, U.B_DEFAULT, 1.0, 1.0, neg, 10, 11, 0, e1)
            worst = max(worst, float(np.max(np.abs(got - ref))) / 10.0)
        out["cases"][name] = {"layout_of_extent_10": worst}
        out["layout_of_extent_10"] = max(out["layout_of_extent_10"], worst)
        say(name, worst)
    return out


def step_tolerances_edges():
    """The same over ``fuzzy_edge_recipes`` and ``layout_edge_recipes`` (tests/test_gpu_umap_edges.py): sigma over the
    rows with rho > 0 (the others are compared by bytes), the positions over every case's own extent and epochs."""
    from spatialcore_amd import _lib

    R, U = restated()
    ctx = _lib.default_context(0)
    normal = 1e-300
    out = {"sigma": 0.0, "w": 0.0, "layout_of_extent": 0.0, "set_by": {}, "cases": {}}

    def rel(got, ref):
        big = ref >= normal
        return float(np.max(np.abs(got[big] - ref[big]) / ref[big])) if big.any() else 0.0

    def record(name, rec):
        out["cases"][name] = rec
        for key in ("sigma", "w", "layout_of_extent"):
            if rec.get(key, 0.0) > out[key]:
                out[key], out["set_by"][key] = rec[key], name
        say(name, rec)

    for name, (X, k) in U.fuzzy_edge_recipes().items():
        idx, d2 = R.knn(X, k)
        g = U.fuzzy_graph(idx, d2)
        ctx.knn_dense(X, k, fetch=False)
        info = ctx.fuzzy_graph()
        _, _, w = ctx.diffmap_graph_get()
        zero = g["rho"] == 0
        record(name, {"sigma": rel(info["sigma"][~zero], g["sigma"][~zero]), "w": rel(w, g["w"]),
                      "rho_equal": bool(np.array_equal(info["rho"], g["rho"])), "rows_with_rho_0": int(zero.sum()),
                      "their_sigma_equal": bool(info["sigma"][zero].tobytes() == g["sigma"][zero].tobytes())})
    for name, case in U.layout_edge_recipes().items():
        run, worst = case["run"], 0.0
        for e1, ref in U.layout_case_epochs(case):
            got = ctx.umap_layout(case["graph"], case["Y0"], run["a"], run["b"], run["gamma"], 1.0, run["neg"], run["n_epochs"],
                                  run["seed"], run["e0"], e1)
            worst = max(worst, float(np.max(np.abs(got - ref))) / case["extent"])
        record(name, {"layout_of_extent": worst, "extent": case["extent"]})
    return out


def step_pipeline(n, G):
    from spatialcore_amd import SimpleAnnData, _lib
    from spatialcore_amd.embedding import umap
    from spatialcore_amd.neighbors import neighbors
    from spatialcore_amd.pca import pca

    ctx = _lib.default_context(0)
    X = counts(n, G)
    names = [f"g{i}" for i in range(G)]
    ad = SimpleAnnData(X, var_names=names)
    out = {}
    out["pca_s"], _ = timed(ctx, pca, ad, 50, normalize=True)
    small = SimpleAnnData(X[:4096], var_names=names)      # code objects, allocations
    small.obsm["X_pca"] = np.ascontiguousarray(ad.obsm["X_pca"][:4096])
    neighbors(small, NEIGHBORS, method="umap")
    umap(small, n_epochs=5)
    out["neighbors_umap_s"], _ = timed(ctx, neighbors, ad, NEIGHBORS, method="umap")
    say(f"neighbors(method='umap'): {out['neighbors_umap_s']:.2f} s")
    ctx.reset_timers()
    out["umap_s"], _ = timed(ctx, umap, ad, n_epochs=EPOCHS)
    out["umap_layout_kernels_ms"] = ctx.kernel_time(_lib.K_UMAP_LAYOUT)[0]
    say(f"umap: {out['umap_s']:.2f} s, layout kernels {out['umap_layout_kernels_ms']:.0f} ms")
    Y = ad.obsm["X_umap"]
    out["extent"] = float(np.abs(Y).max())
    p = ad.uns["umap"]["params"]

    # the two graphs on the same lists
    R = np.ascontiguousarray(ad.obsm["X_pca"])
    ctx.knn_dense_gram(R, NEIGHBORS, fetch=False)
    runs = {"diffmap": [], "fuzzy": []}
    for _ in range(3):
        for what, fn, kid in (("diffmap", ctx.diffmap_graph, _lib.K_DIFF_GRAPH), ("fuzzy", ctx.fuzzy_graph, _lib.K_UMAP_GRAPH)):
            ctx.reset_timers()
            t, _ = timed(ctx, fn)
            runs[what].append({"call_s": t, "kernels_ms": ctx.kernel_time(kid)[0]})
    out["graphs_on_the_same_lists"] = runs
    out["fuzzy_over_diffmap_kernels"] = min(r["kernels_ms"] for r in runs["fuzzy"]) / min(r["kernels_ms"] for r in runs["diffmap"])
    say(json.dumps(runs), out["fuzzy_over_diffmap_kernels"])

    # the layout kernel, epoch by epoch, on the resident fuzzy graph
    indptr, _, w = ctx.diffmap_graph_get()
    out["stored_entries"], out["max_row_degree"] = int(w.size), int(np.diff(indptr).max())
    Y0 = R[:, :2] * (10.0 / np.abs(R[:, :2]).max())
    r = w / w.max()

    def kernels_ms(e0, e1):
        ctx.reset_timers()
        ctx.umap_layout(None, Y0, p["a"], p["b"], 1.0, 1.0, NEG, EPOCHS, 0, e0, e1)
        return ctx.kernel_time(_lib.K_UMAP_LAYOUT)[0]

    kernels_ms(0, 1)
    wmax_ms = min(kernels_ms(7, 7) for _ in range(3))
    out["w_max_launch_ms"] = wmax_ms
    out["all_epochs_kernels_ms"] = min(kernels_ms(0, EPOCHS) for _ in range(2))
    epochs = []
    for e in (0, EPOCHS // 2, EPOCHS - 1):
        ms = min(kernels_ms(e, e + 1) for _ in range(3)) - wmax_ms
        fire = int(np.sum(np.floor((e + 1.0) * r) > np.floor(float(e) * r)))
        inter = fire * (1 + NEG)
        rate = inter / (ms * 1e-3)
        fp64_bound, gather_bound = FP64_VECTOR_PEAK / FP64_OPS_PER_INTERACTION, INFINITY_CACHE_GATHER / LINE_BYTES
        epochs.append({"epoch": e, "kernel_ms": ms, "firings": fire, "interactions": inter, "interactions_per_s": rate,
                       "fraction_of_fp64_vector_bound": rate / fp64_bound, "fraction_of_gather_bound": rate / gather_bound,
                       "nearer_bound": "gather" if gather_bound < fp64_bound else "fp64"})
        say(json.dumps(epochs[-1]))
    out["epochs"] = epochs
    out["bounds"] = {"fp64_vector_interactions_per_s": FP64_VECTOR_PEAK / FP64_OPS_PER_INTERACTION,
                     "gather_interactions_per_s": INFINITY_CACHE_GATHER / LINE_BYTES,
                     "note": "fp64: data-sheet vector rate over the static count of fp64 instructions per interaction; gather: one "
                             "128-byte line per 16-byte position at the measured Infinity Cache gather rate; the lower one applies"}
    return out


def step_cpu(n, G):
    """The numpy restatement at `n` cells, on the lists the device found for them."""
    from spatialcore_amd import SimpleAnnData, _lib
    from spatialcore_amd.pca import pca

    _, U = restated()
    ctx = _lib.default_context(0)
    ad = SimpleAnnData(counts(n, G), var_names=[f"g{i}" for i in range(G)])
    pca(ad, 50, normalize=True)
    R = np.ascontiguousarray(ad.obsm["X_pca"])
    idx, d2, _ = ctx.knn_dense_gram(R, NEIGHBORS)
    t = time.perf_counter()
    g = U.fuzzy_graph(idx, d2)
    out = {"cells": n, "numpy_fuzzy_graph_s": time.perf_counter() - t}
    Y0 = R[:, :2] * (10.0 / np.abs(R[:, :2]).max())
    picks = (0, EPOCHS // 2, EPOCHS - 1)
    t = time.perf_counter()
    for e in picks:
        U.epoch(g["indptr"], g["indices"], g["w"], Y0, e, EPOCHS, U.A_DEFAULT, U.B_DEFAULT, 1.0, 1.0, NEG, 0, U.new_stats())
    out["numpy_epoch_s"] = (time.perf_counter() - t) / len(picks)
    out["numpy_layout_200_epochs_s"] = out["numpy_epoch_s"] * EPOCHS
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


def load(out_path):
    if os.path.exists(out_path):
        with open(out_path) as f:
            return json.load(f)
    return {}


def write(out, out_path):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


def main():
    default = os.path.join(ROOT, "profiles", "umap_1m.json")
    if len(sys.argv) > 1 and sys.argv[1] == "--tolerances":
        out_path = sys.argv[2] if len(sys.argv) > 2 else default
        out = load(out_path)
        out["tolerances"] = child(300, "tolerances")
        out["tolerances"]["note"] = ("largest differences between the device and tests/umap_restated.py over the inputs of "
                                     "tests/test_gpu_umap.py; relative for sigma and w, |dY| / 10 for three epochs of the layout")
        write(out, out_path)
        out["tolerances_edges"] = child(300, "tolerances-edges")
        out["tolerances_edges"]["note"] = ("the same over the inputs of tests/test_gpu_umap_edges.py; sigma over the rows with rho > 0, "
                                           "|dY| over every case's extent and epochs")
        write(out, out_path)
        return
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    out_path = sys.argv[3] if len(sys.argv) > 3 else default
    out = load(out_path)
    out["workload"] = (f"{n} cells x {G} genes of bench.synth_inputs(seed=42) -> pca(50, normalize=True) -> neighbors(method='umap', "
                       f"{NEIGHBORS}) -> umap({EPOCHS} epochs, negative_sample_rate {NEG}, start X_pca); one warm-up of every call on "
                       f"4096 rows, then the timed calls")
    scale = n / 1e6
    out["pipeline"] = child(int(240 + 600 * scale), "pipeline", n, G)
    write(out, out_path)
    cpu_n = min(CPU_CELLS, n)
    cpu = child(600, "cpu", cpu_n, G)
    cpu["scaled_to_cells"] = n
    cpu["numpy_fuzzy_graph_scaled_s"] = cpu["numpy_fuzzy_graph_s"] * n / cpu_n
    cpu["numpy_layout_scaled_s"] = cpu["numpy_layout_200_epochs_s"] * n / cpu_n
    cpu["note"] = "the numpy restatement, scaled linearly in the cells: a figure for this host, not umap-learn (not installed)"
    out["cpu"] = cpu
    write(out, out_path)
    say(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        a = sys.argv[3:]
        if sys.argv[2] == "tolerances":
            rec = step_tolerances()
        elif sys.argv[2] == "tolerances-edges":
            rec = step_tolerances_edges()
        elif sys.argv[2] == "pipeline":
            rec = step_pipeline(int(a[0]), int(a[1]))
        else:
            rec = step_cpu(int(a[0]), int(a[1]))
        say(json.dumps(rec))
    else:
        main()
