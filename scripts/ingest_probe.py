"""ingest at 10^6 cells of the bench's synthetic counts: pca (50 components, normalize=True), the scores truncated to
d = 20 and 50, k = 15, at two shapes:
  same     n_ref = n_query = 10^6: the reference's own cells are the queries (every cell finds itself first)
  atlas    n_ref = 2 x 10^5 (the first rows), n_query = 10^6 (all rows: 8 x 10^5 of them are not in the reference)
Per (shape, d), in ONE process: sc_knn_cross alone three times (path 0, with its info), the two gather kernels
(sc_cross_vote on 20 classes, uniform and distance; sc_cross_regress on 2 columns), the public ``ingest`` call (one label
column, one 2-column embedding), and sc_knn_dense_gram on the same 10^6 rows, three times; their ratio.  Then sklearn's
brute-force KNeighborsClassifier on the same host: 50,000 of the queries against the whole reference, SCALED to 10^6
queries (x 20) and recorded as scaled.

Every step is a child process under its own time limit; a step that fails or runs out of time ends the probe.  Writes
profiles/ingest_1m.json (or the path given last).

Usage:  python scripts/ingest_probe.py [n_cells [n_genes [out.json]]]"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIMS = (20, 50)
NEIGHBORS = 15
CLASSES = 20
SKLEARN_QUERIES = 50_000


def say(*a):
    print(*a, flush=True)


def timed(ctx, fn, *a, **kw):
    ctx.sync()
    t = time.perf_counter()
    r = fn(*a, **kw)
    ctx.sync()
    return time.perf_counter() - t, r


def step_scores(n, G, path):
    import bench
    from scipy import sparse

    from spatialcore_amd import SimpleAnnData, _lib
    from spatialcore_amd.pca import pca

    ctx = _lib.default_context(0)
    _, dense = bench.synth_inputs(n, G, seed=42)
    ad = SimpleAnnData(sparse.csr_matrix(dense), var_names=[f"g{i}" for i in range(G)])
    t, _ = timed(ctx, pca, ad, max(DIMS), normalize=True)
    np.save(path, np.ascontiguousarray(ad.obsm["X_pca"], dtype=np.float64))
    return {"pca_s": t}


def _shape(scores, shape, d):
    X = np.ascontiguousarray(np.load(scores)[:, :d])
    n_ref = X.shape[0] if shape == "same" else X.shape[0] // 5
    return X, X[:n_ref]


def _side_data(n_ref):
    rng = np.random.default_rng(0)
    return rng.integers(0, CLASSES, size=n_ref).astype(np.int32), rng.standard_normal((n_ref, 2))


def step_device(scores, shape, d):
    from spatialcore_amd import SimpleAnnData, _lib
    from spatialcore_amd.neighbors import ingest

    ctx = _lib.default_context(0)
    Q, R = _shape(scores, shape, d)
    codes, Y = _side_data(R.shape[0])
    ctx.knn_cross(R[:4096], Q[:4096], NEIGHBORS)                 # code objects, allocations
    ctx.knn_dense_gram(Q[:4096], NEIGHBORS)
    out = {"shape": shape, "d": d, "n_ref": int(R.shape[0]), "n_query": int(Q.shape[0]), "cross": [], "self": []}
    for _ in range(3):
        t, (_, _, info) = timed(ctx, ctx.knn_cross, R, Q, NEIGHBORS, True)
        out["cross"].append({"call_s": t, "info": info})
        say(f"{shape} d={d} cross: {t:.2f} s {info}")
    gathers = {}
    for name, fn in (("vote_uniform", lambda: ctx.cross_vote(codes, CLASSES, "uniform")),
                     ("vote_distance", lambda: ctx.cross_vote(codes, CLASSES, "distance")),
                     ("regress_uniform", lambda: ctx.cross_regress(Y, "uniform")),
                     ("regress_distance", lambda: ctx.cross_regress(Y, "distance"))):
        fn()
        ctx.reset_timers()
        t, _ = timed(ctx, fn)
        gathers[name] = {"call_s": t, "kernels_ms": ctx.kernel_time(_lib.K_INGEST)[0]}
    out["gathers"] = gathers
    say(f"{shape} d={d} gathers: {gathers}")
    ref = SimpleAnnData(np.zeros((R.shape[0], 1), dtype=np.float32))
    ref.obsm["X_pca"], ref.obsm["X_umap"] = R, Y
    ref.obs["label"] = codes
    ad = SimpleAnnData(np.zeros((Q.shape[0], 1), dtype=np.float32))
    ad.obsm["X_pca"] = Q
    t, _ = timed(ctx, ingest, ad, ref, obs="label", obsm="X_umap", n_neighbors=NEIGHBORS)
    out["ingest_call_s"] = t
    say(f"{shape} d={d} ingest: {t:.2f} s")
    for _ in range(3):
        t, (_, _, info) = timed(ctx, ctx.knn_dense_gram, Q, NEIGHBORS, True)
        out["self"].append({"call_s": t, "info": info})
        say(f"{shape} d={d} self search of the {Q.shape[0]} rows: {t:.2f} s {info}")
    out["cross_over_self"] = min(r["call_s"] for r in out["cross"]) / min(r["call_s"] for r in out["self"])
    return out


def step_sklearn(scores, shape, d):
    from sklearn.neighbors import KNeighborsClassifier

    Q, R = _shape(scores, shape, d)
    codes, _ = _side_data(R.shape[0])
    m = min(SKLEARN_QUERIES, Q.shape[0])
    rows = np.random.default_rng(1).choice(Q.shape[0], size=m, replace=False)
    t = time.perf_counter()
    clf = KNeighborsClassifier(n_neighbors=NEIGHBORS, algorithm="brute").fit(R, codes)
    clf.predict(Q[rows])
    t = time.perf_counter() - t
    return {"shape": shape, "d": d, "queries_run": int(m), "fit_predict_s": t, "scaled_to_all_queries_s": t * Q.shape[0] / m,
            "scaled": True, "threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None}


def child(limit, *args):
    """One step in a fresh process under its own time limit; its last output line is the step's JSON record."""
    say(f"--- step {' '.join(map(str, args))} (limit {limit} s)")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", *map(str, args)], stdout=subprocess.PIPE, timeout=limit,
                       check=True, text=True)
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ingest_1m.json")
    scale = (n / 1e6) ** 2
    out = {"workload": f"{n} cells x {G} genes of bench.synth_inputs(seed=42) -> pca({max(DIMS)}, normalize=True), scores truncated "
                       f"to d, k = {NEIGHBORS}; shape 'same': the reference's own cells as queries; 'atlas': the first fifth of the "
                       f"rows as the reference, all rows as queries; every step a fresh process with one warm-up call on 4096 rows",
           "device": [], "sklearn": []}
    with tempfile.TemporaryDirectory() as tmp:
        scores = os.path.join(tmp, "scores.npy")
        out["pca_s"] = child(600, "scores", n, G, scores)["pca_s"]
        for shape in ("same", "atlas"):
            for d in DIMS:
                out["device"].append(child(int(120 + 60 * scale), "device", scores, shape, d))
        for shape in ("same", "atlas"):
            for d in DIMS:
                out["sklearn"].append(child(int(120 + 300 * scale), "sklearn", scores, shape, d))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    say(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        a = sys.argv[3:]
        if sys.argv[2] == "scores":
            rec = step_scores(int(a[0]), int(a[1]), a[2])
        elif sys.argv[2] == "device":
            rec = step_device(a[0], a[1], int(a[2]))
        else:
            rec = step_sklearn(a[0], a[1], int(a[2]))
        say(json.dumps(rec))
    else:
        main()
