"""The neighbour searches at 10^6 uniform cells (the coordinates of scripts/perf_probe.py), one build of the library
against another: outputs compared with np.array_equal, times side by side.

    python scripts/search_probe.py OTHER_LIB.so [--rounds 1] [--out profiles/search_ab.json]

Searches: kNN for k = 15 (k_knn<16>) and k = 64 (k_knn_heap), indices and squared distances; the radius graph at
r = 30; nearest target with and without exclusion codes for 10^5 queries; sc_ripley_build + the observed counts table.
One fresh child process per run (the library is chosen through SPATIALCORE_HIP_LIB), order other / this / this / other
per round.  A child calls every search once unrecorded and then `--repeats` times by a host clock around a call that
ends in ctx.sync(); the first child of each library also leaves its outputs for the comparison.  All runs are written
to the JSON file; the condition printed per figure is "this build's median inside the other build's min-max range, or
on its fast side".
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_QUERIES, T = 1_000_000, 100_000, 20
RADIUS = 30.0
RIPLEY_RADII = [5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 40.0, 50.0]


def child(save_dir, repeats):
    sys.path.insert(0, ROOT)
    from spatialcore_amd import _lib

    rng = np.random.default_rng(42)
    coords = rng.uniform(0, np.sqrt(N) * 10, (N, 2))
    queries = rng.uniform(-200.0, np.sqrt(N) * 10 + 200.0, (N_QUERIES, 2))     # (some lie outside the targets' grid)
    labels = rng.integers(0, T, N).astype(np.int32)
    q_excl = rng.integers(0, T, N_QUERIES).astype(np.int32)
    ctx = _lib.Context(0)
    out = {}

    def ripley():
        n_pairs = ctx.ripley_build(coords, RIPLEY_RADII)
        return np.array([n_pairs]), ctx.ripley_counts(labels, T, 0)

    searches = {   # name: (timed call, call that returns the outputs, or None if the timed call does)
        "knn_k15": (lambda: ctx.knn(coords, 15, fetch=False), lambda: ctx.knn(coords, 15, return_distance=True)),
        "knn_k64": (lambda: ctx.knn(coords, 64, fetch=False), lambda: ctx.knn(coords, 64, return_distance=True)),
        "radius_r30": (lambda: ctx.radius_graph(coords, RADIUS), None),
        "nearest": (lambda: ctx.nearest(coords, queries), None),
        "nearest_excluding": (lambda: ctx.nearest_excluding(coords, labels, queries, q_excl), None),
        "ripley_build_observed": (ripley, None),
    }
    for name, (timed, fetch) in searches.items():
        result = (fetch or timed)()          # unrecorded first call: code objects, allocations
        ctx.sync()
        if save_dir:
            for j, a in enumerate(result):
                np.save(os.path.join(save_dir, f"{name}_{j}.npy"), a)
        del result
        wall, kernel = [], []
        for _ in range(repeats):
            ctx.reset_timers()
            ctx.sync()
            t0 = time.perf_counter()
            timed()
            ctx.sync()
            wall.append(1e3 * (time.perf_counter() - t0))
            kernel.append(ctx.kernel_time(_lib.K_KNN)[0])    # (the kNN and nearest kernels carry the library's event timer)
        out[name] = {"wall_ms": wall}
        if name.startswith(("knn", "nearest")):
            out[name]["kernel_ms"] = kernel
    print("SEARCH_PROBE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("other", nargs="?", help="the other build of libspatialcore_hip.so")
    ap.add_argument("--other-name", default="another build", help="what the other build is, for the JSON file")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_ab.json"))
    ap.add_argument("--child", metavar="SAVE_DIR", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.repeats)
    if not a.other:
        ap.error("the other build's libspatialcore_hip.so is required")
    libs = {"other": os.path.abspath(a.other), "this": os.path.join(ROOT, "spatialcore_amd", "libspatialcore_hip.so")}
    tmp = tempfile.mkdtemp(prefix="search_probe_")
    runs = {"other": [], "this": []}
    try:
        for which in ["other", "this", "this", "other"] * a.rounds:
            save = os.path.join(tmp, which) if not runs[which] else ""
            if save:
                os.makedirs(save)
            env = dict(os.environ, SPATIALCORE_HIP_LIB=libs[which])
            text = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", save, "--repeats", str(a.repeats)],
                                  env=env, check=True, stdout=subprocess.PIPE, text=True).stdout
            runs[which].append(json.loads([ln for ln in text.splitlines() if ln.startswith("SEARCH_PROBE ")][-1][13:]))
            print(which, json.dumps(runs[which][-1]), flush=True)
        names = sorted(os.listdir(os.path.join(tmp, "other")))
        assert names and names == sorted(os.listdir(os.path.join(tmp, "this"))), names
        equal = {f[:-4]: bool(np.array_equal(np.load(os.path.join(tmp, "other", f), mmap_mode="r"),
                                            np.load(os.path.join(tmp, "this", f), mmap_mode="r"))) for f in names}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    figures = {}
    for name in runs["other"][0]:
        for key in runs["other"][0][name]:
            o = [v for r in runs["other"] for v in r[name][key]]
            t = [v for r in runs["this"] for v in r[name][key]]
            figures[f"{name}.{key}"] = {"other": o, "this": t, "other_min_max": [min(o), max(o)],
                                        "other_median": float(np.median(o)), "this_median": float(np.median(t)),
                                        "this_median_not_above_other_max": bool(np.median(t) <= max(o))}
    out = {"other": a.other_name, "this": "this tree's build",
           "workload": f"{N} uniform cells on a square of side {np.sqrt(N) * 10:g}; kNN k = 15 and 64, radius graph r = {RADIUS:g}, "
                       f"nearest target for {N_QUERIES} queries with and without exclusion codes ({T} codes), sc_ripley_build "
                       f"(radii {RIPLEY_RADII}) + observed counts; host clock around a call that ends in ctx.sync(), first call of "
                       f"every child discarded, {a.repeats} repeats per child, children in the order other / this / this / other",
           "outputs_array_equal": equal, "all_outputs_array_equal": all(equal.values()), "figures_ms": figures}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"outputs_array_equal": equal,
                      "figures": {k: [v["other_min_max"], v["other_median"], v["this_median"], v["this_median_not_above_other_max"]]
                                  for k, v in figures.items()}}, indent=1))
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
