"""harmony_integrate on the device: the measured distance from the numpy restatement, and the 10^6-cell timing.

--tolerances   every input of tests/harmony_restated.py: CASES walked through the checkpoints of walk() (after begin, after 1
               and 5 clustering rounds, after the correction, after 3 outer rounds of 5) on the device and on the restatement
               from the same centres; per array the largest |device - restated| / max |restated| over all cases and
               checkpoints.  tests/test_gpu_harmony.py carries the figures as MEASURED_* and asserts ten times each.
--timing       10^6 cells of the bench's synthetic counts -> pca (50 components) with a synthetic 4-batch column: the public
               call's wall time, the time per clustering round and per correction (one wait per call, so launch gaps are
               inside), the rates of the two contractions against the data-sheet fp64 peak and of the whole round against the
               HBM peak, the launches per round, and the numpy restatement on this host at 50,000 cells scaled linearly.
Both write under their own key of profiles/harmony_1m.json (or --out PATH), keeping the other key.

Usage:  python scripts/harmony_probe.py [--tolerances] [--timing] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import harmony_restated as H  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402

FP64_PEAK, HBM_PEAK = 78.6e12, 8.0e12      # data-sheet figures of the MI355X, not measured here


def say(*a):
    print(*a, flush=True)


def tolerances(ctx):
    worst, where, per_case = {}, {}, {}
    for case in H.CASES:
        got, want = H.device_walk(ctx, case), H.restated_walk(case)
        diff = H.relative_differences(got, want)
        per_case[case[0]] = {a: max(v for (cp, b), v in diff.items() if b == a) for a in H.ARRAYS + ("objective",)}
        for (cp, a), v in diff.items():
            if not np.isfinite(v) or v >= worst.get(a, -1.0):
                worst[a], where[a] = v, f"{case[0]} at {cp}"
        say(case[0], {a: f"{v:.2e}" for a, v in per_case[case[0]].items()})
    return {"figure": "max |device - restated| / max |restated| per array over every case of tests/harmony_restated.py: CASES "
                      "and every checkpoint of walk()",
            "max_relative_difference": worst, "reached_in": where, "per_case": per_case}


def timing(ctx):
    import bench
    from spatialcore_amd.integration import harmony, harmony_integrate
    from spatialcore_amd.pca import pca

    n, G, d, B = 1_000_000, 500, 50, 4
    t0 = time.perf_counter()
    _, dense = bench.synth_inputs(n, G, seed=42)
    ad = SimpleAnnData(dense, var_names=[f"g{i}" for i in range(G)])
    pca(ad, n_comps=d, normalize=True, dtype="float64")
    Z = np.ascontiguousarray(ad.obsm["X_pca"])
    del dense
    rng = np.random.default_rng(3)
    batch = rng.integers(0, B, size=n).astype(np.int32)
    Z = Z + 0.5 * Z.std(axis=0)[None, :] * rng.normal(size=(B, d))[batch]      # every batch moved by its own vector
    say(f"input: {n} x {d} ({time.perf_counter() - t0:.1f} s)")
    ad.obsm["X_pca"], ad.obs["batch"] = Z, batch
    small = SimpleAnnData(np.zeros((4096, 1)), var_names=["g"])
    small.obsm["X_pca"], small.obs["batch"] = Z[:4096], batch[:4096]
    harmony_integrate(small, "batch", max_iter_harmony=1, max_iter_kmeans=2)      # code objects, allocations
    t = time.perf_counter()
    harmony_integrate(ad, "batch")
    wall = time.perf_counter() - t
    info = ad.uns["harmony"]
    K, nb = info["nclust"], info["n_blocks"]
    say(f"public call {wall:.2f} s: {info['n_rounds']} outer rounds of {[len(o) for o in info['objectives']]} clustering rounds")
    # the parts, on the same start
    t = time.perf_counter()
    Y = harmony.kmeans_start(ctx, harmony.unit_rows(Z), K, 10, 0)
    t_start = time.perf_counter() - t
    t = time.perf_counter()
    ctx.harmony_begin(Z, batch, B, Y, nb, 0.1, 2.0, 1.0)
    t_begin = time.perf_counter() - t
    ctx.harmony_cluster(1, -1.0)
    rounds = 10
    t = time.perf_counter()
    ctx.harmony_cluster(rounds, -1.0)
    t_round = (time.perf_counter() - t) / rounds
    t = time.perf_counter()
    ctx.harmony_correct()
    t_correct = time.perf_counter() - t
    t = time.perf_counter()
    ctx.harmony_get("Zcorr")
    t_get = time.perf_counter() - t
    mem = ctx.device_mem()
    ctx.harmony_end()
    flop_round = 2 * 2.0 * n * K * d                      # Zc Y^T and R^T Zc
    # bytes a round moves at the least: dist and S written, S read twice and R written in the blocks, R and dist read by the
    # objective, R and Zc read by R^T Zc, Zc read by the distances
    bytes_round = 8.0 * n * K * (2 + 2 + 1 + 2 + 1) + 8.0 * n * d * 2
    # the numpy restatement on this host at 50,000 cells, scaled linearly in the cells
    nb_small = 50_000
    t = time.perf_counter()
    h = H.Harmony(Z[:nb_small], batch[:nb_small], B, Y, nb, 0.1, 2.0, 1.0)
    h.cluster(2, -1.0)
    h.correct()
    t_np = time.perf_counter() - t
    inner = sum(len(o) for o in info["objectives"])
    np_call = t_np / 3.0 * (inner + info["n_rounds"]) * (n / nb_small)     # begin + 2 rounds + a correction: about three passes
    return {
        "workload": f"{n} cells of bench.synth_inputs(seed=42, {G} genes) -> pca({d}, normalize=True, float64), a synthetic {B}-batch "
                    f"column (uniform) with a per-batch shift of half a standard deviation per component; nclust = {K}, {nb} blocks, defaults",
        "public_call_s": wall, "outer_rounds": info["n_rounds"], "clustering_rounds": [len(o) for o in info["objectives"]],
        "converged": info["converged"],
        "parts_s": {"kmeans_start": t_start, "begin_with_host_sort_and_upload": t_begin, "clustering_round": t_round,
                    "correction": t_correct, "get_zcorr": t_get},
        "parts_note": "wall time around calls that wait for the device once, launch gaps included; no per-kernel events",
        "launches_per_round": 9 + 2 * nb,
        "round": {"flop_of_the_two_contractions": flop_round, "fraction_of_fp64_peak_whole_round": flop_round / t_round / FP64_PEAK,
                  "bytes_at_least": bytes_round, "fraction_of_hbm_peak_whole_round": bytes_round / t_round / HBM_PEAK,
                  "peaks": "78.6 TFLOP/s fp64 and 8 TB/s HBM: data-sheet figures, not measured here",
                  "note": "the contractions, the 2 x blocks launches of the block chain and the objective share the round's time; the "
                          "fractions are those of the whole round, a lower bound for each part"},
        "device_mem_bytes": mem,
        "numpy_restatement_same_host": {"cells": nb_small, "seconds_begin_2_rounds_1_correction": t_np,
                                        "seconds_extrapolated_to_the_public_call": np_call, "extrapolated": True,
                                        "cpus": os.cpu_count(), "threads_env": os.environ.get("OMP_NUM_THREADS")},
        "speedup_vs_extrapolated_numpy": np_call / wall,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tolerances", action="store_true")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmony_1m.json"))
    args = ap.parse_args()
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    ctx = _lib.default_context(0)
    if args.tolerances:
        out["tolerances"] = tolerances(ctx)
    if args.timing:
        out["timing"] = timing(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    say(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
