"""rank_genes_groups at 10^6 cells x 500 genes of the bench's synthetic recipe (bench.synth_inputs): raw counts and
log-normalised values (per-cell size factors + log1p, float32), CSR, with 20 and with 300 groups.  Per case one warm-up,
then three repetitions: device-synchronised wall time of the public call, and the HIP-event time of the three native
stages (emit = count + scan + scatter, sort, runs) of the last repetition.  The comparison figure is the scipy
restatement (scipy.stats.rankdata per gene + per-group sums of the ranks) in this process on 8 of the genes,
extrapolated linearly to 500: an estimate, stated as such, not a gate.  Also the native call alone on resident tiles, which separates its host work (validation,
counting sort of the cells by group, uploads, result copies) from the three device stages.
Writes profiles/markers_1m.json.

Usage:  python scripts/markers_probe.py [--cells N] [--genes G]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
from scipy import sparse
from scipy.stats import rankdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.spatial import rank_genes_groups  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=1_000_000)
ap.add_argument("--genes", type=int, default=500)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "markers_1m.json"))
opt = ap.parse_args()
n, G = opt.cells, opt.genes
SUBSET = 8

_, counts = bench.synth_inputs(n, G, 0)
rng = np.random.default_rng(1)
depth = counts.sum(axis=1, keepdims=True, dtype=np.float64) + rng.uniform(0.5, 1.5, (n, 1))
lognorm = np.log1p(counts / depth * np.median(depth)).astype(np.float32)
inputs = {"raw_counts": sparse.csr_matrix(counts), "log_normalised": sparse.csr_matrix(lognorm)}
del counts, lognorm
ctx = _lib.default_context(0)
genes = [f"g{i}" for i in range(G)]


def adata(X, labels):
    obs = pd.DataFrame({"domain": labels}, index=pd.RangeIndex(n).astype(str))
    return SimpleAnnData(X, obs=obs, var_names=genes)


def public(X, labels):
    a = adata(X, labels)
    ctx.sync()
    ctx.reset_timers()
    t0 = time.perf_counter()
    rank_genes_groups(a, "domain", tie_correct=True)
    ctx.sync()
    wall = time.perf_counter() - t0
    stages = {name: ctx.kernel_time(k) for name, k in (("emit", _lib.K_RANK_EMIT), ("sort", _lib.K_RANK_SORT),
                                                        ("runs", _lib.K_RANK_RUNS))}
    return wall, stages, a


def scipy_restatement(X, code, n_groups):
    """rankdata + per-group rank sums of SUBSET genes, single process: seconds, to be scaled by G / SUBSET."""
    cols = np.asarray(X[:, :SUBSET].todense(), dtype=np.float64)
    t0 = time.perf_counter()
    for g in range(cols.shape[1]):
        r = rankdata(cols[:, g])
        np.bincount(code, weights=r, minlength=n_groups)
    return time.perf_counter() - t0


out = {"workload": f"{n} cells x {G} genes of bench.synth_inputs(seed 0), CSR, tie_correct=True, all groups against the rest",
       "cases": []}
for kind, X in inputs.items():
    for n_groups in (20, 300):
        code = np.random.default_rng(n_groups).integers(0, n_groups, n)
        labels = np.char.add("d", np.char.zfill(code.astype(str), 3)).astype(object)
        public(X, labels)                                    # warm-up: code objects, buffers, the sort's algorithm choice
        walls, keep = [], None
        for _ in range(opt.reps):
            wall, stages, a = public(X, labels)
            walls.append(wall)
            if keep is not None:                             # run to run identical
                assert keep["scores"].tobytes() == a.uns["rank_genes_groups"]["scores"].tobytes()
            keep = a.uns["rank_genes_groups"]
        # the native call alone on the resident tiles (codes 0 .. n_groups - 1): host counting sort + uploads + device + copies
        ctx.set_expression(X, np.arange(G, dtype=np.int32))
        ctx.ranksum(code, n_groups)
        native = []
        for _ in range(opt.reps):
            ctx.sync()
            ctx.reset_timers()
            t0 = time.perf_counter()
            ctx.ranksum(code, n_groups)
            ctx.sync()
            native.append(time.perf_counter() - t0)
        native_dev_ms = sum(ctx.kernel_time(k)[0] for k in (_lib.K_RANK_EMIT, _lib.K_RANK_SORT, _lib.K_RANK_RUNS))
        cpu_subset = scipy_restatement(X, code, n_groups)
        cpu_full = cpu_subset * G / SUBSET
        dev = {k: v[0] for k, v in stages.items()}
        case = {
            "values": kind, "n_groups": n_groups, "nnz": int(X.nnz),
            "public_call_s": walls, "public_call_median_s": float(np.median(walls)),
            "native_call_s": native, "native_call_median_s": float(np.median(native)),
            "native_call_host_and_copies_s": float(native[-1] - native_dev_ms / 1e3),
            "stage_ms": dev, "stage_launches": {k: v[1] for k, v in stages.items()},
            "largest_stage": max(dev, key=dev.get),
            "nonzeros_sorted_per_s": float(X.nnz / (dev["sort"] / 1e3)) if dev["sort"] > 0 else None,
            "scipy_rankdata_subset_genes": SUBSET, "scipy_rankdata_subset_s": cpu_subset,
            "scipy_rankdata_extrapolated_s": cpu_full,
            "ratio_scipy_extrapolated_over_public_call": cpu_full / float(np.median(walls)),
        }
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
out["device_mem_bytes"] = ctx.device_mem()
os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
