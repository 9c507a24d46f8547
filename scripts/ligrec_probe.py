"""ligrec at 10^6 cells, 20 clusters with Dirichlet weights, 300 genes, 200 interactions, 1000 Philox permutations: once on
raw counts and once on log-normalised float32 (the same counts through per-cell size factors and log1p).
One small warm-up call, then each timed call once.  Records the wall time of the public call, the grouped-sum kernel's time
and launches (context timer SC_K_LIGREC, observed pass included), integer adds per second (one 64-bit LDS add per non-zero
value and permutation) and bytes streamed per second (per pass of NP permutations: the fp64 tiles, 128 B per cell and
16-gene tile, and the label words, NP B per cell and tile), and the plain restatement (tests/ligrec_restated.py) timed in
this process at a size it can finish, scaled linearly in cells x permutations: an EXTRAPOLATED speed-up.
Writes profiles/ligrec_1m.json.

    python scripts/ligrec_probe.py [n_cells] [n_perms]

Counters: run the same workload (fewer permutations are enough) under rocprofv3 --pmc, counters only, no tracing
alongside, one pass per counter set, then summarise into profiles/ligrec_1m_pmc.json:

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES -d build/ligrec_pmc_lds --output-format csv -- \
        python scripts/ligrec_probe.py 1000000 64 --no-restatement
    rocprofv3 --pmc FETCH_SIZE GRBM_GUI_ACTIVE -d build/ligrec_pmc_fetch --output-format csv -- python scripts/ligrec_probe.py 1000000 64 --no-restatement
    python scripts/ligrec_probe.py --pmc-summary build/ligrec_pmc_lds build/ligrec_pmc_fetch
"""
import csv
import glob
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pmc_summary(dirs):
    """Per kernel form of k_ligrec_sums: dispatches and the sum of every counter found under the given rocprofv3 output
    directories."""
    acc = defaultdict(lambda: defaultdict(lambda: [0, 0.0]))
    for d in dirs:
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if "k_ligrec_sums" not in row["Kernel_Name"]:
                        continue
                    form = "observed (NP=1)" if "1, true" in row["Kernel_Name"] else "null"
                    a = acc[form][row["Counter_Name"]]
                    a[0] += 1
                    a[1] += float(row["Counter_Value"])
    out = {"method": "rocprofv3 --pmc, counters only, one pass per counter set (see scripts/ligrec_probe.py); sums over all "
                     "dispatches of the run.  SQ_LDS_BANK_CONFLICT = extra LDS cycles, SQ_LDS_IDX_ACTIVE = all LDS-array cycles, "
                     "SQ_WAVE_CYCLES in quad-cycles, GRBM_GUI_ACTIVE summed over the 8 XCDs, FETCH_SIZE in KiB (gfx950 tallies a "
                     "128-byte request of a coalesced read at 64 bytes: fetch_bytes_doubled is the figure to compare with "
                     "the bytes the kernel streams)",
           "kernels": {form: {name: {"dispatches": v[0], "sum": v[1]} for name, v in counters.items()} for form, counters in acc.items()}}
    for form, counters in out["kernels"].items():
        if "SQ_LDS_BANK_CONFLICT" in counters and counters.get("SQ_LDS_IDX_ACTIVE", {}).get("sum"):
            counters["lds_conflict_share_of_lds_cycles"] = counters["SQ_LDS_BANK_CONFLICT"]["sum"] / counters["SQ_LDS_IDX_ACTIVE"]["sum"]
        if "FETCH_SIZE" in counters:
            counters["fetch_bytes_doubled"] = 2 * 1024 * counters["FETCH_SIZE"]["sum"]
        if "GRBM_GUI_ACTIVE" in counters and "SQ_LDS_IDX_ACTIVE" in counters:
            # LDS-array cycles per compute unit (256) over the kernel's active cycles per XCD (8)
            counters["lds_busy_share_of_kernel_cycles"] = (counters["SQ_LDS_IDX_ACTIVE"]["sum"] / 256) / (counters["GRBM_GUI_ACTIVE"]["sum"] / 8)
    with open(os.path.join(ROOT, "profiles", "ligrec_1m_pmc.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if "--pmc-summary" in sys.argv:
    pmc_summary(sys.argv[sys.argv.index("--pmc-summary") + 1:])
    sys.exit(0)

from scipy import sparse  # noqa: E402

from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.spatial import ligrec  # noqa: E402

numbers = [a for a in sys.argv[1:] if a.isdigit()]
n = int(numbers[0]) if numbers else 1_000_000
P = int(numbers[1]) if len(numbers) > 1 else 1000
K, G, I = 20, 300, 200
rng = np.random.default_rng(42)
lam = np.exp(rng.uniform(np.log(0.05), np.log(5.0), G))
counts = sparse.csr_matrix(rng.poisson(lam[None, :], (n, G)).astype(np.float32))
depth = np.asarray(counts.sum(axis=1)).ravel() + rng.uniform(0.5, 1.5, n)
lognorm = sparse.diags((np.median(depth) / depth).astype(np.float32)) @ counts
lognorm.data = np.log1p(lognorm.data).astype(np.float32)
lognorm = sparse.csr_matrix(lognorm, dtype=np.float32)
codes = rng.choice(K, n, p=rng.dirichlet(np.ones(K)))
names = [f"g{i}" for i in range(G)]
pairs = list(dict.fromkeys((names[a], names[b]) for a, b in rng.integers(0, G, (2 * I, 2))))[:I]
ctx = _lib.default_context(0)


def adata(X, sel=slice(None)):
    obs = pd.DataFrame({"cluster": pd.Categorical([f"c{v:02d}" for v in codes[sel]], categories=[f"c{v:02d}" for v in range(K)])},
                       index=pd.RangeIndex(X[sel].shape[0]).astype(str))
    return SimpleAnnData(X[sel], obs=obs, var_names=names)


ligrec(adata(counts, slice(0, 20000)), "cluster", pairs, n_perms=32, rng="philox")     # warm-up: code objects, first allocations


def timed(X):
    a = adata(X)
    ctx.sync()
    ctx.reset_timers()
    t0 = time.perf_counter()
    ligrec(a, "cluster", pairs, n_perms=P, rng="philox", seed=1)
    ctx.sync()
    wall = time.perf_counter() - t0
    ms, launches = ctx.kernel_time(_lib.K_LIGREC)
    used = sorted({names.index(g) for p in pairs for g in p})
    nnz = int(X[:, used].nnz)
    tiles = -(-len(used) // 16)
    np_pass = 16 if K <= 32 else 8 if K <= 64 else 4
    passes = -(-P // np_pass)
    adds = nnz * (P + 1)
    streamed = tiles * n * (128 + np_pass) * passes + tiles * n * 129
    res = a.uns["cluster_ligrec"]
    return {"wall_s": wall, "k_ligrec_sums_s": ms / 1e3, "k_ligrec_sums_launches": launches, "genes_loaded": len(used),
            "non_zero_values": nnz, "integer_adds": adds, "integer_adds_per_s": adds / (ms / 1e3),
            "bytes_streamed": streamed, "bytes_streamed_per_s": streamed / (ms / 1e3),
            "share_of_pvalues_nan": float(np.isnan(res["pvalues"].to_numpy()).mean()),
            "count_ge_checksum": int(res["count_ge"].to_numpy().sum())}


out = {"workload": f"{n} cells, {K} clusters with Dirichlet(1) weights, {G} Poisson genes (rates 0.05 .. 5), {len(pairs)} "
                   f"interactions, {P} Philox permutations, perm_batch 512",
       "raw_counts": timed(counts), "log_normalised_float32": timed(lognorm), "device_mem_bytes": ctx.device_mem()}

if "--no-restatement" not in sys.argv:
    import ligrec_restated as lr

    n_s, P_s = min(n, 20000), 8
    Xs = counts[:n_s].toarray().astype(np.float64)
    perms = _lib.perm_counter_host(1, n_s, P_s)
    idx = [(names.index(a), names.index(b)) for a, b in pairs]
    t0 = time.perf_counter()
    lr.restated(Xs, codes[:n_s], K, idx, perms)
    small = time.perf_counter() - t0
    scaled = small * (n / n_s) * (P / P_s)
    out["restatement"] = {"cells": n_s, "permutations": P_s, "wall_s": small,
                          "extrapolated_wall_s_at_full_size": scaled,
                          "extrapolated_speed_up_of_the_public_call_on_raw_counts": scaled / out["raw_counts"]["wall_s"],
                          "note": "EXTRAPOLATED: the numpy / Python-int restatement timed on this host at the small size and "
                                  "scaled linearly in cells x permutations"}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = "ligrec_1m.json" if (n, P) == (1_000_000, 1000) else f"ligrec_{n}_{P}.json"
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
