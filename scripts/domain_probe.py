"""make_spatial_domains at 10^6 cells: uniform cells at the bench density (10^4 x 10^4), targets in six blobs (60 % of
the cells inside a blob, 1 % outside: the recipe of the tests' input B, scaled up), Xenium defaults d = 50, m = 25,
assign_all_cells=True.  One warm-up, then five repetitions: device-synchronised wall time of the public call and of
the native call alone.  The share of queries that reach the full rim test (nearest target farther than m, not farther
than d) and K, the targets within d + s of such a query, are counted on the host with a k-d tree.
Writes profiles/domains_1m.json.

Usage:  python scripts/domain_probe.py
        rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/domain_probe.py --trace
        python scripts/domain_probe.py --kernel-stats DIR/.../*_kernel_stats.csv     (adds the kernels' times)"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.spatial import make_spatial_domains  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trace", action="store_true", help="one warm-up and one call, nothing written (for a kernel trace)")
ap.add_argument("--kernel-stats", help="kernel_stats.csv of a --kernel-trace --stats run of --trace")
opt = ap.parse_args()

n, d, m = 1_000_000, 50.0, 25.0
rng = np.random.default_rng(2)
L = np.sqrt(n) * 10
coords = rng.uniform(0, L, (n, 2))
cen = rng.uniform(0, L, (6, 2))
rad = rng.uniform(.08, .2, 6) * L
in_blob = np.zeros(n, dtype=bool)
for c, r in zip(cen, rad):
    in_blob |= ((coords - c) ** 2).sum(axis=1) < r * r
dense, sparse = rng.random(n) < 0.6, rng.random(n) < 0.01
target = np.where(in_blob, dense, sparse)
ctx = _lib.default_context(0)


def adata():
    obs = pd.DataFrame({"is_target": target}, index=pd.RangeIndex(n).astype(str))
    return SimpleAnnData(np.zeros((n, 1)), obs=obs, var_names=["g0"], obsm={"spatial": coords})


def public():
    a = adata()
    ctx.sync()
    t0 = time.perf_counter()
    make_spatial_domains(a, "is_target", domain_prefix="blob")     # cell_dist_um: Xenium's 50 by detection; margin 25
    ctx.sync()
    return time.perf_counter() - t0, a


def native():
    T, Q = coords[target], coords[~target]
    ctx.sync()
    t0 = time.perf_counter()
    ctx.domains(T, Q, d, d - m, return_clearance=False)
    ctx.sync()
    return time.perf_counter() - t0


_, first = public()
native()
if opt.trace:
    sys.exit(0)
walls, native_walls = [], []
for _ in range(5):
    w, a = public()
    walls.append(w)
    native_walls.append(native())
assert a.obs["spatial_domain"].fillna("").equals(first.obs["spatial_domain"].fillna(""))     # run to run identical

from scipy.spatial import cKDTree  # noqa: E402

tree = cKDTree(coords[target])
Q = coords[~target]
near = tree.query(Q, k=1)[0]
rim = (near > m) & (near <= d)
K = tree.query_ball_point(Q[rim], d + (d - m), return_length=True)
meta = a.uns["spatialcore_metadata"]["operations"][-1]["outputs"]
out = {
    "workload": f"{n} uniform cells on {L:g} x {L:g}, six blobs of targets (0.6 inside, 0.01 outside), "
                f"cell_dist_um={d}, shrink_margin_um={m}, assign_all_cells=True",
    "n_targets": int(target.sum()), "n_queries": int((~target).sum()),
    "n_domains": int(meta["n_domains"]), "n_cells_assigned": int(meta["n_cells_assigned"]),
    "public_call_s": walls, "public_call_median_s": float(np.median(walls)),
    "native_call_s": native_walls, "native_call_median_s": float(np.median(native_walls)),
    "queries_outside_u_share": float((near > d).mean()),
    "queries_first_exit_share": float((near <= m).mean()),
    "queries_rim_share": float(rim.mean()),
    "rim_K_mean": float(K.mean()), "rim_K_median": float(np.median(K)), "rim_K_p99": float(np.percentile(K, 99)),
    "rim_K_max": int(K.max()),
    "device_mem_bytes": ctx.device_mem(),
}
if opt.kernel_stats:
    with open(opt.kernel_stats) as f:
        for row in csv.DictReader(f):
            for k in ("k_dom_link", "k_dom_flatten", "k_dom_cover"):
                if row["Name"].startswith(k + "("):
                    out[k + "_avg_ms"] = float(row["AverageNs"]) / 1e6
                    out[k + "_calls"] = int(row["Calls"])
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "domains_1m.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
