"""ripley_k at 10^6 cells x 20 cell types x 8 radii with 512 counter-based permutations, against the only route to
the same table without it: eight neighborhood_enrichment(method="radius") calls, and against the single such call at
the largest radius (the same pairs walked once with a T x T histogram: the floor a one-pass design can approach).
One warm-up of each, then three repetitions alternating a / b / c, device-synchronised wall time.
Writes profiles/ripley_1m.json.

Usage:  python scripts/ripley_probe.py"""
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.spatial import neighborhood_enrichment, ripley_k  # noqa: E402

n, T, P = 1_000_000, 20, 512
radii = [5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 40.0, 50.0]
rng = np.random.default_rng(42)
coords = rng.uniform(0, 1.0e4, (n, 2))
labels = np.array([f"type{v:02d}" for v in range(T)])[rng.integers(0, T, n)]
ctx = _lib.default_context(0)


def adata():
    obs = pd.DataFrame({"cell_type": labels}, index=pd.RangeIndex(n).astype(str))
    return SimpleAnnData(np.zeros((n, 1)), obs=obs, var_names=["g0"], obsm={"spatial": coords})


def timed(fn):
    a = adata()
    ctx.sync()
    t0 = time.perf_counter()
    fn(a)
    ctx.sync()
    return time.perf_counter() - t0, a


def route_a(a):
    ripley_k(a, "cell_type", radii, n_permutations=P, seed=0, rng="philox")


def route_b(a):
    for r in radii:
        neighborhood_enrichment(a, "cell_type", method="radius", radius=r, n_permutations=P, seed=0, rng="philox",
                                key_added=f"enrichment_r{r:g}")


def route_c(a):
    neighborhood_enrichment(a, "cell_type", method="radius", radius=radii[-1], n_permutations=P, seed=0, rng="philox")


routes = {"a": route_a, "b": route_b, "c": route_c}
results = {}
for name, fn in routes.items():            # warm-up: code objects, allocations
    _, results[name] = timed(fn)
# the three routes compute the same integers
count = results["a"].uns["ripley_k"]["count"]
for j, r in enumerate(radii):
    assert (count[:, :, j] == results["b"].uns[f"enrichment_r{r:g}"]["count"]).all(), r
assert (count[:, :, -1] == results["c"].uns["neighborhood_enrichment"]["count"]).all()
walls = {name: [] for name in routes}
for _ in range(3):
    for name, fn in routes.items():
        walls[name].append(timed(fn)[0])
n_pairs = int(count[:, :, -1].sum())
meta = results["a"].uns["spatialcore_metadata"]["operations"][-1]["outputs"]
assert meta["n_pairs"] == n_pairs
out = {
    "workload": f"{n} uniform cells on 1e4 x 1e4, {T} independent cell types, radii {radii}, {P} permutations, rng=philox",
    "a_ripley_k_s": walls["a"], "b_eight_radius_enrichments_s": walls["b"], "c_one_enrichment_at_r_max_s": walls["c"],
    "a_median_s": float(np.median(walls["a"])), "b_min_s": float(np.min(walls["b"])), "c_median_s": float(np.median(walls["c"])),
    "ratio_a_over_b": float(np.median(walls["a"]) / np.median(walls["b"])),
    "ratio_a_over_c": float(np.median(walls["a"]) / np.median(walls["c"])),
    "a_median_below_b_min": bool(np.median(walls["a"]) < np.min(walls["b"])),
    "ordered_pairs_within_r_max": n_pairs,
    "stored_pairs": n_pairs // 2,
    "bytes_per_stored_pair": 9,
    "bytes_per_stored_pair_note": "two int32 positions + one radius-bin byte; each unordered pair is stored once",
    "device_mem_bytes": ctx.device_mem(),
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ripley_1m.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
