"""co_occurrence at 10^6 uniform cells (the bench's density: a square of side 10 sqrt(n)), 20 cell types with Dirichlet
weights, interval=50 -- against the existing all-pairs kernel, sc_pair_table_2d, on the same type-sorted points and
offsets in the same process: the same loads and the same distance arithmetic (plus a square root, a sum and a minimum),
without the bin search and the histogram.
One small warm-up call of each, then each timed call once (a call is about 10^12 ordered pairs).
Writes profiles/cooccurrence_1m.json.

Usage:  python scripts/cooccurrence_probe.py [n_cells]"""
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.spatial import co_occurrence  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
T, m = 20, 50
rng = np.random.default_rng(42)
L = np.sqrt(n) * 10.0
coords = rng.uniform(0, L, (n, 2))
weights = rng.dirichlet(np.ones(T))
codes = rng.choice(T, n, p=weights)
names = np.array([f"type{v:02d}" for v in range(T)])
ctx = _lib.default_context(0)


def adata(sel=slice(None)):
    obs = pd.DataFrame({"cell_type": pd.Categorical(names[codes[sel]], categories=list(names))},
                       index=pd.RangeIndex(coords[sel].shape[0]).astype(str))
    return SimpleAnnData(np.zeros((coords[sel].shape[0], 1)), obs=obs, var_names=["g0"], obsm={"spatial": coords[sel]})


def sorted_points(sel=slice(None)):
    c = codes[sel]
    order = np.argsort(c, kind="stable")
    return coords[sel][order], np.concatenate([[0], np.cumsum(np.bincount(c, minlength=T))]).astype(np.int64)


# warm-up at 20,000 cells: code objects, first allocations
co_occurrence(adata(slice(0, 20000)), "cell_type", interval=m)
xs, off = sorted_points(slice(0, 20000))
ctx.pair_table(xs, off, xs, off)

# (a) the public call: wall time, and the kernel's share from the context's timers
a = adata()
ctx.sync()
ctx.reset_timers()
t0 = time.perf_counter()
co_occurrence(a, "cell_type", interval=m)
ctx.sync()
wall_s = time.perf_counter() - t0
kernel_ms, launches = ctx.kernel_time(_lib.K_COOCCUR)
res = a.uns["cell_type_co_occurrence"]
count = res["count"]
assert launches == 1 and (count == count.transpose(1, 0, 2)).all()
# bin 0 is the radius graph at t_0
indptr, _ = ctx.radius_graph(coords, float(res["interval"][0]))
assert int(count[:, :, 0].sum()) == int(indptr[-1])

# (b) the same kernel with thresholds that reach past the tissue's diagonal: every ordered pair is counted exactly once
xs, off = sorted_points()
ctx.reset_timers()
full = ctx.cooccurrence_counts(xs, off, np.linspace(0.0, 1.5 * L, m))
kernel_all_ms, _ = ctx.kernel_time(_lib.K_COOCCUR)
assert int(full.sum()) == n * (n - 1), (int(full.sum()), n * (n - 1))

# (c) the yardstick: every ordered pair of the same points through k_pair_table (it has no timer of its own: wall time
# of the entry point, which uploads the points twice and checks them on the host first)
ctx.sync()
t0 = time.perf_counter()
tot, mn = ctx.pair_table(xs, off, xs, off)
ctx.sync()
pair_table_s = time.perf_counter() - t0
assert np.isfinite(tot).all() and (np.diag(mn) == 0).all()

unordered = n * (n - 1) // 2
out = {
    "workload": f"{n} uniform cells on a square of side {L:g}, {T} cell types with Dirichlet(1) weights "
                f"(smallest {int(res['n_per_type'].min())}, largest {int(res['n_per_type'].max())} cells), interval={m}",
    "thresholds_first_last": [float(res["interval"][0]), float(res["interval"][-1])],
    "co_occurrence_wall_s": wall_s,
    "k_cooccur_kernel_s": kernel_ms / 1e3,
    "unordered_pairs_evaluated": unordered,
    "ordered_pairs_counted": int(count.sum()),
    "share_of_ordered_pairs_dropped": 1.0 - int(count.sum()) / (n * (n - 1)),
    "k_cooccur_unordered_pairs_per_s": unordered / (kernel_ms / 1e3),
    "k_cooccur_all_pairs_in_range_kernel_s": kernel_all_ms / 1e3,
    "k_cooccur_all_pairs_in_range_unordered_pairs_per_s": unordered / (kernel_all_ms / 1e3),
    "pair_table_wall_s": pair_table_s,
    "pair_table_ordered_pairs_evaluated": n * n,
    "pair_table_pairs_per_s": n * n / pair_table_s,
    "ratio_cooccur_over_pair_table_pairs_per_s": (unordered / (kernel_ms / 1e3)) / (n * n / pair_table_s),
    "time_ratio_cooccur_kernel_over_pair_table": (kernel_ms / 1e3) / pair_table_s,
    "device_mem_bytes": ctx.device_mem(),
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
name = "cooccurrence_1m.json" if n == 1_000_000 else f"cooccurrence_{n}.json"
with open(os.path.join(ROOT, "profiles", name), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
