"""identify_niches at 10^6 cells x 20 cell types, K = 8, the reference's defaults (n_init=10, max_iter=300):
wall time (one warm-up call, then the median of 5), the context's kernel timers, iterations, and the bytes one Lloyd
pass reads against the HBM peak.  Writes profiles/niches_1m.json.

Usage:  python scripts/niche_probe.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.spatial import identify_niches  # noqa: E402

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes / s

n, C, K = 1_000_000, 20, 8
rng = np.random.default_rng(0)
mix = rng.dirichlet(np.full(C, 0.5), size=12)
P = (rng.dirichlet(np.ones(C), size=n) * 0.3 + mix[rng.integers(0, 12, n)] * 0.7).astype(np.float32)
ctx = _lib.default_context(0)


def once():
    a = SimpleAnnData(np.zeros((n, 1)), var_names=["g0"], obsm={"neighborhood_profile": P})
    ctx.sync()
    t0 = time.perf_counter()
    identify_niches(a, n_niches=K)
    return time.perf_counter() - t0, a


once()                                   # warm-up: code objects, allocations
ctx.reset_timers()
walls = []
for _ in range(5):
    w, a = once()
    walls.append(w)
seed_ms, seed_n = ctx.kernel_time(_lib.K_KMEANS_SEED)
lloyd_ms, lloyd_n = ctx.kernel_time(_lib.K_KMEANS_LLOYD)
meta = a.uns["spatialcore_metadata"]["operations"][-1]["outputs"]
iters_best = meta["n_iter"]
pass_bytes = n * C * 4
lloyd_per_launch_ms = lloyd_ms / max(lloyd_n, 1)
out = {
    "workload": "identify_niches, 1e6 cells x 20 cell types (float32), K=8, n_init=10, max_iter=300, random_state=0",
    "wall_s_median": float(np.median(walls)), "wall_s_all": walls,
    "kernel_ms_per_call": {"seeding (centring + k-means++ rounds)": seed_ms / 5, "lloyd (E-step + reduction)": lloyd_ms / 5},
    "launch_scopes_per_call": {"seeding": seed_n / 5, "lloyd": lloyd_n / 5},
    "n_iter_best_run": iters_best, "strict_convergence_best_run": meta["strict_convergence"],
    "lloyd_pass_ms_mean": lloyd_per_launch_ms,
    "lloyd_pass_bytes_X": pass_bytes, "lloyd_pass_hbm_floor_ms": pass_bytes / HBM_PEAK * 1e3,
    "cpu_reference_s": 12.4,
    "cpu_reference_note": "reference identify_niches (sklearn 1.7.2), same shape, measured on another machine, 8 threads",
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "niches_1m.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
