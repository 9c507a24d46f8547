"""ripley_g at 10^6 cells x 20 cell types x 8 radii with 512 counter-based permutations, with ripley_k on the same input
alternating in the same process as the yardstick -- on ripley_probe.py's uniform input, and on an input of the same size
with clustered coordinates (Gaussian clumps over a thin uniform background: rows of hundreds of entries next to rows of
almost none), which is where one thread per cell would show if long rows wanted a wavefront.
One warm-up of each, then three repetitions alternating g / k, device-synchronised wall time of the public calls; per
kernel family the HIP-event times of one ripley_g call (list build, relabel, counting: sc_ctx_kernel_time).
Writes profiles/ripley_g_1m.json.

Usage:  python scripts/ripley_g_probe.py"""
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.spatial import ripley_g, ripley_k  # noqa: E402

n, T, P, REPS = 1_000_000, 20, 512, 3
radii = [5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 40.0, 50.0]
ctx = _lib.default_context(0)


def uniform_input():
    rng = np.random.default_rng(42)
    coords = rng.uniform(0, 1.0e4, (n, 2))
    return coords, rng.integers(0, T, n)


def clustered_input(clumps=1800, sigma=30.0, background=100_000):
    rng = np.random.default_rng(43)
    centres = rng.uniform(0, 1.0e4, (clumps, 2))
    in_clumps = centres[rng.integers(0, clumps, n - background)] + rng.normal(0, sigma, (n - background, 2))
    coords = np.concatenate([in_clumps, rng.uniform(0, 1.0e4, (background, 2))])
    return coords, rng.integers(0, T, n)


def probe(coords, codes):
    labels = np.array([f"type{v:02d}" for v in range(T)])[codes]

    def adata():
        obs = pd.DataFrame({"cell_type": labels}, index=pd.RangeIndex(n).astype(str))
        return SimpleAnnData(np.zeros((n, 1)), obs=obs, var_names=["g0"], obsm={"spatial": coords})

    def timed(fn, key):
        a = adata()
        ctx.sync()
        t0 = time.perf_counter()
        fn(a, "cell_type", radii, n_permutations=P, seed=0, rng="philox")
        ctx.sync()
        return time.perf_counter() - t0, a.uns[key], a.uns["spatialcore_metadata"]["operations"][-1]["outputs"]

    routes = {"g": (ripley_g, "ripley_g"), "k": (ripley_k, "ripley_k")}
    first = {name: timed(*route) for name, route in routes.items()}          # warm-up: code objects, allocations
    g, k = first["g"][1], first["k"][1]
    n_entries = first["g"][2]["n_entries"]
    assert n_entries == first["k"][2]["n_pairs"] == int(k["count"][:, :, -1].sum())
    assert (g["count"] <= np.minimum(g["n_per_type"][:, None, None], k["count"])).all()
    assert ((g["count"] > 0) == (k["count"] > 0)).all() and (np.diff(g["count"], axis=2) >= 0).all()
    walls = {name: [] for name in routes}
    kernels = []
    for _ in range(REPS):
        for name, route in routes.items():
            if name == "g":
                ctx.reset_timers()
            walls[name].append(timed(*route)[0])
            if name == "g":
                kernels.append({what: ctx.kernel_time(kid) for what, kid in (
                    ("list_build", _lib.K_RIPLEY_G_LIST), ("relabel", _lib.K_RIPLEY_G_RELABEL), ("counting", _lib.K_RIPLEY_G_COUNT))})
    med = {name: float(np.median(w)) for name, w in walls.items()}
    return {
        "ripley_g_s": walls["g"], "ripley_k_s": walls["k"], "ripley_g_median_s": med["g"], "ripley_k_median_s": med["k"],
        "ratio_g_over_k": med["g"] / med["k"],
        "ripley_g_kernel_ms": {what: [rep[what][0] for rep in kernels] for what in kernels[0]},
        "ripley_g_kernel_launches": {what: kernels[0][what][1] for what in kernels[0]},
        "list_entries": n_entries, "mean_row_length": n_entries / n, "bytes_per_entry": 5,
        "ripley_k_stored_pairs": n_entries // 2,
        "G_at_r_max_min_max": [float(np.nanmin(g["G"][:, :, -1])), float(np.nanmax(g["G"][:, :, -1]))],
    }


out = {
    "workload": f"{n} cells on 1e4 x 1e4, {T} independent cell types, radii {radii}, {P} permutations, rng=philox; "
                f"ripley_g and ripley_k alternating in one process, one warm-up then {REPS} repetitions",
    "bytes_per_entry_note": "one int32 column position + one radius-index byte per ORDERED pair, plus one int64 offset per cell",
    "uniform": probe(*uniform_input()),
    "clustered": probe(*clustered_input()),
    "clustered_note": "900 000 cells in 1800 Gaussian clumps (sigma 30) + 100 000 uniform background cells",
    "device_mem_bytes": ctx.device_mem(),
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ripley_g_1m.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
