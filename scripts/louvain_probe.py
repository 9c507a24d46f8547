"""louvain at 10^6 cells of the bench's synthetic counts: pca (50 components, normalize=True), then louvain on X_pca.
The public call's wall time; its parts measured on their own (the neighbour search, the symmetric union with its kernel
weights, the weights' read-back and quantisation on the host, the adoption of the resident graph, every level); the
HIP-event time of the move kernels per round at level 0; the move kernels' compulsory bytes per round as a fraction of
the HBM peak -- derived from the formulation (the CSR once, comm and tot once each way), no counters are read; the final
modularity.  Baseline: networkx 3.4.2 louvain_communities (seed 0) on this host on the graph of the first `baseline_cells`
cells, scaled linearly in the cells and labelled as extrapolated.  Writes profiles/louvain_1m.json (or the path given last).

Usage:  python scripts/louvain_probe.py [n_cells [n_genes [baseline_cells [out.json]]]]"""
import json
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.cluster import communities, louvain  # noqa: E402
from spatialcore_amd.pca import pca  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 500
n_base = int(sys.argv[3]) if len(sys.argv) > 3 else 50_000
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "louvain_1m.json")
K, NEIGHBORS = 50, 15
HBM_PEAK = 8.0e12        # bytes / s, MI355X
ctx = _lib.default_context(0)


def say(*a):
    print(*a, flush=True)


def timed(fn, *a, **kw):
    ctx.sync()
    t = time.perf_counter()
    r = fn(*a, **kw)
    ctx.sync()
    return time.perf_counter() - t, r


t0 = time.perf_counter()
_, dense = bench.synth_inputs(n, G, seed=42)
X = sparse.csr_matrix(dense)
del dense
say(f"input: {n} x {G}, {X.nnz} stored entries ({time.perf_counter() - t0:.1f} s)")
names = [f"g{i}" for i in range(G)]
ad = SimpleAnnData(X, var_names=names)
t_pca, _ = timed(pca, ad, K, normalize=True)
say(f"pca {t_pca:.2f} s")
R = np.ascontiguousarray(ad.obsm["X_pca"])

small = SimpleAnnData(X[:4096], var_names=names)      # code objects, allocations
small.obsm["X_pca"] = R[:4096]
louvain(small, n_neighbors=NEIGHBORS)
wall, _ = timed(louvain, ad, n_neighbors=NEIGHBORS)
info = ad.uns["louvain"]
say(f"public call {wall:.2f} s, {len(info['levels'])} levels, modularity {info['modularity']:.4f}")

# the parts
g = communities.resolution_units(1.0)
t_search, _ = timed(ctx.knn_dense, R, NEIGHBORS, False)
t_graph, ginfo = timed(ctx.diffmap_graph)
nnz = int(ginfo["n_edges"])
t_weights, (q, scale) = timed(lambda: communities.quantise_weights(ctx.louvain_resident_weights()))
t_begin, _ = timed(ctx.louvain_begin_resident, q, g, 500)
levels, t_levels, move_ms = [], [], []
while True:
    ctx.reset_timers()
    t, lv = timed(ctx.louvain_level)
    ms, scopes = ctx.kernel_time(_lib.K_LOUVAIN_MOVE)
    other_ms, _ = ctx.kernel_time(_lib.K_LOUVAIN_LEVEL)
    lv.pop("labels")
    lv["qnum"] = str(lv["qnum"])
    lv.update(call_s=t, move_kernels_ms=ms, move_launches=scopes, split_and_aggregation_ms=other_ms)
    levels.append(lv)
    say(f"level {len(levels) - 1}: {lv['n_vertices']} vertices, {lv['rounds']} rounds, {t:.3f} s, move kernels {ms:.1f} ms "
        f"in {scopes} launches, rows {lv['rows_wavefront']} / {lv['rows_workgroup']} / {lv['rows_global']}")
    if lv["finished"]:
        break
t_labels, labels = timed(ctx.louvain_labels, n)
device_mem = ctx.device_mem()
ctx.louvain_end()
np.testing.assert_array_equal(labels, np.asarray(ad.obs["louvain"].cat.codes))      # the parts are the call
l0 = levels[0]
per_round_ms = l0["move_kernels_ms"] / l0["move_launches"]
# a round at level 0: row offsets, int32 columns and uint16 weights once; comm read per vertex and written; tot copied, read
compulsory = (n + 1) * 8 + nnz * (4 + 2) + n * (4 + 4) + n * (8 + 8 + 8)
say(f"level 0: {per_round_ms:.3f} ms per launch, compulsory {compulsory / 1e6:.1f} MB = "
    f"{compulsory / (per_round_ms * 1e-3) / HBM_PEAK:.3f} of the HBM peak")

import networkx as nx  # noqa: E402

ctx.knn_dense(R[:n_base], NEIGHBORS, False)
ctx.diffmap_graph()
indptr, indices, w = ctx.diffmap_graph_get()
qb, _ = communities.quantise_weights(w)
Gx = nx.from_scipy_sparse_array(sparse.csr_matrix((qb.astype(np.float64), indices, indptr), shape=(n_base, n_base)))
t = time.perf_counter()
parts = nx.community.louvain_communities(Gx, seed=0)
t_nx = time.perf_counter() - t
q_nx = nx.community.modularity(Gx, parts)
sub = SimpleAnnData(X[:n_base], var_names=names)
sub.obsm["X_pca"] = R[:n_base]
t_sub, _ = timed(louvain, sub, n_neighbors=NEIGHBORS)
say(f"networkx at {n_base} cells: {t_nx:.1f} s, modularity {q_nx:.4f}; ours there {t_sub:.2f} s, {sub.uns['louvain']['modularity']:.4f}")

out = {
    "workload": f"{n} cells x {G} genes of bench.synth_inputs(seed=42) -> pca({K}, normalize=True) -> louvain(n_neighbors={NEIGHBORS}), "
                f"resolution 1, kernel weights; one small warm-up call, then one timed call",
    "pca_s": t_pca, "public_call_s": wall, "stored_entries": nnz, "weight_scale": scale,
    "parts_s": {"sc_knn_dense": t_search, "sc_diffmap_graph": t_graph, "weights_read_back_and_quantised_on_the_host": t_weights,
                "sc_louvain_begin_resident": t_begin, "sc_louvain_level_all": sum(lv["call_s"] for lv in levels),
                "sc_louvain_labels": t_labels},
    "graph_build_s": t_search + t_graph,
    "levels": levels,
    "level0_move": {"scope": "k_lv_move_wave + k_lv_move_wg (both tables) + k_lv_sumsq, HIP events around one round's launches",
                    "ms_per_launch": per_round_ms, "launches": l0["move_launches"],
                    "compulsory_bytes_per_round": compulsory, "hbm_peak_bytes_per_s": HBM_PEAK,
                    "compulsory_fraction_of_hbm_peak": compulsory / (per_round_ms * 1e-3) / HBM_PEAK,
                    "note": "derived from the formulation (CSR once, comm and tot once each way); no counters were collected"},
    "modularity": info["modularity"], "n_clusters": int(labels.max()) + 1, "hit_max_rounds": info["hit_max_rounds"],
    "device_mem_bytes": device_mem,
    "networkx_same_host": {"cells": n_base, "louvain_communities_s": t_nx, "modularity": q_nx,
                           "ours_same_graph_s": t_sub, "ours_same_graph_modularity": sub.uns["louvain"]["modularity"],
                           "louvain_communities_s_extrapolated_to_n": t_nx * n / n_base, "extrapolated": True,
                           "note": "seed 0, quantised kernel weights of the first cells' own graph; linear scaling in the cells"},
}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
say(json.dumps(out, indent=1))
