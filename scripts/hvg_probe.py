"""highly_variable_genes at two shapes of the bench's synthetic counts: 10^6 cells x 500 genes, and 25,000 cells x 20,000
genes (the same 5 x 10^8 pairs, whole-transcriptome width).  Per shape: the public call's wall time; its parts (canonical
CSR on the host, sc_hvg_pearson with upload and read-back); the HIP-event times per kernel family (sc_ctx_kernel_time)
averaged over REPS calls; the dense kernel's pair rate against the fp64 vector issue bound; the number of distinct row
sums (what grouping cells of equal row sum could save in the dense term); the numpy textbook version (densify 1000 genes
at a time, every residual, np.var) on this host at a size it can run, scaled linearly in the pairs and labelled as
extrapolated, and the device's result checked against it at that size.  Writes profiles/hvg_1m.json (or the path given).

Usage:  python scripts/hvg_probe.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib, _sparse_input  # noqa: E402
from spatialcore_amd.preprocessing import highly_variable_genes  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hvg_1m.json")
SHAPES = ((1_000_000, 500, 100_000, 500), (25_000, 20_000, 25_000, 2_000))   # cells, genes, baseline cells, baseline genes
REPS = 5
THETA = 100.0
# k_hvg_dense's loop as hipcc compiles it for gfx950 (-O3 -ffp-contract=off): 173 vector instructions per four pairs, of
# which 140 are fp64 arithmetic (8 of them v_rsq_f64 / v_rcp_f64) and 32 are 32-bit selects.  The bound prices every one at
# 4 cycles per wave-instruction (MI355X: 256 CUs x 4 SIMDs, wave64); the issue cost of the fp64 rsq / rcp is not known to
# be 4, so the bound is an upper bound on the rate.
DENSE_VALU_PER_PAIR = 173 / 4
SIMDS, CYCLES_PER_VALU, PEAK_CLOCK_HZ = 256 * 4, 4, 2.4e9
ctx = _lib.default_context(0)


def say(*a):
    print(*a, flush=True)


def timed(fn, *a, **kw):
    ctx.sync()
    t = time.perf_counter()
    r = fn(*a, **kw)
    ctx.sync()
    return time.perf_counter() - t, r


def textbook_chunked(X, theta, chunk=1000):
    """The textbook algorithm on a CSR: residual variances, densifying ``chunk`` genes at a time."""
    n, G = X.shape
    s = np.asarray(X.sum(axis=1), dtype=np.float64).reshape(-1, 1)
    t = np.asarray(X.sum(axis=0), dtype=np.float64).reshape(1, -1)
    total, clip = t.sum(), np.sqrt(n)
    Xc = X.tocsc()
    out = np.empty(G)
    for g0 in range(0, G, chunk):
        g1 = min(g0 + chunk, G)
        A = Xc[:, g0:g1].toarray().astype(np.float64)
        mu = s * t[:, g0:g1] / total
        with np.errstate(divide="ignore", invalid="ignore"):
            z = (A - mu) / np.sqrt(mu + mu ** 2 / theta)
        z = np.clip(np.where(mu > 0, z, 0.0), -clip, clip)
        out[g0:g1] = np.var(z, axis=0)
    return out


def probe(n, G, n_base, G_base):
    t0 = time.perf_counter()
    _, dense = bench.synth_inputs(n, G, seed=42)
    X = sparse.csr_matrix(dense)
    del dense
    nnz = int(X.nnz)
    say(f"input: {n} x {G}, {nnz} stored entries ({time.perf_counter() - t0:.1f} s)")
    names = [f"g{i}" for i in range(G)]
    highly_variable_genes(SimpleAnnData(X[:2048], var_names=names), n_top_genes=100)      # code objects, allocations
    ad = SimpleAnnData(X, var_names=names)
    wall, _ = timed(highly_variable_genes, ad, n_top_genes=min(2000, G // 4))
    say(f"public call {wall:.3f} s")
    t_csr, (Xc, _) = timed(_sparse_input.canonical_csr, X, np.arange(G), G, negative="negative", all_zero="all zero", real=True)
    clip = float(np.sqrt(n))
    ctx.hvg_pearson(Xc.indptr, Xc.indices, Xc.data, G, THETA, clip)
    ctx.reset_timers()
    calls = [timed(ctx.hvg_pearson, Xc.indptr, Xc.indices, Xc.data, G, THETA, clip) for _ in range(REPS)]
    kern = {what: ctx.kernel_time(kid) for what, kid in (("setup", _lib.K_HVG_SETUP), ("dense", _lib.K_HVG_DENSE),
                                                         ("sparse", _lib.K_HVG_SPARSE))}
    res = calls[0][1]
    assert all(np.stack(r).tobytes() == np.stack(res).tobytes() for _, r in calls)      # the same bytes every time
    np.testing.assert_array_equal(res[3], ad.var["residual_variances"].values)          # the parts are the call
    dense_s = kern["dense"][0] * 1e-3 / REPS
    pairs = float(n) * G
    bound_rate = SIMDS * 64 * PEAK_CLOCK_HZ / (DENSE_VALU_PER_PAIR * CYCLES_PER_VALU)
    s = np.asarray(X.sum(axis=1)).ravel()
    # the textbook version on this host, and the device against it at that size
    Xb = sparse.csr_matrix(X[:n_base, :G_base], dtype=np.float64)
    t = time.perf_counter()
    want = textbook_chunked(Xb, THETA)
    t_np = time.perf_counter() - t
    got = ctx.hvg_pearson(Xb.indptr, Xb.indices, Xb.data, G_base, THETA, float(np.sqrt(n_base)))[3]
    pos = want > 0
    err = float(np.max(np.abs(got[pos] - want[pos]) / want[pos]))
    assert err <= 1e-10 and not got[~pos].any(), err
    scale = pairs / (float(n_base) * G_base)
    say(f"numpy textbook at {n_base} x {G_base}: {t_np:.2f} s; device against it {err:.1e}")
    return {
        "workload": f"{n} cells x {G} genes of bench.synth_inputs(seed=42) (float32 counts), {nnz} stored entries, theta = {THETA:g}, "
                    f"clip = sqrt(cells); one small warm-up call, then one timed public call; the entry point alone {REPS} times",
        "pairs": pairs, "stored_entries": nnz, "density": nnz / pairs, "public_call_s": wall,
        "parts_s": {"host_canonical_csr": t_csr, "sc_hvg_pearson_min": min(c[0] for c in calls),
                    "sc_hvg_pearson_median": float(np.median([c[0] for c in calls]))},
        "kernel_ms_per_call": {k: v[0] / REPS for k, v in kern.items()},
        "kernel_scopes": {"setup": "k_hvg_rows, the column sort and chunk table (sc_colsort.h), k_hvg_colsum_chunks, k_hvg_gene_add, k_hvg_total",
                          "dense": "k_hvg_dense + k_chunk_add", "sparse": "k_hvg_correct_chunks + k_hvg_finish"},
        "dense": {"pairs_per_s": pairs / dense_s, "valu_instructions_per_pair": DENSE_VALU_PER_PAIR,
                  "issue_bound_pairs_per_s_at_2.4GHz": bound_rate, "fraction_of_issue_bound": pairs / dense_s / bound_rate,
                  "bound": "fp64 vector issue: vector instructions per pair x 4 cycles per wave-instruction on 1024 SIMDs at the peak "
                           "clock of 2.4 GHz; the clock under load was not measured, and v_rsq_f64 / v_rcp_f64 are priced as ordinary",
                  "bytes_read_per_pair": 8.0 / 64, "note": "one scalar load of s_i per cell and wavefront: not memory-bound"},
        "distinct_row_sums": int(np.unique(s).size), "cells_without_a_count": int(np.count_nonzero(s == 0)),
        "numpy_textbook_same_host": {"cells": n_base, "genes": G_base, "seconds": t_np, "seconds_extrapolated_to_shape": t_np * scale,
                                     "extrapolated": True, "note": "1000 genes densified at a time; linear scaling in the pairs",
                                     "device_against_it_max_rel": err, "cpus": os.cpu_count(),
                                     "threads_env": os.environ.get("OMP_NUM_THREADS")},
        "speedup_vs_extrapolated_numpy": t_np * scale / wall,
        "device_mem_bytes_after": ctx.device_mem(),
    }


out = {"shapes": [probe(*shape) for shape in SHAPES]}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
say(json.dumps(out, indent=1))
