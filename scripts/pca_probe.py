"""pca at 10^6 cells x 500 genes of the bench's synthetic counts, normalize=True, 50 components.
The public call's wall time; its parts measured on their own (canonical CSR on the host, sc_pca_begin: upload and
normalisation, sc_pca_gram, the host's eigenproblem, sc_pca_project with its read-back); the HIP-event times per kernel
family (sc_ctx_kernel_time); the Gram scope's fraction of the fp64 matrix peak and of the HBM peak on its compulsory
bytes; the host eigenproblem alone at G = 4096.  Baseline: sklearn's PCA(svd_solver="covariance_eigh") on this host at
the first 10^5 cells (normalised on the host, not timed), scaled linearly to 10^6 cells and labelled as extrapolated.
Writes profiles/pca_1m.json (or the path given last).

Usage:  python scripts/pca_probe.py [n_cells [n_genes [baseline_cells [out.json]]]]"""
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
from spatialcore_amd.pca import decompose, pca  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 500
n_base = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "pca_1m.json")
K = 50
HBM_PEAK = 8.0e12        # bytes / s, MI355X
FP64_MATRIX_PEAK = 78.6e12   # flop / s: AMD's MI355X data sheet, "peak double precision matrix (FP64)"; not measured here
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
nnz = int(X.nnz)
say(f"input: {n} x {G}, {nnz} stored entries ({time.perf_counter() - t0:.1f} s)")
names = [f"g{i}" for i in range(G)]

pca(SimpleAnnData(X[:4096], var_names=names), K, normalize=True)      # code objects, allocations
ad = SimpleAnnData(X, var_names=names)
wall, _ = timed(pca, ad, K, normalize=True)
say(f"public call {wall:.2f} s")

t_csr, (Xc, _) = timed(_sparse_input.canonical_csr, X, np.arange(G), G, negative="negative", all_zero="all zero", real=True)   # as pca asks
ctx.reset_timers()
t_begin, _ = timed(ctx.pca_begin, Xc.indptr, Xc.indices, Xc.data, G, True, 1e4)
t_gram, (colsum, gram) = timed(ctx.pca_gram)
t_host, host = timed(decompose.host_decompose, gram, colsum, n, K, False)
t_ops, (Vs, offset) = timed(decompose.projection_operands, host["components"], host["mean"], host["scale"])
t_proj, scores = timed(ctx.pca_project, Vs, offset, np.float32)
device_mem = ctx.device_mem()      # the resident matrix, the partial sums and the scores, before sc_pca_end frees them
ctx.pca_end()
np.testing.assert_array_equal(scores, ad.obsm["X_pca"])      # the parts are the call
kern = {what: ctx.kernel_time(kid) for what, kid in (("setup", _lib.K_PCA_SETUP), ("gram", _lib.K_PCA_GRAM),
                                                     ("project", _lib.K_PCA_PROJECT))}
# the Gram kernel: what the formulation asks for (the upper triangle with its diagonal, one multiply and one add per row)
# and what the MFMA kernel executes (64 x 64 quarters of 128 x 128 blocks: 3 of a diagonal block, 4 of any other)
nb = -(-G // 128)
quarters = 3 * nb + 4 * (nb * (nb - 1) // 2)
flops_useful = float(n) * G * (G + 1)
flops_executed = 2.0 * n * quarters * 64 * 64
gram_s = kern["gram"][0] * 1e-3
compulsory = nnz * 12 + (n + 1) * 8 + G * G * 8      # the CSR once (int32 index + fp64 value, row pointers), the result once

t_e4096 = None
if G <= 4096:
    rng = np.random.default_rng(0)
    B = rng.normal(size=(4096, 512))
    C4096 = B @ B.T / 512 + np.diag(rng.uniform(0.5, 1.5, 4096))
    t = time.perf_counter()
    decompose.eigen_decompose(C4096, K)
    t_e4096 = time.perf_counter() - t
    say(f"host eigenproblem at G = 4096: {t_e4096:.1f} s")

from sklearn.decomposition import PCA  # noqa: E402

Xb = sparse.csr_matrix(X[:n_base], dtype=np.float64)
s = np.asarray(Xb.sum(axis=1)).ravel()
Xb.data = np.log1p(Xb.data / np.repeat(s, np.diff(Xb.indptr)) * 1e4)
t = time.perf_counter()
PCA(n_components=K, svd_solver="covariance_eigh").fit_transform(Xb)
t_sk = time.perf_counter() - t
say(f"sklearn covariance_eigh at {n_base} cells: {t_sk:.2f} s")

out = {
    "workload": f"{n} cells x {G} genes of bench.synth_inputs(seed=42) (float32 counts), {nnz} stored entries, normalize=True, "
                f"{K} components, dtype float32; one small warm-up call, then one timed call",
    "stored_entries": nnz, "public_call_s": wall,
    "parts_s": {"host_canonical_csr": t_csr, "sc_pca_begin": t_begin, "sc_pca_gram": t_gram, "host_decompose": t_host,
                "host_projection_operands": t_ops, "sc_pca_project": t_proj},
    "kernel_ms": {k: v[0] for k, v in kern.items()}, "kernel_scopes": {k: v[1] for k, v in kern.items()},
    "gram": {"scope": "k_pca_gram + k_pca_gram_reduce + k_pca_colsum (HIP events around the three launches)",
             "flops_useful": flops_useful, "flops_executed_by_mfma": flops_executed,
             "fp64_matrix_peak_flops": FP64_MATRIX_PEAK,
             "fp64_matrix_peak_source": "AMD Instinct MI355X data sheet (78.6 TFLOP/s FP64 matrix); taken as published, not measured",
             "useful_fraction_of_fp64_matrix_peak": flops_useful / gram_s / FP64_MATRIX_PEAK,
             "executed_fraction_of_fp64_matrix_peak": flops_executed / gram_s / FP64_MATRIX_PEAK,
             "compulsory_bytes": compulsory, "hbm_peak_bytes_per_s": HBM_PEAK,
             "compulsory_fraction_of_hbm_peak": compulsory / gram_s / HBM_PEAK},
    "host_eigenproblem_s": {"G": G, "host_decompose": t_host, "eigen_decompose_at_G_4096": t_e4096,
                            "cpus": os.cpu_count(), "threads_env": os.environ.get("OMP_NUM_THREADS")},
    "sklearn_same_host": {"solver": "covariance_eigh", "cells": n_base, "fit_transform_s": t_sk,
                          "fit_transform_s_extrapolated_to_n": t_sk * n / n_base, "extrapolated": True,
                          "note": "normalised on the host beforehand (not timed); linear scaling in the cells"},
    "device_mem_bytes": device_mem,
}
out["speedup_vs_extrapolated_sklearn"] = out["sklearn_same_host"]["fit_transform_s_extrapolated_to_n"] / wall
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
say(json.dumps(out, indent=1))
