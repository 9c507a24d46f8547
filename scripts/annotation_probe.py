"""train_celltypist_model and annotate_celltypist at 10^6 cells x 500 genes of the bench's synthetic counts, T = 20
labels (the argmax of 20 fixed random gene programs, standardised so that every class has about n / T cells).
Reports the public-call wall time of both functions, the HIP-event time per training iteration by pass
(sc_ctx_kernel_time: forward row pass, gradient pass, line-search evaluations, step), the prediction kernel, and the compulsory
bytes of each pass against the HBM peak.  Baseline: sklearn's LogisticRegression (lbfgs, one-vs-rest, same C and
max_iter) on this host at the first 10^5 cells, scaled linearly to 10^6 cells (labelled as extrapolated).
Writes profiles/annotation_1m.json.

Usage:  python scripts/annotation_probe.py [n_cells [n_genes [baseline_cells]]]"""
import json
import os
import sys
import time
import warnings

import numpy as np
import pandas as pd
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spatialcore_amd import SimpleAnnData, _lib  # noqa: E402
from spatialcore_amd.annotation import annotate_celltypist, train_celltypist_model  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 500
n_base = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
T, MAX_ITER, TOL = 20, 30, 1e-4
HBM_PEAK = 8.0e12      # bytes / s, MI355X
ctx = _lib.default_context(0)


def say(*a):
    print(*a, flush=True)


t0 = time.perf_counter()
_, dense = bench.synth_inputs(n, G, seed=42)
X = sparse.csr_matrix(dense)
programs = np.random.default_rng(7).normal(size=(G, T)).astype(np.float32)
scores = np.log1p(dense) @ programs
labels = np.argmax((scores - scores.mean(axis=0)) / scores.std(axis=0), axis=1)      # every class about n / T cells
del scores
assert np.bincount(labels, minlength=T).min() > 0
del dense
nnz = int(X.nnz)
say(f"input: {n} x {G}, {nnz} stored entries, class sizes {np.bincount(labels, minlength=T).min()} .. "
    f"{np.bincount(labels, minlength=T).max()} ({time.perf_counter() - t0:.1f} s)")
names = [f"g{i}" for i in range(G)]


def adata(rows=slice(None)):
    obs = pd.DataFrame({"unified_cell_type": [f"type{t:02d}" for t in labels[rows]]})
    obs.index = obs.index.astype(str)
    return SimpleAnnData(X[rows], obs=obs, var_names=names)


def timed(fn, *a, **kw):
    ctx.sync()
    t = time.perf_counter()
    r = fn(*a, **kw)
    ctx.sync()
    return time.perf_counter() - t, r


# compulsory bytes per pass: CSR entry = int32 index + fp64 value
rows_bytes = nnz * 12 + n * T * 8                 # row pass: the entries once, the n x T product written once
grad_bytes = 2 * n * T * 8 + nnz * 12 + n * T * 8     # residuals: scores read, residuals written; column pass: entries, residual rows at least once
line_bytes = 2 * n * T * 8                        # one evaluation: scores and direction product read once
pred_bytes = nnz * 12 + n * T * 4                 # prediction: the entries once, float32 scores written once
gathered = nnz * T * 8                            # the T-value rows fetched per stored entry (table rows / residual rows)

train_celltypist_model(adata(slice(0, 4096)), max_iter=2)          # code objects, allocations
ctx.reset_timers()
wall_train, out = timed(train_celltypist_model, adata(), max_iter=MAX_ITER, tol=TOL)
k = {what: ctx.kernel_time(kid) for what, kid in (("setup", _lib.K_ANNOT_SETUP), ("rows", _lib.K_ANNOT_ROWS),
                                                 ("grad", _lib.K_ANNOT_GRAD), ("line", _lib.K_ANNOT_LINE),
                                                 ("step", _lib.K_ANNOT_STEP))}
iters = int(out["n_iter"].max())
say(f"train: public call {wall_train:.2f} s, {iters} iterations, converged {int(out['converged'].sum())}/{T}")
model = out["model"]
annotate_celltypist(adata(slice(0, 4096)), model=model)
ctx.reset_timers()
wall_pred, ad = timed(annotate_celltypist, adata(), model=model)
kp = ctx.kernel_time(_lib.K_ANNOT_PREDICT)
kps = ctx.kernel_time(_lib.K_ANNOT_SETUP)
say(f"annotate: public call {wall_pred:.2f} s, kernel {kp[0]:.2f} ms")
agree = float(np.mean(ad.obs["cell_type_predicted"].to_numpy() == np.asarray([f"type{t:02d}" for t in labels])))


def baseline():
    from sklearn.linear_model import LogisticRegression
    from sklearn.multiclass import OneVsRestClassifier
    from sklearn.preprocessing import StandardScaler

    Xb = X[:n_base].astype(np.float64)
    rs = np.asarray(Xb.sum(axis=1)).ravel()
    Xb = sparse.diags(1e4 / np.maximum(rs, 1)) @ Xb
    Z = np.minimum(StandardScaler().fit_transform(np.log1p(Xb.toarray())), 10.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = time.perf_counter()
        clf = OneVsRestClassifier(LogisticRegression(C=1.0, solver="lbfgs", max_iter=MAX_ITER)).fit(Z, labels[:n_base])
        fit_s = time.perf_counter() - t
        t = time.perf_counter()
        clf.decision_function(Z)
        pred_s = time.perf_counter() - t
    say(f"sklearn {n_base} cells: fit {fit_s:.1f} s, decision_function {pred_s:.2f} s")
    return {"cells": n_base, "max_iter": MAX_ITER, "fit_s": fit_s, "decision_function_s": pred_s,
            "fit_s_extrapolated_to_n": fit_s * n / n_base, "decision_function_s_extrapolated_to_n": pred_s * n / n_base,
            "extrapolated": True, "note": "dense standardised input prepared outside the timed region"}


res = {
    "workload": f"{n} cells x {G} genes of bench.synth_inputs(seed=42) (float32 counts), {nnz} stored entries, T = {T} classes "
                f"(argmax of {T} standardised random gene programs), balance_cell_type=True, C = 1, tol = {TOL}, max_iter = {MAX_ITER}; "
                "one small warm-up call, then one timed call of each function",
    "stored_entries": nnz, "hbm_peak_bytes_per_s": HBM_PEAK,
    "train": {
        "public_call_s": wall_train, "iterations": iters, "converged_classes": int(out["converged"].sum()),
        "largest_scaled_gradient": float(out["grad_norm"].max()),
        "kernel_ms": {a: v[0] for a, v in k.items()}, "kernel_scopes": {a: v[1] for a, v in k.items()},
        "per_iteration_kernel_ms": {"forward_row_pass": k["rows"][0] / max(k["rows"][1], 1),
                                    "gradient_pass": k["grad"][0] / max(k["grad"][1], 1),
                                    "line_evaluation": k["line"][0] / max(k["line"][1], 1),
                                    "line_evaluations_per_iteration": k["line"][1] / max(iters, 1),
                                    "line_search_per_iteration": k["line"][0] / max(iters, 1),
                                    "step": k["step"][0] / max(k["step"][1], 1)},
        "compulsory_bytes": {"row_pass": rows_bytes, "gradient_pass": grad_bytes, "line_evaluation": line_bytes,
                             "gathered_rows_per_sparse_pass": gathered},
        "compulsory_fraction_of_hbm_peak": {
            "row_pass": rows_bytes / (k["rows"][0] / max(k["rows"][1], 1) * 1e-3) / HBM_PEAK,
            "gradient_pass": grad_bytes / (k["grad"][0] / max(k["grad"][1], 1) * 1e-3) / HBM_PEAK,
            "line_evaluation": line_bytes / (k["line"][0] / max(k["line"][1], 1) * 1e-3) / HBM_PEAK},
    },
    "annotate": {
        "public_call_s": wall_pred, "predict_kernel_ms": kp[0], "setup_kernel_ms": kps[0], "compulsory_bytes": pred_bytes,
        "compulsory_fraction_of_hbm_peak": pred_bytes / (kp[0] * 1e-3) / HBM_PEAK,
        "labels_equal_to_training_labels": agree,
    },
    "sklearn_same_host": baseline(),
    "device_mem_bytes": ctx.device_mem(),
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "annotation_1m.json"), "w") as f:
    json.dump(res, f, indent=1)
say(json.dumps(res, indent=1))
