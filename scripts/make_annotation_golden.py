"""Generate tests/golden/ref_annotation.npz from the reference's own transform_confidence (annotation/confidence.py).

Build container only: needs the reference's source tree (REF_SRC).  The reference module is imported with inert
stand-ins for the absent ``anndata`` and for its package __init__ (the technique of scripts/make_threshold_golden.py);
only arrays are written, with allow_pickle=False on the reading side.

Per case ``c`` the file holds the float64 matrix (``c_scores``; its float32 rounding is what the reference really sees,
because it reads ``obsm``), and per method the reference's result on the float32 rounding (``c_METHOD_f32``) and on the
float64 matrix itself (``c_METHOD_f64``), with the deviation of tests/annotation_restated.py's ``confidences``
from each (``..._dev``) and the restatement's spread under a one-ulp move of every exp result (``..._ulp``): the
device-against-reference tolerance is 4 x the deviation, or 16 x the spread where the deviation is exactly 0 (the rule of
tests/threshold_restated.py: reference_tolerance).

Usage:  python scripts/make_annotation_golden.py
"""

from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "ref_annotation.npz")
REF_SRC = "/root/reference/src"
METHODS = ("raw", "zscore", "softmax", "minmax")

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from spatialcore_amd._adata import SimpleAnnData  # noqa: E402
import annotation_restated as ar  # noqa: E402


def import_reference():
    ad = types.ModuleType("anndata")
    ad.AnnData = SimpleAnnData
    sys.modules["anndata"] = ad
    for name, sub in (("spatialcore", ""), ("spatialcore.core", "core"), ("spatialcore.annotation", "annotation")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF_SRC, "spatialcore", sub)]
        sys.modules[name] = pkg
    return importlib.import_module("spatialcore.annotation.confidence")


def cases():
    rng = np.random.default_rng(2024)
    special = np.array([
        [1.25, 1.25, 1.25, 1.25, 1.25],              # all scores equal
        [0.5, 0.5 + 3e-11, 0.5 + 1e-11, 0.5, 0.5],   # range < 1e-10 as float64 (float32 rounds the row to all equal)
        [2.0, -1.0, 2.0, 0.5, 2.0],                  # an exact tie for the maximum
        [-7.5, -3.25, -9.0, -3.5, -12.0],            # negative scores
        [-0.125, -0.125, -6.0, -0.125, -30.0],       # negative, tied
        [5.0, 0.1, 0.1, 0.1, 0.1],
        [2.0, 1.8, 1.9, 1.7, 1.6],
    ])
    out = {"special": special,
           # guards reached from both sides by values that survive the float32 rounding: 0 < range, std < 1e-10; range and
           # std above 1e-10; range above, std below; the same below zero
           "tiny": np.array([[1e-11, 4e-11, 2e-11, 3e-11, 0.0, 1.5e-11, 2.5e-11, 3.5e-11, 5e-12, 1e-11],
                             [0.0, 4e-10, 2e-10, 3e-10, 1e-10, 3.5e-10, 5e-11, 2.5e-10, 1.5e-10, 4e-10],
                             [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5e-10],
                             [-4e-11, -1e-11, -3e-11, -2e-11, -5e-11, -1.5e-11, -2.5e-11, -3.5e-11, -4.5e-11, -1e-11]]),
           "two": np.array([[0.3, -0.7], [-4.0, -4.0], [-2.0, 1.5], [10.0, -10.0]]),        # T = 2
           "negative33": -np.abs(rng.normal(3.0, 2.0, size=(40, 33))),
           "mixed70": rng.normal(-2.0, 4.0, size=(50, 70)),                                 # more than one wavefront
           "wide130": rng.normal(-5.0, 3.0, size=(20, 130))}
    out["mixed70"][3, 10] = out["mixed70"][3].max() + 1.0
    out["mixed70"][3, 55] = out["mixed70"][3, 10]                                           # a tie across lane blocks
    return out


def main():
    ref = import_reference()
    store = {"methods": np.array(METHODS), "cases": np.array(sorted(cases()))}
    for name, S in cases().items():
        S32 = S.astype(np.float32)
        store[f"{name}_scores"] = S
        for wide, M in (("f32", S32), ("f64", S)):      # the float64 values themselves, not the rounded ones widened
            mine, spread = ar.ulp_tolerance(lambda e: ar.confidences(M.astype(np.float64), e), METHODS)
            for method in METHODS:
                got = np.asarray(ref.transform_confidence(M, method=method))
                store[f"{name}_{method}_{wide}"] = got
                dev = float(np.max(np.abs(got.astype(np.float64) - mine[method])))
                store[f"{name}_{method}_{wide}_dev"] = np.float64(dev)
                store[f"{name}_{method}_{wide}_ulp"] = np.float64(np.max(spread[method]) / 16.0)
                print(f"{name:>10} {method:>8} {wide}: restatement deviates {dev:.3e}")
    np.savez(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
