"""The two paths of the cross search, sc_knn_cross: the direct kernels (path 1) against the certified Gram-form filter
(path 2) on PCA-like features (tests/neighbors_restated.py: pca_like), k = 15, over (n_query, n_ref, d): one warm-up call,
then the best of three per point.  The `path = 0` rule of sc_knn_cross is read off this table.  Writes
profiles/ingest_sweep.json (or the path given).

Usage:  python scripts/ingest_sweep.py [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import neighbors_restated as N  # noqa: E402
from spatialcore_amd import _lib  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ingest_sweep.json")
ctx = _lib.default_context(0)
rows = []
for n_ref in (2000, 10000, 50000, 100000):
    for n_query in (500, 2000, 10000, 50000):
        for d in (20, 32, 50):
            R, Q = N.pca_like(n_ref, d, 1), N.pca_like(n_query, d, 2)
            row = {"n_query": n_query, "n_ref": n_ref, "d": d}
            for path in (1, 2):
                ctx.knn_cross(R, Q, 15, fetch=False, path=path)
                ts = []
                for _ in range(3):
                    ctx.sync()
                    t = time.perf_counter()
                    ctx.knn_cross(R, Q, 15, fetch=False, path=path)
                    ctx.sync()
                    ts.append(time.perf_counter() - t)
                row[f"path{path}_ms"] = round(min(ts) * 1e3, 2)
            print(row, flush=True)
            rows.append(row)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rows, f)
