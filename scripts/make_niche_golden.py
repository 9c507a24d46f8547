"""Generate tests/golden/ref_niches.npz from the reference's own identify_niches (sklearn's KMeans).

Build container only: needs the reference's source tree (REF_SRC) and sklearn.  The reference module is imported
with inert stand-ins for the absent ``anndata`` (the technique of oracle/make_golden.py); only data is written.

Per case: the input profiles (shared by the cases of one profile kind), labels, centroids, inertia and params of the
reference, the sklearn version, every run's k-means++ seed indices (recorded by wrapping sklearn's
``_kmeans_plusplus``), a per-run ``seed_stable`` flag (the seeds do not change when the float32 potential that scales
the draws is moved by +-2 ulps, recomputed with sklearn's own helpers) and ``label_margin`` (the smallest relative gap
over all cells between the nearest and the second-nearest reference centroid).

Usage:  python scripts/make_niche_golden.py
"""

from __future__ import annotations

import importlib
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "ref_niches.npz")
REF_SRC = "/root/reference/src"

sys.path.insert(0, ROOT)
from spatialcore_amd._adata import SimpleAnnData  # noqa: E402


def import_reference():
    ad = types.ModuleType("anndata")
    ad.AnnData = SimpleAnnData
    sys.modules["anndata"] = ad
    for name, sub in (("spatialcore", ""), ("spatialcore.core", "core"), ("spatialcore.spatial", "spatial")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF_SRC, "spatialcore", sub)]
        sys.modules[name] = pkg
    return importlib.import_module("spatialcore.spatial.neighborhoods")


def tissue(n, seed):
    """Labelled synthetic tissue: cell-type mixtures that vary over a few spatial regions."""
    rng = np.random.default_rng(seed)
    L = np.sqrt(n) * 10.0
    coords = rng.uniform(0, L, (n, 2))
    types_ = np.array(["T", "B", "Mac", "Epi", "Fib", "Endo", "NK"])
    mix = rng.dirichlet(np.full(types_.size, 0.6), size=6)
    region = (np.floor(coords[:, 0] / (L / 3)).astype(int) + 3 * (coords[:, 1] > L / 2)).clip(0, 5)
    labels = np.array([rng.choice(types_, p=mix[r]) for r in region])
    return coords, labels


def adata_of(coords, labels):
    obs = pd.DataFrame({"cell_type": labels}, index=pd.RangeIndex(len(labels)).astype(str))
    return SimpleAnnData(np.zeros((len(labels), 1)), obs=obs, var_names=["g0"], obsm={"spatial": coords})


RECORD = []


def install_seed_recorder():
    import sklearn.cluster._kmeans as km

    orig = km._kmeans_plusplus

    def wrapped(X, n_clusters, x_squared_norms, sample_weight, random_state, n_local_trials=None):
        state = random_state.get_state()
        centers, indices = orig(X, n_clusters, x_squared_norms, sample_weight, random_state, n_local_trials)
        RECORD.append({"X": X, "xsq": x_squared_norms, "w": sample_weight, "state": state, "indices": indices.copy()})
        return centers, indices

    km._kmeans_plusplus = wrapped


def seeds_with_pot_shift(rec, K, ulps):
    """sklearn's k-means++ (its own helpers) with the potential moved by `ulps` float32 ulps before every draw."""
    from sklearn.metrics.pairwise import _euclidean_distances
    from sklearn.utils.extmath import stable_cumsum

    X, xsq, w = rec["X"], rec["xsq"], rec["w"]
    rs = np.random.RandomState()
    rs.set_state(rec["state"])
    n = X.shape[0]
    L = 2 + int(np.log(K))
    idx = [rs.choice(n, p=w / w.sum())]
    closest = _euclidean_distances(X[idx[0]][None, :], X, Y_norm_squared=xsq, squared=True)
    pot = closest @ w
    for _ in range(1, K):
        p = np.asarray(pot, dtype=X.dtype)
        for _ in range(abs(ulps)):
            p = np.nextafter(p, np.inf if ulps > 0 else -np.inf, dtype=X.dtype)
        rand_vals = rs.uniform(size=L) * p
        cand = np.searchsorted(stable_cumsum(w * closest), rand_vals)
        np.clip(cand, None, closest.size - 1, out=cand)
        dc = _euclidean_distances(X[cand], X, Y_norm_squared=xsq, squared=True)
        np.minimum(closest, dc, out=dc)
        cp = dc @ w.reshape(-1, 1)
        b = int(np.argmin(cp))
        pot = cp[b]
        closest = dc[b]
        idx.append(int(cand[b]))
    return np.array(idx)


def label_margin(X, centroids):
    d = ((X.astype(np.float64)[:, None, :] - centroids.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    d.sort(axis=1)
    return float(np.min((d[:, 1] - d[:, 0]) / np.maximum(d[:, 1], 1e-300)))


def main():
    import sklearn

    nb = import_reference()
    install_seed_recorder()
    coords, labels = tissue(6000, 17)
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    profiles = {}
    for kind, kw in (("knn", dict(method="knn", k=15)), ("radius", dict(method="radius", radius=30.0)),
                     ("knn_raw", dict(method="knn", k=10, normalize=False))):
        a = adata_of(coords, labels)
        nb.compute_neighborhood_profile(a, celltype_column="cell_type", **kw)
        profiles[kind] = np.asarray(a.obsm["neighborhood_profile"])
    base = profiles["knn"]
    uniq = np.unique(base, axis=0)[:5]
    profiles["dup"] = uniq[np.random.default_rng(3).integers(0, 5, 2000)]
    for kind, P in profiles.items():
        out[f"profile_{kind}"] = P

    cases = [  # name, profile kind, K, n_init, random_state, max_iter
        ("knn_k5", "knn", 5, 10, 0, 300),
        ("knn_k8", "knn", 8, 10, 7, 300),
        ("knn_k8_init1", "knn", 8, 1, 0, 300),
        ("radius_k2", "radius", 2, 10, 0, 300),
        ("raw_k12", "knn_raw", 12, 10, 3, 300),
        ("knn_k8_iter2", "knn", 8, 10, 0, 2),
        ("dup_k8", "dup", 8, 10, 0, 300),
    ]
    out["cases"] = np.array([c[0] for c in cases])
    for name, kind, K, n_init, rs, max_iter in cases:
        a = SimpleAnnData(np.zeros((profiles[kind].shape[0], 1)), var_names=["g0"],
                          obsm={"neighborhood_profile": profiles[kind]})
        RECORD.clear()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            nb.identify_niches(a, n_niches=K, random_state=rs, n_init=n_init, max_iter=max_iter)
        warn = [str(w.message) for w in caught if type(w.message).__name__ == "ConvergenceWarning"]
        seeds = np.stack([r["indices"] for r in RECORD])
        stable = np.array([all(np.array_equal(seeds_with_pot_shift(r, K, d), r["indices"]) for d in (-2, 2, 0))
                           for r in RECORD])
        cat = a.obs["niche"]
        out[f"{name}_kind"] = np.array(kind)
        out[f"{name}_labels"] = cat.cat.codes.to_numpy().astype(np.int32)
        out[f"{name}_categories"] = np.array(list(cat.cat.categories))
        out[f"{name}_centroids"] = np.asarray(a.uns["niche_centroids"])
        prm = a.uns["niche_params"]
        out[f"{name}_inertia"] = np.array(prm["inertia"])
        for k in ("n_niches", "random_state", "n_init", "max_iter"):
            out[f"{name}_{k}"] = np.array(prm[k])
        out[f"{name}_seeds"] = seeds
        out[f"{name}_seed_stable"] = stable
        out[f"{name}_label_margin"] = np.array(label_margin(profiles[kind], out[f"{name}_centroids"]))
        out[f"{name}_warning"] = np.array(warn[0] if warn else "")
        print(f"{name}: inertia {prm['inertia']:.6g} seeds stable {stable.sum()}/{stable.size} "
              f"margin {out[f'{name}_label_margin']:.2e} warning {bool(warn)}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
