"""ingest on the device: sc_knn_cross byte for byte against the numpy restatement (tests/ingest_restated.py) on every path
and slack, the tie to the self search, hard inputs, the state it leaves, sc_cross_vote and sc_cross_regress bit for bit,
sklearn on the device's output, and the public functions.

The shapes of SEARCH_CASES straddle the kernels' constants (sc_neighbors.hip): the 16-wide MFMA block, 128 queries per
filter workgroup, the 64-candidate tile, the direct kernels' blocks of 256 / 128 (rows in registers, padded d <= 32) and
64 / 32 (rows in LDS).  Every array has at most 3000 rows but one: ``duplicates(100, 40)`` of the tie test (4000 rows) is
the recipe whose every row holds more exact copies than any list length, so that every row misses the certificate.

The bounds against sklearn are derived in tests/test_cpu_ingest.py (``sklearn_bounds``)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import ingest_restated as IR
import neighbors_restated as NR
from conftest import make_adata
from test_cpu_ingest import GAP, self_from_cross, sklearn_bounds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = [(1, 0), (2, 0), (2, 1), (2, 16)]      # (path, slack)


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


# (n_query, n_ref (None: k), d, k)
SEARCH_CASES = [
    (1, 3000, 50, 16), (1000, 33, 33, 8),                       # the candidates split over workgroups: one query; many queries, few candidates
    (1, None, 1, 1), (15, 31, 3, 2), (16, 63, 8, 9), (17, 64, 9, 17), (127, 65, 32, 32), (128, 129, 33, 1),
    (129, 1000, 64, 2), (257, 3000, 1, 8), (1000, None, 3, 32), (15, 33, 8, 32), (16, 31, 9, 16), (17, 63, 32, 17),
    (127, 64, 64, 9), (128, 65, 50, 16), (129, 129, 33, 17), (257, 1000, 64, 1),
]


def _pair(nq, nref, d, seed):
    """A reference and queries of one family; narrow rows are rounded to integers (ties), and every fifth query is a
    reference row (zero distances)."""
    R = NR.pca_like(nref, d, seed)
    Q = NR.pca_like(nq, d, seed + 100)
    if d <= 3:
        R, Q = np.round(R), np.round(Q)
    Q[::5] = R[(np.arange(0, nq, 5) * 7) % nref]
    return Q, R


def _all_paths(Q, R, k):
    ctx = _ctx()
    out = []
    for path, slack in PATHS:
        idx, d2, info = ctx.knn_cross(R, Q, k, path=path, slack=slack)
        assert info["path"] == path and info["rows_certified"] + info["rows_fallback"] == (Q.shape[0] if path == 2 else 0)
        out.append((idx, d2, info))
    return out


@pytest.mark.parametrize("nq, nref, d, k", SEARCH_CASES, ids=[f"q{a}-r{b or 'k'}-d{c}-k{e}" for a, b, c, e in SEARCH_CASES])
def test_cross_search_equals_the_restatement_on_every_path(nq, nref, d, k):
    nref = k if nref is None else nref
    Q, R = _pair(nq, nref, d, 11 * d + k)
    want_i, want_d = IR.cross_knn(Q, R, k)
    for (idx, d2, info), (path, slack) in zip(_all_paths(Q, R, k), PATHS):
        assert idx.tobytes() == want_i.tobytes(), (path, slack)
        assert d2.tobytes() == want_d.tobytes(), (path, slack)
        if path == 2 and nref < info["list_length"]:
            assert info["rows_fallback"] == 0          # a row that kept fewer than L candidates is certified
    if nref == k:
        np.testing.assert_array_equal(np.sort(want_i, axis=1), np.tile(np.arange(k, dtype=np.int32), (nq, 1)))


def test_the_cases_cover_every_value_twice_and_a_short_reference():
    cols = list(zip(*[(a, b or "k", c, e) for a, b, c, e in SEARCH_CASES]))
    want = [{1, 15, 16, 17, 127, 128, 129, 257, 1000}, {"k", 31, 33, 63, 64, 65, 129, 1000, 3000}, {1, 3, 8, 9, 32, 33, 50, 64},
            {1, 2, 8, 9, 16, 17, 32}]
    for col, values in zip(cols, want):
        assert all(col.count(v) >= 2 for v in values)
    assert any(b is not None and b < e + 16 for _, b, _, e in SEARCH_CASES)      # n_ref < L at slack 16


# ---- the tie to the self search ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pca_like", "lattice", "duplicates"])
def test_cross_search_of_a_set_against_itself_is_the_self_search(name):
    X = {"pca_like": lambda: NR.pca_like(1500, 50, 1), "lattice": lambda: NR.lattice(1500, 2),
         "duplicates": lambda: NR.duplicates(100, 40)}[name]()
    k = 15
    ctx = _ctx()
    si, sd = ctx.knn_dense(X, k)
    for path, slack in PATHS:
        ci, cd, info = ctx.knn_cross(X, X, k + 1, path=path, slack=slack)
        got_i, got_d = self_from_cross(ci, cd)
        assert got_i.tobytes() == si.tobytes() and got_d.tobytes() == sd.tobytes(), (path, slack)
        if name == "duplicates" and path == 2:
            assert info["rows_fallback"] == X.shape[0] and info["rows_certified"] == 0


# ---- hard inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["offset_1e6", "tiny", "huge", "float32", "f32_query_f64_reference"])
def test_hard_inputs(name):
    if name == "f32_query_f64_reference":
        base = NR.recipes(600)["pca_like"]
        R, Q = base[:400], base[400:].astype(np.float32)
    else:
        base = NR.recipes(600)[name]
        R, Q = base[:400], base[400:]
    k = 15
    want_i, want_d = IR.cross_knn(Q, R, k)
    assert np.all(np.isfinite(want_d)) and np.all(want_d[:, -1] > 0)
    for idx, d2, _ in _all_paths(Q, R, k):
        assert idx.tobytes() == want_i.tobytes() and d2.tobytes() == want_d.tobytes()


def test_a_permutation_of_the_reference_finds_every_row_at_distance_zero():
    R = NR.pca_like(1000, 33, 5)
    perm = np.random.default_rng(0).permutation(1000)
    for idx, d2, _ in _all_paths(R[perm], R, 4):
        np.testing.assert_array_equal(d2[:, 0], 0.0)
        np.testing.assert_array_equal(idx[:, 0], perm)


# ---- the state it leaves ----------------------------------------------------------------------------------------------------------------
def test_a_cross_search_leaves_no_self_graph():
    from spatialcore_amd._lib import SpatialCoreHipError

    ctx = _ctx()
    X = NR.pca_like(500, 20, 3)
    ctx.knn_dense_gram(X, 10, fetch=False)
    first = ctx.diffmap_graph()
    graph = ctx.diffmap_graph_get()
    ctx.knn_cross(X, X[:100], 10, fetch=False)
    for call in (ctx.diffmap_graph, ctx.fuzzy_graph, ctx.diffmap_graph_get, lambda: ctx.louvain_begin_resident(None, 1, 10)):
        with pytest.raises(SpatialCoreHipError, match="resident"):
            call()
    ctx.knn_dense_gram(X, 10, fetch=False)
    with pytest.raises(SpatialCoreHipError, match="no cross lists"):      # ... and a self search leaves no cross lists
        ctx.cross_vote(np.zeros(500, dtype=np.int32), 1)
    again = ctx.diffmap_graph()
    assert again["s2"].tobytes() == first["s2"].tobytes() and again["n_edges"] == first["n_edges"]
    for a, b in zip(ctx.diffmap_graph_get(), graph):
        assert a.tobytes() == b.tobytes()


# ---- vote and regress ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gather_lists(k):
    """Lists with rows that hold one and several zero distances: the queries are reference rows, and the reference holds
    every row of its first 40 three times."""
    base = NR.pca_like(300, 12, 9)
    R = np.vstack([base, base[:40], base[:40]])
    Q = np.vstack([NR.pca_like(150, 12, 10), base[:20], base[100:120]])
    idx, d2 = IR.cross_knn(Q, R, k)
    zeros = (d2 == 0.0).sum(axis=1)
    assert (zeros == 0).any() and (zeros == 1).any() and ((zeros > 1) if k > 1 else (zeros == 1)).any()
    return Q, R, idx, d2


@pytest.mark.parametrize("weighting", ["uniform", "distance"])
@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("n_classes", [1, 2, 64, 65, 5000])
def test_vote_equals_the_restatement(n_classes, k, weighting):
    Q, R, idx, d2 = _gather_lists(k)
    codes = np.random.default_rng(n_classes).integers(0, n_classes, size=R.shape[0]).astype(np.int32)
    ctx = _ctx()
    got_i, got_d, _ = ctx.knn_cross(R, Q, k)
    assert got_i.tobytes() == idx.tobytes() and got_d.tobytes() == d2.tobytes()
    label, conf, proba = ctx.cross_vote(codes, n_classes, weighting, proba=True)
    want = IR.vote(idx, d2, codes, n_classes, weighting)
    for got, ref in zip((label, conf, proba), want):
        assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes()
    l2, c2, none = ctx.cross_vote(codes, n_classes, weighting)
    assert none is None and l2.tobytes() == label.tobytes() and c2.tobytes() == conf.tobytes()


def test_vote_supports_32767_classes():
    Q, R, idx, d2 = _gather_lists(32)
    codes = (np.arange(R.shape[0]) * 97 % 32767).astype(np.int32)
    codes[-1] = 32766
    ctx = _ctx()
    ctx.knn_cross(R, Q, 32, fetch=False)
    label, conf, _ = ctx.cross_vote(codes, 32767, "distance")
    want = IR.vote(idx, d2, codes, 32767, "distance")
    assert label.tobytes() == want[0].tobytes() and conf.tobytes() == want[1].tobytes()


def test_a_constructed_vote_tie_goes_to_the_lowest_code():
    """Four reference points at distances 1, 1, 2, 2 from the query (exact in fp64); the codes are laid so that the class
    met first is not the lowest: uniform 2 votes each; distance 1 + 1/2 each."""
    R = np.array([[1.0, 0.0], [0.0, -1.0], [0.0, 2.0], [-2.0, 0.0]])
    Q = np.zeros((1, 2))
    ctx = _ctx()
    idx, d2, _ = ctx.knn_cross(R, Q, 4)
    np.testing.assert_array_equal(idx, [[0, 1, 2, 3]])
    np.testing.assert_array_equal(d2, [[1.0, 1.0, 4.0, 4.0]])
    label, conf, proba = ctx.cross_vote(np.array([5, 5, 2, 2], dtype=np.int32), 6, "uniform", proba=True)
    assert label[0] == 2 and conf[0] == 0.5 and proba[0, 2] == proba[0, 5] == 0.5
    label, conf, proba = ctx.cross_vote(np.array([4, 1, 1, 4], dtype=np.int32), 5, "distance", proba=True)
    assert label[0] == 1 and conf[0] == 0.5 and proba[0, 1] == proba[0, 4] == 0.5


@pytest.mark.parametrize("weighting", ["uniform", "distance"])
@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("C, dtype", [(1, np.float64), (2, np.float32), (33, np.float64), (64, np.float64)])
def test_regress_equals_the_restatement(C, dtype, k, weighting):
    Q, R, idx, d2 = _gather_lists(k)
    Y = (np.random.default_rng(C).standard_normal((R.shape[0], C)) * 50.0).astype(dtype)
    ctx = _ctx()
    ctx.knn_cross(R, Q, k, fetch=False)
    out = ctx.cross_regress(Y, weighting)
    want = IR.regress(idx, d2, Y, weighting)
    assert out.dtype == np.float64 and out.tobytes() == want.tobytes()


# ---- sklearn on the device's output -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", ["uniform", "distance"])
def test_labels_probabilities_and_values_agree_with_sklearn(weighting):
    from sklearn.neighbors import KNeighborsClassifier, KNeighborsRegressor

    k, n_classes = 15, 9
    R, Q = NR.pca_like(3000, 50, 0), NR.pca_like(3000, 50, 7)
    rng = np.random.default_rng(4)
    # labels with structure, so that votes are not all near ties: the sign pattern of the two widest columns plus noise
    codes = ((R[:, 0] > 0).astype(np.int32) * 4 + (R[:, 1] > 0) * 2 + (rng.random(3000) < 0.15) * 1 + (rng.random(3000) < 0.05) * 1)
    codes = codes.astype(np.int32)
    Y = rng.standard_normal((3000, 2)) * 10.0
    assert IR.kth_gap(Q, R, k).min() > GAP                      # the condition under which sklearn finds the same neighbours
    idx, d2 = IR.cross_knn(Q, R, k)
    tol_p, tol_y = sklearn_bounds(Q, R, idx, d2, np.abs(Y).max(), weighting)
    want_label, _, want_proba = IR.vote(idx, d2, codes, n_classes, weighting)
    top = np.sort(want_proba, axis=1)
    if weighting == "distance":
        assert (top[:, -1] - top[:, -2]).min() > tol_p          # no vote within the tolerance of a tie
    else:
        assert tol_p == 0.0                                     # uniform: integer counts on both sides, ties to the lowest code on both

    ctx = _ctx()
    ctx.knn_cross(R, Q, k, fetch=False)
    label, conf, proba = ctx.cross_vote(codes, n_classes, weighting, proba=True)
    out = ctx.cross_regress(Y, weighting)
    clf = KNeighborsClassifier(n_neighbors=k, algorithm="brute", weights=weighting).fit(R, codes)
    sk_proba = np.zeros((3000, n_classes))
    sk_proba[:, clf.classes_] = clf.predict_proba(Q)
    sk_out = KNeighborsRegressor(n_neighbors=k, algorithm="brute", weights=weighting).fit(R, Y).predict(Q)
    print(f"{weighting}: max |proba - sklearn| = {np.abs(proba - sk_proba).max():.3e} (bound {tol_p:.3e}); "
          f"max |regress - sklearn| = {np.abs(out - sk_out).max():.3e} (bound {tol_y:.3e})")
    np.testing.assert_array_equal(label, clf.predict(Q))        # every label, no row left out
    assert np.abs(proba - sk_proba).max() <= tol_p
    assert np.abs(out - sk_out).max() <= tol_y


# ---- the public functions ------------------------------------------------------------------------------------------------------------------------
def _reference(n=900, seed=0):
    """Three well-separated blobs in 10 dimensions with a 2-D embedding that keeps them apart."""
    rng = np.random.default_rng(seed)
    blob = np.arange(n) % 3
    centres = np.zeros((3, 10))
    centres[0, 0], centres[1, 1], centres[2, 2] = 40.0, 40.0, 40.0
    X = centres[blob] + rng.standard_normal((n, 10))
    ad = make_adata(np.zeros((n, 2)), np.zeros((n, 2)))
    ad.obsm["X_pca"] = X
    ad.obsm["X_umap"] = (np.array([[0.0, 0.0], [100.0, 0.0], [0.0, 100.0]])[blob] + rng.standard_normal((n, 2))).astype(np.float32)
    ad.obs["blob"] = pd.Categorical(np.array(["a", "b", "c"])[blob], categories=["c", "unused", "a", "b"])
    ad.obs["number"] = blob * 10
    return ad, blob


def _subset(ad, rows):
    sub = make_adata(np.zeros((len(rows), 2)), np.zeros((len(rows), 2)))
    sub.obsm = {key: np.asarray(val)[rows] for key, val in ad.obsm.items() if key != "spatial"}
    sub.obs = ad.obs.iloc[rows].copy()
    return sub


def test_ingest_onto_itself_with_one_neighbour_returns_the_input():
    from spatialcore_amd.neighbors import ingest, query_neighbors

    ref, _ = _reference()
    ad = _subset(ref, np.arange(ref.n_obs))
    ad.obs = ad.obs[[]].copy()
    del ad.obsm["X_umap"]
    out = ingest(ad, ref, obs=["blob", "number"], obsm=["X_umap", "X_pca"], n_neighbors=1, store_proba=True)
    assert out is ad
    assert list(ad.obs["blob"].cat.categories) == ["c", "unused", "a", "b"]
    np.testing.assert_array_equal(ad.obs["blob"].astype(str).values, ref.obs["blob"].astype(str).values)
    np.testing.assert_array_equal(ad.obs["number"].astype(int).values, ref.obs["number"].values)
    np.testing.assert_array_equal(ad.obs["blob_confidence"].values, 1.0)
    assert ad.obsm["X_umap"].dtype == np.float64
    assert ad.obsm["X_umap"].tobytes() == ref.obsm["X_umap"].astype(np.float64).tobytes()
    np.testing.assert_array_equal(ad.obs["ingest_distance"].values, 0.0)
    assert ad.obsm["blob_proba"].shape == (ref.n_obs, 4) and np.all(ad.obsm["blob_proba"].sum(axis=1) == 1.0)
    assert ad.uns["ingest"]["n_ref"] == ref.n_obs and ad.uns["ingest"]["obs"] == ["blob", "number"]
    assert ad.uns["ingest"]["params"]["n_neighbors"] == 1 and "path" in ad.uns["ingest"]["search"]
    assert ad.uns["spatialcore_metadata"]["operations"][-1]["function"] == "ingest"
    idx, dist = query_neighbors(ad, ref, n_neighbors=1)
    np.testing.assert_array_equal(idx[:, 0], np.arange(ref.n_obs))
    assert idx.dtype == np.int32 and dist.dtype == np.float64 and not dist.any()


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_held_out_cells_get_their_blob(weights):
    from spatialcore_amd.neighbors import ingest, query_neighbors

    full, blob = _reference()
    held = np.arange(full.n_obs) % 3 == np.arange(full.n_obs) // 3 % 3          # a third of every blob
    ref, ad = _subset(full, np.flatnonzero(~held)), _subset(full, np.flatnonzero(held))
    truth = ad.obs["blob"].astype(str).values
    ad.obs = ad.obs[[]].copy()
    del ad.obsm["X_umap"]
    before = {key: val.copy() for key, val in ad.obsm.items()}
    out = ingest(ad, ref, obs="blob", obsm="X_umap", weights=weights, copy=True)
    assert out is not ad and list(ad.obs.columns) == [] and sorted(ad.obsm) == sorted(before) and "ingest" not in ad.uns
    assert (out.obs["blob"].astype(str).values == truth).mean() == 1.0
    assert list(out.obs["blob"].cat.categories) == ["c", "unused", "a", "b"]
    for b, name in enumerate("abc"):
        box = np.asarray(ref.obsm["X_umap"])[ref.obs["blob"].astype(str).values == name]
        got = out.obsm["X_umap"][truth == name]
        assert np.all(got >= box.min(axis=0)) and np.all(got <= box.max(axis=0))
    idx, dist = query_neighbors(ad, ref, n_neighbors=15)
    want_i, want_d = IR.cross_knn(ad.obsm["X_pca"], ref.obsm["X_pca"], 15)
    assert idx.tobytes() == want_i.tobytes() and dist.tobytes() == np.sqrt(want_d).tobytes()
    np.testing.assert_array_equal(out.obs["ingest_distance"].values, dist[:, 0])


def test_nothing_is_written_on_error():
    """After one good call: a refused second call (tests/test_cpu_ingest.py has every refusal) leaves the first one's
    results as they were."""
    from spatialcore_amd.neighbors import ingest

    ref, _ = _reference(90)
    ad = _subset(ref, np.arange(30))
    ad.obs = ad.obs[[]].copy()
    del ad.obsm["X_umap"]
    ingest(ad, ref, obs="blob", n_neighbors=3)
    state = (ad.obs.copy(), {key: np.array(val) for key, val in ad.obsm.items()}, dict(ad.uns["ingest"]),
             len(ad.uns["spatialcore_metadata"]["operations"]))
    ref.obs["score"] = np.linspace(0.0, 1.0, 90)
    for kwargs in (dict(obs=["number", "score"], obsm="X_umap"), dict(obs="number", obsm=["X_umap", "missing"]),
                   dict(obs="number", n_neighbors=91)):
        with pytest.raises(ValueError):
            ingest(ad, ref, **kwargs)
        assert ad.obs.equals(state[0]) and sorted(ad.obsm) == sorted(state[1]) and ad.uns["ingest"] == state[2]
        assert len(ad.uns["spatialcore_metadata"]["operations"]) == state[3]


_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import test_gpu_ingest as T
np.savez(sys.argv[1], **T._public_bytes())
"""


def _public_bytes():
    from spatialcore_amd.neighbors import ingest

    full, _ = _reference(600, 1)
    ref, ad = _subset(full, np.arange(400)), _subset(full, np.arange(400, 600))
    ad.obs = ad.obs[[]].copy()
    del ad.obsm["X_umap"]
    out = ingest(ad, ref, obs="blob", obsm="X_umap", weights="distance", store_proba=True, copy=True)
    R, Q = NR.pca_like(3000, 50, 0), NR.pca_like(700, 50, 7)
    idx, d2, _ = _ctx().knn_cross(R, Q, 15, path=2)
    return {"codes": np.asarray(out.obs["blob"].cat.codes), "conf": out.obs["blob_confidence"].values, "umap": out.obsm["X_umap"],
            "proba": out.obsm["blob_proba"], "dist": out.obs["ingest_distance"].values, "idx": idx, "d2": d2}


def test_two_calls_and_a_child_on_four_hardware_queues_give_the_same_bytes(tmp_path):
    first, again = _public_bytes(), _public_bytes()
    script = tmp_path / "ingest_child.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    run = subprocess.run([sys.executable, str(script), str(tmp_path / "child.npz")], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    child = np.load(tmp_path / "child.npz")
    for key, val in first.items():
        assert again[key].tobytes() == val.tobytes() and child[key].tobytes() == val.tobytes(), key
