"""sc_fuzzy_graph, sc_umap_layout, neighbors(method="umap") and spatialcore_amd.embedding.umap on the device, against the
numpy restatement (tests/umap_restated.py), whose recipes and their properties are checked on the host in
tests/test_cpu_umap.py.

What is exact is compared byte for byte: rho (a sqrt of a pinned d2), the union's pattern, the symmetry of the weights,
and every statement about one layout run against another.  sigma, the weights and the positions go through exp, pow and
divisions of their results, where the device's and numpy's functions differ in the last place.  MEASURED_* are the largest
differences over all the inputs of this file as scripts/umap_probe.py --tolerances measured them on an MI355X
(profiles/umap_1m.json, "tolerances"); the tests assert ten times those figures and never more than 1e-9, the cap the
project uses for pca against sklearn.

Quality: the restatement on the CPU takes the ten-blob recipe (n = 1500, k = 15, 200 epochs, default a and b, 2-D PCA
start scaled to 10) from trustworthiness 0.7989 to 0.9757 (sklearn, 15 neighbours) and from 1-NN label accuracy 0.619 to
1.000, extent 14.2; the thresholds below come from those figures and from the start, never from the device's output."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import sparse

import diffusion_restated as R
import umap_restated as U
from conftest import ROOT, make_adata

pytestmark = pytest.mark.gpu

CAP = 1e-9
MEASURED_SIGMA = 0.0            # every sigma came out bit-equal: the bisection's branches agree and its values are dyadic
MEASURED_W = 4.29e-16           # (traj-n1000-d20-k15)
MEASURED_LAYOUT = 1.69e-15      # of the extent 10 (n257-C2-coincident)
TOL_SIGMA, TOL_W, TOL_LAYOUT = (min(10 * m, CAP) for m in (MEASURED_SIGMA, MEASURED_W, MEASURED_LAYOUT))
NORMAL = 1e-300                 # below this a double has lost bits and a relative difference says nothing

RESTATED_TRUST_START, RESTATED_TRUST_END = 0.7989, 0.9757


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


@functools.lru_cache(maxsize=None)
def _fuzzy_truth(name):
    X, k = U.fuzzy_recipes()[name]
    idx, d2 = R.knn(X, k)
    return X, k, idx, d2, U.fuzzy_graph(idx, d2)


def _rel(got, ref):
    """Largest relative difference over the normal-range entries; the others must be tiny on both sides."""
    big = ref >= NORMAL
    assert np.all(got[~big] < 10 * NORMAL)
    return float(np.max(np.abs(got[big] - ref[big]) / ref[big])) if big.any() else 0.0


# ---- 1. the fuzzy graph ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.fuzzy_recipes()))
def test_fuzzy_graph_equals_the_restatement(name):
    X, k, idx, d2, g = _fuzzy_truth(name)
    n = X.shape[0]
    ctx = _ctx()
    got_idx, got_d2 = ctx.knn_dense(X, k)
    assert np.array_equal(got_idx, idx) and got_d2.tobytes() == d2.tobytes()
    info = ctx.fuzzy_graph()
    indptr, indices, w, T = ctx.diffmap_graph_get(transition=True)
    assert info["n_edges"] == indices.size == g["indices"].size
    assert indptr.dtype == np.int64 and indices.dtype == np.int32
    assert indptr.tobytes() == g["indptr"].tobytes() and indices.tobytes() == g["indices"].tobytes()
    assert info["rho"].tobytes() == g["rho"].tobytes()
    rel_sigma, rel_w = _rel(info["sigma"], g["sigma"]), _rel(w, g["w"])
    print(f"{name}: max relative difference sigma {rel_sigma:.3e}, w {rel_w:.3e}")
    assert rel_sigma <= TOL_SIGMA and rel_w <= TOL_W
    A = sparse.csr_matrix((w, indices, indptr), shape=(n, n))
    At = A.T.tocsr()
    At.sort_indices()
    assert np.array_equal(At.indices, indices) and At.data.tobytes() == w.tobytes()          # bit-symmetric
    assert info["n_components"] == R.n_components(indptr, indices)
    assert np.all(np.isfinite(T)) and np.all(T >= 0)                  # the tail ran: Lanczos and Louvain may follow
    if name.startswith(("traj", "scaled")):                           # the duplicates have no Gaussian kernel matrix
        ctx.knn_dense(X, k, fetch=False)
        ctx.diffmap_graph()
        ref = ctx.diffmap_graph_get()
        assert ref[0].tobytes() == indptr.tobytes() and ref[1].tobytes() == indices.tobytes()


def test_fuzzy_graph_twice_and_after_the_gram_search_gives_the_same_bytes():
    X, k = U.features(1000, 20), 15
    ctx = _ctx()
    ctx.knn_dense(X, k, fetch=False)
    a = ctx.fuzzy_graph()
    ga = ctx.diffmap_graph_get(transition=True)
    ctx.knn_dense_gram(X, k, fetch=False, path=2)
    b = ctx.fuzzy_graph()
    gb = ctx.diffmap_graph_get(transition=True)
    assert a["rho"].tobytes() == b["rho"].tobytes() and a["sigma"].tobytes() == b["sigma"].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ga, gb))


def test_fuzzy_graph_needs_resident_lists():
    from spatialcore_amd import _lib

    ctx = _lib.Context(0)
    with pytest.raises(Exception, match="no neighbour lists are resident"):
        ctx.fuzzy_graph()


def _adata(X, key="X_pca"):
    ad = make_adata(np.zeros((X.shape[0], 2)), np.zeros((X.shape[0], 1)))
    ad.obsm[key] = X
    return ad


def test_neighbors_default_is_gauss_byte_for_byte_and_umap_is_the_fuzzy_graph():
    from spatialcore_amd.cluster import louvain
    from spatialcore_amd.neighbors import neighbors

    X, k, idx, d2, g = _fuzzy_truth("traj-n1000-d20-k15")
    default, gauss, fuzzy = neighbors(_adata(X), k), neighbors(_adata(X), k, method="gauss"), neighbors(_adata(X), k, method="umap")
    for key in ("distances", "connectivities"):
        a, b = default.obsp[key], gauss.obsp[key]
        assert a.indptr.tobytes() == b.indptr.tobytes() and a.indices.tobytes() == b.indices.tobytes()
        assert a.data.tobytes() == b.data.tobytes()
    assert default.uns["neighbors"] == gauss.uns["neighbors"] and default.uns["neighbors"]["params"]["method"] == "gauss"
    ref = R.graph(X, k)
    assert np.max(np.abs(default.obsp["connectivities"].data - ref["w"]) / ref["w"]) <= 1e-13

    assert fuzzy.uns["neighbors"]["params"] == {"n_neighbors": k, "method": "umap", "metric": "euclidean", "use_rep": "X_pca",
                                                "n_features": 20}
    assert set(fuzzy.uns["neighbors"]) == {"connectivities_key", "distances_key", "params", "search"}
    assert fuzzy.obsp["distances"].data.tobytes() == default.obsp["distances"].data.tobytes()
    C = fuzzy.obsp["connectivities"]
    assert sparse.isspmatrix_csr(C) and C.dtype == np.float64 and C.shape == (1000, 1000)
    assert np.array_equal(C.indptr, g["indptr"]) and np.array_equal(C.indices, g["indices"])
    assert _rel(C.data, g["w"]) <= TOL_W
    assert (C != C.T).nnz == 0
    assert fuzzy.uns["spatialcore_metadata"]["operations"][-1]["parameters"]["method"] == "umap"
    louvain(fuzzy, graph="connectivities")                             # its symmetry check takes the matrix unchanged
    assert 2 <= len(fuzzy.obs["louvain"].cat.categories) < 200


# ---- 2. the layout against the restatement -------------------------------------------------------------------------------
SEED = 11


@functools.lru_cache(maxsize=None)
def _recipes():
    return U.layout_recipes()


@pytest.mark.parametrize("name", list(U.layout_recipes()))
def test_layout_epochs_equal_the_restatement(name):
    graph, Y0, neg = _recipes()[name]
    ctx = _ctx()
    ref = Y0
    for e1 in (1, 2, 3):
        ref = U.layout(*graph, ref, 10, e1 - 1, e1, neg=neg, seed=SEED)
        got = ctx.umap_layout(graph, Y0, U.A_DEFAULT, U.B_DEFAULT, 1.0, 1.0, neg, 10, SEED, 0, e1)
        assert got.dtype == np.float64 and got.shape == Y0.shape
        diff = float(np.max(np.abs(got - ref))) / 10.0
        print(f"{name}: epochs [0, {e1}): max |Y - restated| / 10 = {diff:.3e}")
        assert diff <= TOL_LAYOUT
    assert not np.array_equal(got, Y0)


def test_layout_moves_by_the_documented_step_on_two_vertices():
    """One edge, no negatives, one epoch: both ends move towards each other by alpha clip(c_att dlt)."""
    graph = (np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32), np.array([0.7, 0.7]))
    Y0 = np.array([[0.0, 0.0], [3.0, 0.25]])
    a, b = U.A_DEFAULT, U.B_DEFAULT
    got = _ctx().umap_layout(graph, Y0, a, b, 1.0, 0.5, 0, 4, 0, 0, 1)
    d2 = 3.0 * 3.0 + 0.25 * 0.25
    coef = (((-2.0 * a) * b) * (d2 ** b / d2)) / (a * d2 ** b + 1.0)
    step = 0.5 * np.clip(coef * (Y0[0] - Y0[1]), -4.0, 4.0)
    assert np.allclose(got[0], Y0[0] + step, rtol=1e-12, atol=1e-14)
    assert np.array_equal(got[0] - Y0[0], -(got[1] - Y0[1]))


# ---- 3. exactness, byte for byte -----------------------------------------------------------------------------------------
def _run(name="n257-C2", e0=0, e1=10, Y=None):
    g, Y0, neg = _recipes()[name]
    return _ctx().umap_layout(g, Y0 if Y is None else Y, U.A_DEFAULT, U.B_DEFAULT, 1.0, 1.0, neg, 10, SEED, e0, e1)


@pytest.mark.parametrize("name", ["n257-C3", "star-C2"])
def test_split_epoch_ranges_and_repeated_runs_give_the_same_bytes(name):
    whole = _run(name)
    assert _run(name).tobytes() == whole.tobytes()
    assert _run(name, 4, 10, Y=_run(name, 0, 4)).tobytes() == whole.tobytes()
    assert _run(name, 3, 3).tobytes() == _recipes()[name][1].tobytes()             # an empty range returns the start


def test_resident_graph_and_uploaded_graph_give_the_same_bytes():
    X, k = U.features(257, 8), 15
    ctx = _ctx()
    ctx.knn_dense(X, k, fetch=False)
    ctx.fuzzy_graph()
    graph = ctx.diffmap_graph_get()
    Y0 = U.start(257, 2, 4)
    resident = ctx.umap_layout(None, Y0, U.A_DEFAULT, U.B_DEFAULT, 1.0, 1.0, 5, 10, SEED)
    uploaded = ctx.umap_layout(graph, Y0, U.A_DEFAULT, U.B_DEFAULT, 1.0, 1.0, 5, 10, SEED)
    assert resident.tobytes() == uploaded.tobytes()


_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {oracle!r}); sys.path.insert(0, {tests!r})
import test_gpu_umap as T
open(sys.argv[1], "wb").write(T._run("n257-C2").tobytes() + T._run("star-C2").tobytes())
"""


def test_the_bytes_do_not_depend_on_the_hardware_queues(tmp_path):
    """Fresh children held to GPU_MAX_HW_QUEUES=4 and 24 compute the bytes this process computes."""
    script = tmp_path / "umap_child.py"
    script.write_text(_CHILD.format(root=ROOT, oracle=os.path.join(ROOT, "oracle"), tests=os.path.join(ROOT, "tests")))
    here = _run("n257-C2").tobytes() + _run("star-C2").tobytes()
    for queues in ("4", "24"):
        out = tmp_path / f"child{queues}.bin"
        run = subprocess.run([sys.executable, str(script), str(out)], env=dict(os.environ, GPU_MAX_HW_QUEUES=queues),
                             capture_output=True, text=True, timeout=240)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
        assert open(out, "rb").read() == here, queues


def test_layout_refusals_come_from_the_host():
    graph, Y0, _ = _recipes()["n17-C2"]
    ctx = _ctx()
    ok = dict(a=1.0, b=1.0, gamma=1.0, alpha0=1.0, neg=5, n_epochs=10, seed=0)
    for change, match in ((dict(neg=17), "neg"), (dict(n_epochs=0), "n_epochs"), (dict(a=0.0), "a and b"), (dict(e0=4, e1=3), "epoch range"),
                          (dict(e1=11), "epoch range"), (dict(gamma=-1.0), "gamma"), (dict(alpha0=float("nan")), "alpha0")):
        with pytest.raises(ValueError, match=match):
            ctx.umap_layout(graph, Y0, **{**ok, **change})
    with pytest.raises(ValueError, match="2 or 3 components"):
        ctx.umap_layout(graph, np.zeros((17, 4)), **ok)
    bad = (graph[0], graph[1][::-1].copy(), graph[2])
    with pytest.raises(ValueError, match="not canonical"):
        ctx.umap_layout(bad, Y0, **ok)
    with pytest.raises(ValueError, match="finite and > 0"):
        ctx.umap_layout((graph[0], graph[1], np.zeros_like(graph[2])), Y0, **ok)
    Y = Y0.copy()
    Y[3, 1] = np.nan
    with pytest.raises(ValueError, match="position value 7 is not finite"):
        ctx.umap_layout(graph, Y, **ok)


# ---- 4. quality ----------------------------------------------------------------------------------------------------------------
def test_ten_blobs_separate():
    from sklearn.manifold import trustworthiness

    from spatialcore_amd.embedding import umap
    from spatialcore_amd.neighbors import neighbors

    X, labels = U.blobs()
    ad = _adata(X, key="X")
    ad.obsm["X_pca"] = U.pca2(X)
    neighbors(ad, 15, use_rep="X", method="umap")
    umap(ad, n_epochs=200, a=U.A_DEFAULT, b=U.B_DEFAULT)
    Y = ad.obsm["X_umap"]
    start = trustworthiness(X, ad.obsm["X_pca"], n_neighbors=15)
    trust, acc, extent = trustworthiness(X, Y, n_neighbors=15), U.one_nn_accuracy(Y, labels), float(np.abs(Y).max())
    print(f"trustworthiness {start:.4f} -> {trust:.4f}, 1-NN accuracy {acc:.4f}, extent {extent:.2f}")
    assert abs(start - RESTATED_TRUST_START) < 1e-3
    assert trust >= start + 0.5 * (RESTATED_TRUST_END - RESTATED_TRUST_START)
    assert acc >= 0.99
    assert extent < 100.0


# ---- 5. the public call ------------------------------------------------------------------------------------------------------
def test_pca_neighbors_umap():
    from spatialcore_amd.embedding import umap
    from spatialcore_amd.neighbors import neighbors

    n = 600
    X = U.features(n, 12)
    ad = _adata(X)
    neighbors(ad, 10, method="umap")
    before = {k: v.copy() for k, v in ad.obsm.items()}
    out = umap(ad, n_epochs=30, copy=True)
    assert out is not ad and set(ad.obsm) == set(before) and "umap" not in ad.uns
    assert ad.uns["spatialcore_metadata"]["operations"][-1]["function"] == "neighbors"
    Y = out.obsm["X_umap"]
    assert Y.dtype == np.float64 and Y.shape == (n, 2) and np.all(np.isfinite(Y))
    p = out.uns["umap"]["params"]
    assert set(p) == {"a", "b", "min_dist", "spread", "n_epochs", "alpha", "gamma", "negative_sample_rate", "seed", "init_pos",
                      "n_components", "neighbors_key"}
    assert abs(p["a"] - 0.58303) < 1e-4 and abs(p["b"] - 1.33417) < 1e-4 and p["n_epochs"] == 30 and p["init_pos"] == "X_pca"
    assert p["n_components"] == 2 and p["neighbors_key"] is None and p["negative_sample_rate"] == 5 and p["seed"] == 0
    op = out.uns["spatialcore_metadata"]["operations"][-1]
    assert op["function"] == "umap" and op["outputs"] == {"obsm": "X_umap", "uns": "umap"}

    assert umap(ad, n_epochs=30) is ad
    assert ad.obsm["X_umap"].tobytes() == Y.tobytes()                     # a second call, the same bytes
    assert umap(ad, n_epochs=None, copy=True).uns["umap"]["params"]["n_epochs"] == 500

    # the restatement on the stored graph, from the documented start, for the first epochs
    C = ad.obsp["connectivities"]
    Y0 = X[:, :2] * (10.0 / np.abs(X[:, :2]).max())
    three = umap(ad, n_epochs=30, copy=True, key_added="three")          # key_added routing
    assert "three" in three.obsm and three.uns["three"]["params"]["n_epochs"] == 30 and "X_umap" in three.obsm
    ref = U.layout(C.indptr.astype(np.int64), C.indices, C.data, Y0, 30, 0, 2, a=p["a"], b=p["b"], seed=0)
    got = _ctx().umap_layout((C.indptr, C.indices, C.data), Y0, p["a"], p["b"], 1.0, 1.0, 5, 30, 0, 0, 2)
    assert np.max(np.abs(got - ref)) / 10.0 <= TOL_LAYOUT

    # neighbors_key and graph= routing, 3 components from a random start
    neighbors(ad, 6, key_added="coarse")
    by_key = umap(ad, neighbors_key="coarse", n_epochs=20, n_components=3, init_pos="random", seed=3, copy=True)
    by_graph = umap(ad, graph="coarse_connectivities", n_epochs=20, n_components=3, init_pos="random", seed=3, copy=True)
    by_matrix = umap(ad, graph=ad.obsp["coarse_connectivities"], n_epochs=20, n_components=3, init_pos="random", seed=3, copy=True)
    assert by_key.obsm["X_umap"].shape == (n, 3) and by_key.uns["umap"]["params"]["neighbors_key"] == "coarse"
    assert by_key.obsm["X_umap"].tobytes() == by_graph.obsm["X_umap"].tobytes() == by_matrix.obsm["X_umap"].tobytes()
    assert by_key.obsm["X_umap"].tobytes() != umap(ad, n_epochs=20, n_components=3, init_pos="random", seed=3,
                                                   copy=True).obsm["X_umap"].tobytes()
