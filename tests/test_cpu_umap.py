"""Host side of spatialcore_amd.embedding.umap and neighbors(method="umap"): the recipes of tests/test_gpu_umap.py have the
properties those tests rely on (counted by the numpy restatement, tests/umap_restated.py), the curve fit gives scanpy's
published a and b, every bad argument is refused before a device is touched, and the restated fuzzy graph is a fuzzy graph."""
import functools

import numpy as np
import pytest
from scipy import sparse

import diffusion_restated as R
import umap_restated as U
from conftest import make_adata


@functools.lru_cache(maxsize=None)
def _fuzzy(name):
    X, k = U.fuzzy_recipes()[name]
    idx, d2 = R.knn(X, k)
    return idx, d2, U.fuzzy_graph(idx, d2)


FAST = [name for name in U.fuzzy_recipes() if name != "copies-40"]      # the 4,000-cell search runs once, below


# ---- the fuzzy graph's recipes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAST)
def test_restated_fuzzy_graph_is_symmetric_and_meets_the_target(name):
    idx, d2, g = _fuzzy(name)
    n, k = idx.shape
    A = sparse.csr_matrix((g["w"], g["indices"], g["indptr"]), shape=(n, n))
    T = A.T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indptr, A.indptr) and np.array_equal(T.indices, A.indices)
    assert T.data.tobytes() == A.data.tobytes()                       # bit-symmetric
    assert np.all(g["w"] >= 0) and np.all(g["w"] <= 1) and g["w"].max() == 1.0
    info = g["info"]
    ok = info["converged"] & ~info["floored"]
    assert np.all(np.abs(g["p"][ok].sum(axis=1) - np.log2(k + 1)) < 1e-5)
    assert np.all(g["rho"] <= np.sqrt(d2[:, -1]))
    assert np.all(g["sigma"] > 0)


def test_the_shapes_converge_and_the_scaled_ones_take_the_doubling_branch():
    for n, d, k in U.FUZZY_SHAPES:
        info = _fuzzy(f"traj-n{n}-d{d}-k{k}")[2]["info"]
        assert info["converged"].all() and not info["floored"].any()
    big, small = _fuzzy("scaled-1e3")[2], _fuzzy("scaled-1e-3")[2]
    assert big["sigma"].min() > 2.0          # mid left 1 upwards: only the doubling while hi = inf gets there
    assert small["sigma"].max() < 1e-3 and small["info"]["converged"].all()


def test_duplicate_recipes_reach_rho_the_iteration_limit_and_the_floors():
    idx, d2, two = _fuzzy("copies-2")
    assert np.all(d2[:, 0] == 0) and np.all(d2[:, 1] > 0)
    assert np.array_equal(two["rho"], np.sqrt(d2[:, 1]))               # the first NON-ZERO distance
    assert two["info"]["converged"].all()
    _, d2, six = _fuzzy("copies-6")
    assert np.all(d2[:, 4] == 0) and np.all(d2[:, 5] > 0)
    assert np.all(six["info"]["iterations"] == U.ITERS) and not six["info"]["converged"].any()   # five ones > log2(16)
    assert six["info"]["floored"].all() and np.all(six["rho"] > 0)     # the row-mean floor
    assert np.array_equal(six["sigma"], 1e-3 * (six["info"]["row_sums"] / 16.0))
    _, d2, forty = _fuzzy("copies-40")
    assert np.all(d2 == 0) and np.all(forty["rho"] == 0) and forty["info"]["global_mean"] == 0.0
    assert np.all(forty["info"]["iterations"] == U.ITERS)
    assert np.all(forty["sigma"] == 2.0 ** -64) and np.all(forty["p"] == 1.0) and np.all(forty["w"] == 1.0)


# ---- the layout's recipes --------------------------------------------------------------------------------------------
def test_layout_recipes_clip_skip_coincide_and_hold_entries_that_never_fire():
    recipes = U.layout_recipes()
    stats = {}
    for name, (graph, Y, neg) in recipes.items():
        stats[name] = U.new_stats()
        out = U.layout(*graph, Y, 10, 0, 3, neg=neg, seed=11, stats=stats[name])
        assert np.all(np.isfinite(out)) and out.shape == Y.shape
        print(name, stats[name])
    assert stats["n3-C2"]["skipped"] >= 10                         # a third of the draws on three vertices
    assert stats["n257-C2"]["clipped"] >= 1 and stats["n257-C2"]["skipped"] >= 1
    assert stats["star-C2"]["clipped"] >= 1
    assert stats["n257-C2-neg0"]["skipped"] == 0
    assert stats["n257-C2-coincident"]["coincident"] >= 1 and stats["n257-C2"]["coincident"] == 0
    indptr, _, w = recipes["star-C2"][0]
    assert np.diff(indptr).max() == 299 and np.sum(np.diff(indptr) == 2) >= 290
    assert w.min() < w.max() / 10 and U.never_fires(w, 10).any()
    assert U.never_fires(recipes["n257-C2"][0][2], 10).any()


def test_layout_recipes_are_well_conditioned():
    """Three restated epochs move by less than 1e-12 of the extent under a one-ulp change of every pow: a difference to the
    device beyond that is the device's."""
    for name, (graph, Y, neg) in U.layout_recipes().items():
        moved = U.conditioning(graph, Y, neg)
        print(name, moved)
        assert moved < 1e-12, name


def test_firing_counts_follow_the_weights():
    """Over n_epochs epochs entry t fires floor(n_epochs r_t) times: umap's epochs_per_sample schedule."""
    w = np.array([1.0, 0.5, 0.26, 0.1, 0.0999, 0.37])
    count = sum(U.firing(w, e).astype(int) for e in range(10))
    assert count.tolist() == [10, 5, 2, 1, 0, 3]


def test_negatives_are_philox_words_scaled_to_n(oracle):
    t, e, n, seed = np.array([0, 5, 2**33 + 7]), 3, 1000, (9 << 32) | 4
    for q in (0, 3, 4, 15):
        got = U.negatives(t, e, q, n, seed)
        for p, tt in enumerate(t):
            o = oracle.philox4x32_10(np.array([int(tt) & 0xFFFFFFFF, int(tt) >> 32, e, q >> 2], dtype=np.uint32), (4, 9))
            assert got[p] == (int(o[q & 3]) * n) >> 32


# ---- the public calls --------------------------------------------------------------------------------------------------
def test_default_a_and_b_are_scanpys():
    from spatialcore_amd.embedding.layout import default_epochs, find_ab_params

    a, b = find_ab_params(1.0, 0.5)
    assert abs(a - 0.58303) < 1e-4 and abs(b - 1.33417) < 1e-4
    assert abs(a - U.A_DEFAULT) < 1e-4 and abs(b - U.B_DEFAULT) < 1e-4
    assert default_epochs(10000) == 500 and default_epochs(10001) == 200


def _adata(n=30):
    X = U.features(n, 4)
    ad = make_adata(np.zeros((n, 2)), np.zeros((n, 1)))
    ad.obsm["X_pca"] = X
    g = U.fuzzy_graph(*R.knn(X, 5))
    ad.obsp["connectivities"] = sparse.csr_matrix((np.maximum(g["w"], 1e-300), g["indices"], g["indptr"]), shape=(n, n))
    ad.uns["neighbors"] = {"connectivities_key": "connectivities"}
    return ad


BAD = [
    (dict(min_dist=-0.1), "min_dist"), (dict(min_dist=3.0), "min_dist"), (dict(spread=0.0), "spread"),
    (dict(spread=float("nan")), "spread"), (dict(n_components=4), "n_components"), (dict(n_components=2.0), "n_components"),
    (dict(n_epochs=0), "n_epochs"), (dict(n_epochs=1.5), "n_epochs"), (dict(alpha=0.0), "alpha"), (dict(gamma=-1.0), "gamma"),
    (dict(negative_sample_rate=17), "negative_sample_rate"), (dict(negative_sample_rate=-1), "negative_sample_rate"),
    (dict(seed=-1), "seed"), (dict(seed=2**64), "seed"), (dict(a=1.0), "a and b"), (dict(a=1.0, b=0.0), "a and b"),
    (dict(key_added=""), "key_added"), (dict(neighbors_key=3), "neighbors_key"), (dict(copy=1), "copy"),
    (dict(init_pos="X_missing"), "init_pos"), (dict(init_pos=np.zeros((30, 3))), "columns"),
    (dict(init_pos=np.zeros((29, 2))), "init_pos"), (dict(init_pos=np.full((30, 2), np.inf)), "NaN or infinite"),
    (dict(n_components=3, init_pos="X_two"), "columns"), (dict(graph="nothing"), "obsp"),
    (dict(graph=np.eye(30)), "sparse"), (dict(graph=sparse.eye(29, format="csr")), "30 x 30"),
]


@pytest.mark.parametrize("kw, match", BAD, ids=[f"{i}-{m.split()[0]}" for i, (_, m) in enumerate(BAD)])
def test_umap_refuses_bad_arguments_before_any_device_call(kw, match):
    from spatialcore_amd.embedding import umap

    ad = _adata()
    ad.obsm["X_two"] = ad.obsm["X_pca"][:, :2]
    with pytest.raises(ValueError, match=match):
        umap(ad, **kw)
    assert "X_umap" not in ad.obsm and "umap" not in ad.uns


def test_umap_refuses_an_asymmetric_graph_and_a_missing_one():
    from spatialcore_amd.embedding import umap

    ad = _adata()
    lop = ad.obsp["connectivities"].tolil()
    lop[0, int(ad.obsp["connectivities"].indices[0])] = 0.123
    with pytest.raises(ValueError, match="symmetric"):
        umap(ad, graph=lop.tocsr())
    del ad.uns["neighbors"]
    with pytest.raises(KeyError, match="neighbors"):
        umap(ad)
    with pytest.raises(KeyError, match="neighbors"):
        umap(ad, neighbors_key="other")
    ad.uns["neighbors"] = {"connectivities_key": "gone"}
    with pytest.raises(KeyError, match="neighbors"):
        umap(ad)


def test_neighbors_refuses_an_unknown_method_before_any_device_call():
    from spatialcore_amd.neighbors import neighbors

    ad = _adata()
    before = set(ad.obsp)
    for method in ("UMAP", "rapids", None, 1):
        with pytest.raises(ValueError, match=r"method must be one of \('gauss', 'umap'\)"):
            neighbors(ad, n_neighbors=5, method=method)
    assert set(ad.obsp) == before


def test_start_positions():
    from spatialcore_amd.embedding.layout import _start

    ad = _adata()
    Y, name = _start(ad, "X_pca", 30, 2, 0)
    assert name == "X_pca" and Y.dtype == np.float64 and Y.shape == (30, 2) and Y.flags.c_contiguous
    assert np.abs(Y).max() == pytest.approx(10.0, rel=1e-15)
    assert np.allclose(Y, ad.obsm["X_pca"][:, :2] * (10.0 / np.abs(ad.obsm["X_pca"][:, :2]).max()), rtol=1e-15)   # no noise
    Y, name = _start(ad, "random", 30, 3, 5)
    assert name == "random" and np.array_equal(Y, np.random.default_rng(5).uniform(-10, 10, size=(30, 3)))
    given = np.arange(60.0).reshape(30, 2)
    Y, name = _start(ad, given, 30, 2, 0)
    assert name == "<array>" and np.array_equal(Y, given) and Y is not given
