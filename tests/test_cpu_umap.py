"""Host side of spatialcore_amd.embedding.umap and neighbors(method="umap"): the recipes of tests/test_gpu_umap.py and
tests/test_gpu_umap_edges.py have the properties those tests rely on (counted by the numpy restatement, tests/umap_restated.py), the curve fit gives scanpy's
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


# ---- the recipes at the kernels' constants (tests/test_gpu_umap_edges.py) -----------------------------------------------
@pytest.mark.parametrize("n, k", U.MIXED_CASES)
def test_mixed_recipes_floor_the_copies_at_a_global_mean_that_sees_the_order(n, k):
    """k + 2 identical cells among ordinary ones: the only rows with rho = 0, floored at 1e-3 of a global mean that is not
    zero and whose chunked order (sc_chunk_sum.h) gives other bits than the rows added one after another."""
    X, copies = U.mixed(n, k)
    assert X.shape == (n, 8) and copies.size == k + 2 and np.all(X[copies] == X[0])
    idx, d2 = R.knn(X, k)
    rho, sigma, info = U.smooth_knn(d2)
    assert -(-n // R.CHUNK) == {1023: 1, 1024: 1, 1025: 2, 2049: 3}[n]           # the partial sums k_um_mean adds
    zero = np.flatnonzero(rho == 0)
    assert zero.size == k + 2 and np.array_equal(zero, copies)
    assert np.all(d2[copies] == 0)
    mean = info["global_mean"]
    print(f"mixed({n}, {k}): global mean {mean!r}, plain order {U.plain_mean(info['row_sums'], k)!r}")
    assert mean > 0 and 6.5 < mean < 8.6
    assert sigma[copies].tobytes() == np.full(k + 2, 1e-3 * mean).tobytes()
    assert U.plain_mean(info["row_sums"], k) != mean                              # what makes the case see the order
    # The cells whose nearest cell is the copied one list k copies at one distance d > 0: rho = d, every t = 0, psum = k >
    # log2(k + 1), the row-mean floor.  They and the copies are the floored rows; every other row converges unfloored.
    tied = np.flatnonzero((d2[:, 0] > 0) & (d2[:, 0] == d2[:, -1]))
    assert 1 <= tied.size <= 4 and np.all(np.isin(idx[tied], copies))
    assert np.array_equal(np.flatnonzero(info["floored"]), np.union1d(copies, tied))
    assert np.array_equal(np.flatnonzero(info["floored"] & (rho == 0)), copies)   # the global-mean floor: the copies alone
    assert np.array_equal(np.flatnonzero(~info["converged"]), np.union1d(copies, tied))
    assert np.array_equal(sigma[tied], 1e-3 * (info["row_sums"][tied] / float(k + 1)))
    assert n - copies.size - tied.size >= 1000                                    # ordinary rows through k_um_sigma<K>


@pytest.mark.parametrize("k", U.WIDTH_KS)
def test_width_recipes_converge_unfloored(k):
    assert {8, 9, 17, 31} < set(U.WIDTH_KS) and min(U.WIDTH_KS) == 2              # sc_knn_dense refuses k = 1
    _, d2 = R.knn(U.features(129, 8), k)
    info = U.smooth_knn(d2)[2]
    assert info["converged"].all() and not info["floored"].any()
    assert set(U.fuzzy_edge_recipes()) == {f"mixed-n{n}-k{kk}" for n, kk in U.MIXED_CASES} | {f"width-k{kk}" for kk in U.WIDTH_KS}


@functools.lru_cache(maxsize=None)
def _edge_cases():
    return U.layout_edge_recipes()


@functools.lru_cache(maxsize=None)
def _edge_run(name):
    """(restated positions after the case's last epoch, its statistics)"""
    stats = U.new_stats()
    return U.layout_case_epochs(_edge_cases()[name], stats=stats)[-1][1], stats


def test_edge_layout_recipes_are_the_listed_cases():
    cases = _edge_cases()
    assert set(cases) == ({f"neg{q}-C2" for q in (1, 3, 4, 8, 9, 16)} | {"neg4-C3", "neg16-C3", "seed-high-word", "ring-wmax-tail",
                          "star-empty-rows", "gamma0", "gamma0-neg0", "a1.5-b0.9", "late-epochs"})
    for name, case in cases.items():
        run = case["run"]
        assert case["Y0"].shape[1] == (3 if name.endswith("C3") else 2)
        assert (run["n_epochs"], run["e0"], run["e1"]) == {"ring-wmax-tail": (4, 0, 2), "late-epochs": (
            2 ** 31 - 1, 10 ** 9, 10 ** 9 + 3)}.get(name, (10, 0, 3))
        assert case["extent"] == (100.0 if name == "ring-wmax-tail" else 10.0)
        assert np.abs(case["Y0"]).max() <= case["extent"]


@pytest.mark.parametrize("name", [f"neg{q}-C2" for q in (1, 3, 4, 8, 9, 16)] + ["neg4-C3", "neg16-C3"])
def test_sample_block_recipes_skip_and_clip(name):
    case = _edge_cases()[name]
    neg = case["run"]["neg"]
    assert neg == int(name[3:].split("-")[0]) and case["run"]["seed"] == 11
    _, stats = _edge_run(name)
    print(name, stats)
    assert stats["skipped"] >= 1 and stats["clipped"] >= 1 and stats["coincident"] == 0


def test_high_seed_word_changes_the_restated_layout():
    graph, Y0, neg = U.layout_recipes()["n257-C2"]
    case = _edge_cases()["seed-high-word"]
    assert case["run"]["seed"] >> 32 == 5 and case["run"]["seed"] & 0xFFFFFFFF == 11 and case["run"]["neg"] == neg
    assert case["Y0"].tobytes() == Y0.tobytes()
    low = U.layout(*graph, Y0, 10, 0, 3, neg=neg, seed=11)
    assert not np.array_equal(_edge_run("seed-high-word")[0], low)


def test_ring_holds_its_largest_weight_past_the_strided_grid():
    (indptr, indices, w), top = U.ring()
    assert indptr[-1] == w.size == 560_000 and top.tolist() == [559_971, 559_999]
    assert np.all(top >= U.WMAX_GRID) and U.WMAX_GRID == 524_288
    rows = np.repeat(np.arange(20000), 28)
    assert sorted(zip(rows[top].tolist(), indices[top].tolist())) == [(19998, 19999), (19999, 19998)]
    assert np.all(np.diff(indices.reshape(20000, 28), axis=1) > 0)                       # canonical
    A = sparse.csr_matrix((w, indices, indptr), shape=(20000, 20000))
    At = A.T.tocsr()
    At.sort_indices()
    assert np.array_equal(At.indices, indices) and At.data.tobytes() == w.tobytes()       # symmetric
    head = float(w[:U.WMAX_GRID].max())
    assert head <= 0.55 < w[U.WMAX_GRID:].max() == w.max() == 1.0 and w.min() >= 0.05
    case = _edge_cases()["ring-wmax-tail"]
    assert case["run"]["neg"] == 5 and case["graph"][2].tobytes() == w.tobytes()
    true, stats = _edge_run("ring-wmax-tail")
    assert stats["firings"] > 50_000
    wrong = U.layout_case_epochs(case, w_max=head)[-1][1]                                # w_max of the unstrided part only
    assert np.all(np.abs(wrong - true).max(axis=1) > 1e-6)                               # moves every vertex


def test_empty_rows_keep_their_start_in_the_restatement():
    case = _edge_cases()["star-empty-rows"]
    indptr, indices, w = case["graph"]
    deg = np.diff(indptr)
    assert deg.size == 302 and np.flatnonzero(deg == 0).tolist() == [0, 301] and deg[1] == 299
    assert indices.min() == 1 and indices.max() == 300 and w.tobytes() == U.star(300)[2].tobytes()
    out, _ = _edge_run("star-empty-rows")
    assert out[[0, 301]].tobytes() == case["Y0"][[0, 301]].tobytes()
    moved = np.any(out[1:301] != case["Y0"][1:301], axis=1)            # a row whose weights are small fires in no early epoch
    assert moved[0] and moved.sum() >= 200


def test_gamma_zero_is_the_run_without_negatives_and_other_a_b_is_another_run():
    cases = _edge_cases()
    zero, none = cases["gamma0"], cases["gamma0-neg0"]
    assert zero["run"]["gamma"] == none["run"]["gamma"] == 0.0 and zero["run"]["neg"] == 5 and none["run"]["neg"] == 0
    assert not np.any(zero["Y0"] == 0.0)                              # no -0.0, which adding alpha * 0 would turn into +0.0
    assert _edge_run("gamma0")[0].tobytes() == _edge_run("gamma0-neg0")[0].tobytes()
    assert not np.any(_edge_run("gamma0")[0] == 0.0)
    assert _edge_run("gamma0")[1]["skipped"] >= 1                     # the negatives were drawn
    ab = cases["a1.5-b0.9"]
    assert (ab["run"]["a"], ab["run"]["b"]) == (1.5, 0.9)
    default = U.layout(*ab["graph"], ab["Y0"], **{**ab["run"], "a": U.A_DEFAULT, "b": U.B_DEFAULT})
    assert not np.array_equal(_edge_run("a1.5-b0.9")[0], default)


def test_late_epochs_fire_where_a_float32_epoch_index_would_not():
    case = _edge_cases()["late-epochs"]
    run, w = case["run"], case["graph"][2]
    assert run["e0"] > 2 ** 24 and run["e1"] <= run["n_epochs"] == 2 ** 31 - 1
    for e in range(run["e0"], run["e1"]):
        true, narrow = U.firing(w, e), U.firing_float32(w, e)
        assert true.any() and np.any(true != narrow), e
    assert 0.5 < 1.0 - run["e0"] / run["n_epochs"] < 0.6             # alpha: the steps are not negligible
    assert np.abs(_edge_run("late-epochs")[0] - case["Y0"]).max() > 1.0


def test_edge_layout_recipes_are_well_conditioned():
    """The rule of ``test_layout_recipes_are_well_conditioned`` for every new case, over its own epochs and arguments."""
    for name, case in _edge_cases().items():
        moved = U.conditioning(case["graph"], case["Y0"], None, extent=case["extent"], run=case["run"])
        print(name, moved)
        assert moved <= 1e-12, name


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
