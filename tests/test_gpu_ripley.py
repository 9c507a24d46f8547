"""GPU: ripley_k (extension, N6) against the numpy restatement of its definition and scipy's exact tree counts.

Every comparison of counts, exceedances and p-values is exact (integers); ``mean`` (rtol 1e-12) and ``std``
(rtol 1e-9, atol 1e-9) carry the tolerances test_neighborhood_enrichment_extension uses for the same arithmetic.
"""
import numpy as np
import pytest

from conftest import make_adata, synth
from ripley_restated import brute_counts, null_tables, scipy_counts

pytestmark = pytest.mark.gpu


def _run(coords, labels, radii, **kw):
    from spatialcore_amd.spatial import ripley_k

    ad = make_adata(coords, np.zeros((coords.shape[0], 1)), labels=labels)
    ripley_k(ad, "cell_type", radii, **kw)
    return ad.uns["ripley_k"]


def _codes(labels, cats=None):
    cats = sorted(set(np.asarray(labels).tolist())) if cats is None else cats
    return cats, np.array([cats.index(v) for v in np.asarray(labels).tolist()])


def _structured(n=3000, seed=21):
    """The enrichment test's recipe: left half mostly A/B, right half mostly C/D, E everywhere."""
    rng = np.random.default_rng(seed)
    coords = rng.uniform(0, 550, (n, 2))
    left = coords[:, 0] < 275
    labels = np.where(left, rng.choice(["A", "B", "E"], n, p=[.5, .4, .1]), rng.choice(["C", "D", "E"], n, p=[.5, .4, .1]))
    return coords, labels


def _check_counts(coords, labels, radii, cats=None):
    res = _run(coords, labels, radii)
    cats, codes = _codes(labels, cats)
    assert res["celltypes"] == cats
    want = brute_counts(coords, codes, len(cats), radii)
    assert res["count"].dtype == np.int64 and res["count"].shape == (len(cats), len(cats), len(radii))
    np.testing.assert_array_equal(res["count"], want)
    np.testing.assert_array_equal(res["n_per_type"], np.bincount(codes, minlength=len(cats)))
    return res, want


def test_counts_structured_labels():
    coords, labels = _structured()
    res, _ = _check_counts(coords, labels, [5.0, 10.0, 22.0, 40.0])
    ext = coords.max(axis=0) - coords.min(axis=0)
    assert res["area"] == float(ext[0] * ext[1])
    n_t = res["n_per_type"].astype(float)
    np.testing.assert_allclose(res["K"][0, 1], res["area"] * res["count"][0, 1] / (n_t[0] * n_t[1]), rtol=1e-15)
    np.testing.assert_allclose(res["K"][2, 2], res["area"] * res["count"][2, 2] / (n_t[2] * (n_t[2] - 1)), rtol=1e-15)
    np.testing.assert_allclose(res["L"], np.sqrt(res["K"] / np.pi), rtol=1e-15)
    assert "p_value" not in res and res["n_permutations"] == 0


def test_counts_clustered_coordinates():
    rng = np.random.default_rng(4)
    centres = rng.uniform(0, 400, (12, 2))
    coords = centres[rng.integers(0, 12, 2500)] + rng.normal(0, 6.0, (2500, 2))
    labels = rng.choice(["a", "b", "c"], 2500)
    _check_counts(coords, labels, [2.0, 4.0, 8.0, 16.0, 30.0])


def test_counts_duplicate_points():
    rng = np.random.default_rng(5)
    base = rng.uniform(0, 100, (400, 2))
    coords = np.concatenate([base, base[:200], base[:50], base[:50]])     # up to four cells on one spot
    labels = rng.choice(["x", "y", "z"], coords.shape[0])
    res, want = _check_counts(coords, labels, [0.5, 3.0, 9.0])
    assert want[:, :, 0].sum() >= 2 * (200 + 3 * 50)                       # (the coincident pairs are counted: d = 0 <= r)


def test_counts_integer_lattice_with_tie_radii():
    g = np.arange(45, dtype=np.float64)
    coords = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    labels = np.random.default_rng(6).choice(["p", "q", "r", "s"], coords.shape[0])
    _check_counts(coords, labels, [5.0, 5.0 * np.sqrt(2.0), 10.0, 15.0, 25.0])


def test_counts_one_radius_and_thirty_two_radii():
    coords, labels = _structured(n=1500, seed=8)
    _check_counts(coords, labels, [17.0])
    _check_counts(coords, labels, np.linspace(2.0, 45.0, 32))


def test_counts_one_type_and_a_sparse_marker():
    rng = np.random.default_rng(9)
    coords = rng.uniform(0, 300, (3000, 2))
    res, want = _check_counts(coords, np.array(["only"] * 3000), [4.0, 9.0, 20.0])
    assert res["count"].shape == (1, 1, 3)
    # T = 2 with a 1 % minority type: a sparse marker, passed as a boolean column
    marker = rng.uniform(size=3000) < 0.01
    res = _run(coords, marker, [4.0, 9.0, 20.0, 35.0])
    assert res["celltypes"] == [False, True]
    np.testing.assert_array_equal(res["count"], brute_counts(coords, marker.astype(int), 2, [4.0, 9.0, 20.0, 35.0]))
    assert 10 <= res["n_per_type"][1] <= 60


def test_counts_single_cell_type_and_absent_category():
    import pandas as pd

    rng = np.random.default_rng(10)
    coords = rng.uniform(0, 200, (1200, 2))
    labels = rng.choice(["A", "B"], 1200).astype(object)
    labels[17] = "Z"                                                      # one cell of its own type
    res, _ = _check_counts(coords, labels, [6.0, 12.0])
    iz = res["celltypes"].index("Z")
    assert np.isnan(res["K"][iz, iz]).all() and np.isfinite(res["K"][iz, 0]).all()
    assert (res["count"][iz, iz] == 0).all()
    # a category without cells: _label_codes factorises the VALUES, so the table has the types that occur --
    # and a type that the codes never use (the native entry point with n_types = 3, codes in {0, 2}) counts zero
    from spatialcore_amd import _lib

    ad = make_adata(coords, np.zeros((1200, 1)),
                    labels=pd.Categorical(np.where(labels == "Z", "A", labels), categories=["A", "B", "ghost"]))
    from spatialcore_amd.spatial import ripley_k

    ripley_k(ad, "cell_type", [6.0, 12.0])
    assert ad.uns["ripley_k"]["celltypes"] == ["A", "B"]
    ctx = _lib.default_context(0)
    codes = np.where(labels == "B", 2, 0).astype(np.int32)
    ctx.ripley_build(coords, [6.0, 12.0])
    got = ctx.ripley_counts(codes, 3, 0)[0]
    np.testing.assert_array_equal(got, brute_counts(coords, codes, 3, [6.0, 12.0]))
    assert (got[1] == 0).all() and (got[:, 1] == 0).all()
    from spatialcore_amd.spatial.neighborhoods import ripley_statistics

    K = ripley_statistics(got, np.bincount(codes, minlength=3), 4.0e4)["K"]
    assert np.isnan(K[1]).all() and np.isnan(K[:, 1]).all() and np.isfinite(K[0, 2]).all()


def test_identities_against_the_older_paths():
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import neighborhood_enrichment

    coords, labels = _structured(n=2500, seed=12)
    radii = [6.0, 13.0, 22.0, 31.0]
    res = _run(coords, labels, radii)
    ctx = _lib.default_context(0)
    np.testing.assert_array_equal(res["count"], res["count"].transpose(1, 0, 2))
    for j, r in enumerate(radii):
        indptr, indices = ctx.radius_graph(coords, r)
        assert res["count"][:, :, j].sum() == indices.size == indptr[-1]
        ad = make_adata(coords, np.zeros((2500, 1)), labels=labels)
        neighborhood_enrichment(ad, "cell_type", method="radius", radius=r, n_permutations=0)
        np.testing.assert_array_equal(res["count"][:, :, j], ad.uns["neighborhood_enrichment"]["count"])


def test_null_numpy_source_three_batches(oracle):
    coords, labels = _structured()
    radii = [5.0, 10.0, 22.0, 40.0]
    res = _run(coords, labels, radii, n_permutations=37, seed=5, perm_batch=16)
    cats, codes = _codes(labels)
    perms, _ = oracle.perm_table(5, 3000, 37)
    null = null_tables(coords, codes, len(cats), radii, perms)
    obs = brute_counts(coords, codes, len(cats), radii)
    np.testing.assert_array_equal(res["count"], obs)
    np.testing.assert_allclose(res["mean"], null.astype(float).mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(res["std"], null.astype(float).std(axis=0), rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(res["p_value"], ((null >= obs).sum(axis=0) + 1) / 38)
    np.testing.assert_array_equal(res["p_value_less"], ((null <= obs).sum(axis=0) + 1) / 38)
    assert res["n_permutations"] == 37 and res["seed"] == 5 and res["rng"] == "numpy"
    # structured labels: same-side types cluster, opposite-side types avoid each other below the structure's scale (275)
    ia, ib, ic = cats.index("A"), cats.index("B"), cats.index("C")
    assert (res["zscore"][ia, ia] > 3).all() and (res["zscore"][ia, ib] > 3).all()
    assert (res["zscore"][ia, ic] < -3).all() and (res["zscore"][ic, ia] < -3).all()


def test_null_philox_source_and_disjoint_halves(oracle):
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial.neighborhoods import ripley_statistics

    coords, labels = _structured()
    radii = [5.0, 10.0, 22.0, 40.0]
    res = _run(coords, labels, radii, n_permutations=21, seed=77, perm_batch=8, rng="philox")
    cats, codes = _codes(labels)
    perms = np.stack([oracle.counter_permutation(77, 3000, p) for p in range(21)])
    null = null_tables(coords, codes, len(cats), radii, perms)
    obs = brute_counts(coords, codes, len(cats), radii)
    np.testing.assert_array_equal(res["count"], obs)
    np.testing.assert_allclose(res["mean"], null.astype(float).mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(res["std"], null.astype(float).std(axis=0), rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(res["p_value"], ((null >= obs).sum(axis=0) + 1) / 22)
    np.testing.assert_array_equal(res["p_value_less"], ((null <= obs).sum(axis=0) + 1) / 22)
    # two disjoint halves add up to the whole: what two ranks all-reduce
    ctx = _lib.default_context(0)
    ctx.ripley_build(coords, radii)
    c32 = codes.astype(np.int32)
    o_all, s_all = ctx.ripley_counter(c32, len(cats), 77, 0, 21, 8)
    o_a, s_a = ctx.ripley_counter(c32, len(cats), 77, 0, 10, 8)
    o_b, s_b = ctx.ripley_counter(c32, len(cats), 77, 10, 11, 8)
    np.testing.assert_array_equal(o_all, obs)
    np.testing.assert_array_equal(o_a, obs)
    np.testing.assert_array_equal(o_b, obs)
    np.testing.assert_array_equal(s_a + s_b, s_all)
    dev = null - obs
    np.testing.assert_array_equal(s_all, np.stack([dev.sum(0), (dev * dev).sum(0), (dev >= 0).sum(0), (dev <= 0).sum(0)]))
    np.testing.assert_array_equal(ripley_statistics(obs, res["n_per_type"], res["area"], s_a + s_b, 21)["p_value"], res["p_value"])
    # the per-permutation tables of the table form, fed the same rows
    ctx.set_permutations(perms[:5])
    np.testing.assert_array_equal(ctx.ripley_counts(c32, len(cats), 5)[:5], null[:5])
    np.testing.assert_array_equal(ctx.ripley_counts(c32, len(cats), 2, perm_row0=3)[:2], null[3:5])


@pytest.mark.parametrize("T", [23, 32, 45, 64])
def test_null_at_every_permutations_per_pass(oracle, T):
    """Four radii and T = 23 / 32 / 45 / 64 give histograms of 2 T (T + 1) = 1104 / 2112 / 4140 / 8320 words: the
    smallest T at which the pair kernel runs 8, 4, 2 and 1 permutations per pass (the largest NP with
    NP * (words | 1) <= 16384; the tests above run 16).  21 counter-based permutations in batches of 8, the last ragged:
    the observed table and the four sum rows equal the restatement, exactly; so do table rows at an offset."""
    from spatialcore_amd import _lib

    n, P, seed, radii = 1200, 21, 41, [4.0, 8.0, 13.0, 20.0]
    rng = np.random.default_rng(16)
    coords = rng.uniform(0, 250, (n, 2))
    codes = rng.integers(0, T, n).astype(np.int32)
    perms = np.stack([oracle.counter_permutation(seed, n, p) for p in range(P)])
    null = null_tables(coords, codes, T, radii, perms)
    obs = brute_counts(coords, codes, T, radii)
    ctx = _lib.default_context(0)
    ctx.ripley_build(coords, radii)
    got_obs, got_sums = ctx.ripley_counter(codes, T, seed, 0, P, 8)
    dev = null - obs
    np.testing.assert_array_equal(got_obs, obs)
    np.testing.assert_array_equal(got_sums, np.stack([dev.sum(0), (dev * dev).sum(0), (dev >= 0).sum(0), (dev <= 0).sum(0)]))
    ctx.set_permutations(perms)
    np.testing.assert_array_equal(ctx.ripley_counts(codes, T, 17, perm_row0=2), np.concatenate([null[2:19], obs[None]]))


def test_run_to_run_identical_and_no_stale_state():
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import morans_i

    coords, labels = _structured(n=2000, seed=14)
    radii = [7.0, 15.0, 30.0]
    a = _run(coords, labels, radii, n_permutations=40, seed=3, perm_batch=16, rng="philox")
    b = _run(coords, labels, radii, n_permutations=40, seed=3, perm_batch=16, rng="philox")
    for key in ("count", "K", "L", "mean", "std", "zscore", "p_value", "p_value_less"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    # ripley_k between two morans_i calls: the graph state of neither leaks into the other
    xy, X = synth(4000, 6, 11, dtype=np.float32)
    genes = [f"g{i}" for i in range(6)]
    ad1 = make_adata(xy, X)
    morans_i(ad1, genes=genes, n_neighbors=6, n_permutations=49, seed=0)
    c = _run(coords, labels, radii, n_permutations=40, seed=3, perm_batch=16, rng="philox")
    ad2 = make_adata(xy, X)
    morans_i(ad2, genes=genes, n_neighbors=6, n_permutations=49, seed=0)
    for col in ("I", "z_score", "p_value"):
        np.testing.assert_array_equal(ad1.uns["morans_i"][col].values, ad2.uns["morans_i"][col].values, err_msg=col)
    np.testing.assert_array_equal(a["count"], c["count"])
    np.testing.assert_array_equal(a["p_value"], c["p_value"])
    # ... and a neighbour search after the build leaves no stale pair list reachable
    ctx = _lib.default_context(0)
    _, codes = _codes(labels)
    ctx.ripley_build(coords, radii)
    ctx.knn(coords, 5)
    with pytest.raises(_lib.SpatialCoreHipError, match="no pair list"):
        ctx.ripley_counts(codes.astype(np.int32), 5, 0)
    with pytest.raises(_lib.SpatialCoreHipError, match="no pair list"):
        ctx.ripley_counter(codes.astype(np.int32), 5, 0, 0, 4, 4)


def test_shapes_beyond_the_lds_limit_are_refused_with_the_limit():
    rng = np.random.default_rng(15)
    n = 2000
    coords = rng.uniform(0, 100, (n, 2))
    labels = np.array([f"t{v:02d}" for v in np.arange(n) % 96])
    radii = np.linspace(1.0, 8.0, 32)
    with pytest.raises(ValueError, match=r"n_types \(n_types \+ 1\) / 2 \* n_radii = 148992 exceeds the limit of 16384"):
        _run(coords, labels, radii)
    # T T R = 16384 exactly is inside the envelope: T = 32, R = 16, one histogram per pass
    labels = np.array([f"t{v:02d}" for v in rng.integers(0, 32, n)])
    _check_counts(coords, labels, np.linspace(1.0, 8.0, 16))
    # ... and so is the largest T with three radii (T (T + 1) / 2 * R = 13968)
    labels = np.array([f"t{v:02d}" for v in np.arange(n) % 96])
    res = _run(coords, labels, [2.0, 4.0, 6.0], n_permutations=3, seed=1, rng="philox", perm_batch=2)
    np.testing.assert_array_equal(res["count"], brute_counts(coords, np.arange(n) % 96, 96, [2.0, 4.0, 6.0]))


@pytest.mark.timeout(900)
def test_at_size_one_million_cells(oracle):
    """n = 10^6 uniform cells, T = 20 independent labels, 8 radii: the WHOLE observed table against scipy's tree counts;
    512 counter-based permutations in two halves that add up to the whole and to what the public function reports;
    two sampled permutations' own tables (six type pairs each) against scipy on the permuted labels."""
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial.neighborhoods import ripley_statistics

    n, T, P, seed = 1_000_000, 20, 512, 9
    rng = np.random.default_rng(42)
    coords = rng.uniform(0, 1.0e4, (n, 2))
    codes = rng.integers(0, T, n).astype(np.int32)
    radii = [5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 40.0, 50.0]
    labels = np.array([f"type{v:02d}" for v in range(T)])[codes]
    res = _run(coords, labels, radii, n_permutations=P, seed=seed, rng="philox")
    want = scipy_counts(coords, codes, T, radii)
    print(f"ordered pairs at r = 50: {want[:, :, -1].sum():,}")
    np.testing.assert_array_equal(res["count"], want)
    assert want[:, :, -1].sum() == 78_187_486
    assert np.nanmax(np.abs(res["zscore"])) < 8          # independent labels: nothing is enriched (the enrichment test's bound)
    ctx = _lib.default_context(0)
    assert ctx.ripley_build(coords, radii) == 78_187_486
    o_a, s_a = ctx.ripley_counter(codes, T, seed, 0, P // 2, 512)
    o_b, s_b = ctx.ripley_counter(codes, T, seed, P // 2, P - P // 2, 512)
    o_all, s_all = ctx.ripley_counter(codes, T, seed, 0, P, 512)
    np.testing.assert_array_equal(o_a, want)
    np.testing.assert_array_equal(o_b, want)
    np.testing.assert_array_equal(s_a + s_b, s_all)
    stats = ripley_statistics(want, np.bincount(codes, minlength=T), res["area"], s_all, P)
    for key in ("K", "L", "mean", "std", "zscore", "p_value", "p_value_less"):
        np.testing.assert_array_equal(res[key], stats[key], err_msg=key)
    assert (s_all[2] + s_all[3] >= P).all()              # every permutation is >= or <= (both when equal)
    pick = np.random.default_rng(1)
    for p in (3, 400):
        perm = oracle.counter_permutation(seed, n, p)
        ctx.set_permutations(perm[None, :])
        got = ctx.ripley_counts(codes, T, 1)
        np.testing.assert_array_equal(got[1], want)
        pairs = [tuple(sorted(pick.integers(0, T, 2).tolist())) for _ in range(6)]
        ref = scipy_counts(coords, codes[perm], T, radii, pairs=pairs)
        for a, b in pairs:
            np.testing.assert_array_equal(got[0][a, b], ref[a, b], err_msg=f"permutation {p}, types ({a}, {b})")
            np.testing.assert_array_equal(got[0][b, a], ref[a, b], err_msg=f"permutation {p}, types ({b}, {a})")
