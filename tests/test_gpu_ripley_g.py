"""GPU: ripley_g (extension, N11) against the two restatements of its definition in ripley_g_restated.py.

Every comparison of counts, sums and p-values is exact (integers); ``mean`` (rtol 1e-12) and ``std`` (rtol 1e-9,
atol 1e-9) carry the tolerances test_gpu_ripley.py uses for the same arithmetic.
"""
import numpy as np
import pytest

from conftest import make_adata
from ripley_g_restated import brute_counts_g, null_tables_g, scipy_counts_g

pytestmark = pytest.mark.gpu

STRUCTURED_RADII = [3.0, 5.0, 8.0, 12.0]


def _run(coords, labels, radii, **kw):
    from spatialcore_amd.spatial import ripley_g

    ad = make_adata(coords, np.zeros((coords.shape[0], 1)), labels=labels)
    ripley_g(ad, "cell_type", radii, **kw)
    return ad.uns["ripley_g"]


def _codes(labels, cats=None):
    cats = sorted(set(np.asarray(labels).tolist())) if cats is None else cats
    return cats, np.array([cats.index(v) for v in np.asarray(labels).tolist()])


def _structured(n=3000, seed=21):
    """test_gpu_ripley's recipe: left half mostly A/B, right half mostly C/D, E everywhere."""
    rng = np.random.default_rng(seed)
    coords = rng.uniform(0, 550, (n, 2))
    left = coords[:, 0] < 275
    labels = np.where(left, rng.choice(["A", "B", "E"], n, p=[.5, .4, .1]), rng.choice(["C", "D", "E"], n, p=[.5, .4, .1]))
    return coords, labels


@pytest.fixture(scope="module")
def structured():
    """The structured input with its restated observed table, shared (read-only) by the tests on it."""
    coords, labels = _structured()
    cats, codes = _codes(labels)
    return coords, labels, cats, codes, brute_counts_g(coords, codes, len(cats), STRUCTURED_RADII)


def _sum_rows(null, obs):
    dev = null - obs
    return np.stack([dev.sum(0), (dev * dev).sum(0), (dev >= 0).sum(0), (dev <= 0).sum(0)])


def _check_counts(coords, labels, radii, cats=None, **kw):
    res = _run(coords, labels, radii, **kw)
    cats, codes = _codes(labels, cats)
    assert res["celltypes"] == cats
    want = brute_counts_g(coords, codes, len(cats), radii)
    assert res["count"].dtype == np.int64 and res["count"].shape == (len(cats), len(cats), len(radii))
    np.testing.assert_array_equal(res["count"], want)
    np.testing.assert_array_equal(res["n_per_type"], np.bincount(codes, minlength=len(cats)))
    return res, want


# ---- counts against the restatement -----------------------------------------------------------------------------------

def test_counts_structured_labels(structured):
    coords, labels, cats, codes, want = structured
    res = _run(coords, labels, STRUCTURED_RADII)
    assert res["celltypes"] == cats and res["count"].dtype == np.int64
    np.testing.assert_array_equal(res["count"], want)
    np.testing.assert_array_equal(want, scipy_counts_g(coords, codes, len(cats), STRUCTURED_RADII))
    n_t = res["n_per_type"]
    np.testing.assert_array_equal(n_t, np.bincount(codes, minlength=len(cats)))
    assert (res["count"] != res["count"].transpose(1, 0, 2)).any()                  # the table is not symmetric
    assert (res["count"] < n_t[:, None, None]).all()                               # ... and not saturated at these radii
    np.testing.assert_array_equal(res["G"], res["count"] / n_t[:, None, None].astype(float))
    ext = coords.max(axis=0) - coords.min(axis=0)
    assert res["area"] == float(ext[0] * ext[1])
    lam = n_t[1] / res["area"]
    np.testing.assert_allclose(res["G_poisson"][0, 1], 1 - np.exp(-lam * np.pi * np.square(STRUCTURED_RADII)), rtol=1e-14)
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
    assert want[:, :, 0].sum() > 200                                       # (a coincident cell counts: d = 0 <= r)


def test_counts_integer_lattice_with_tie_radii():
    g = np.arange(45, dtype=np.float64)
    coords = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    labels = np.random.default_rng(6).choice(["p", "q", "r", "s"], coords.shape[0])
    res, want = _check_counts(coords, labels, [1.0, np.sqrt(2.0), 2.0, np.sqrt(5.0), 3.0])
    assert (np.diff(want.sum(axis=(0, 1))) > 0).all()                      # every tie radius adds first contacts


def test_counts_one_radius_and_thirty_two_radii():
    coords, labels = _structured(n=1500, seed=8)
    _check_counts(coords, labels, [9.0])
    res, want = _check_counts(coords, labels, np.linspace(1.0, 24.0, 32))   # the byte range, the in-row order over 32 bins
    assert (np.diff(want.sum(axis=(0, 1)), prepend=0) > 0).all()           # (every one of the 32 indices is some cell's first contact)


def test_counts_one_type_and_a_sparse_marker():
    rng = np.random.default_rng(9)
    coords = rng.uniform(0, 300, (3000, 2))
    res, want = _check_counts(coords, np.array(["only"] * 3000), [1.0, 2.5, 6.0])
    assert res["count"].shape == (1, 1, 3)
    # T = 2 with a 1 % minority type: a sparse marker, passed as a boolean column
    marker = rng.uniform(size=3000) < 0.01
    radii = [4.0, 9.0, 20.0, 35.0]
    res = _run(coords, marker, radii)
    assert res["celltypes"] == [False, True]
    np.testing.assert_array_equal(res["count"], brute_counts_g(coords, marker.astype(int), 2, radii))
    assert 10 <= res["n_per_type"][1] <= 60


def test_counts_single_cell_type_and_unused_code():
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import ripley_k
    from spatialcore_amd.spatial.neighborhoods import ripley_g_statistics

    rng = np.random.default_rng(10)
    coords = rng.uniform(0, 200, (1200, 2))
    labels = rng.choice(["A", "B"], 1200).astype(object)
    labels[17] = "Z"                                                       # one cell of its own type
    res, _ = _check_counts(coords, labels, [6.0, 12.0])
    iz = res["celltypes"].index("Z")
    ad = make_adata(coords, np.zeros((1200, 1)), labels=labels)
    ripley_k(ad, "cell_type", [6.0, 12.0])
    # every cell has at most one Z neighbour: "has one" and "how many" are the same number
    np.testing.assert_array_equal(res["count"][:, iz], ad.uns["ripley_k"]["count"][:, iz])
    assert (res["count"][iz, iz] == 0).all() and (res["G"][iz, iz] == 0).all() and res["count"][:, iz, -1].sum() > 0
    # a code the labels never use (the native entry point with n_types = 3, codes in {0, 2}): zero row and column
    ctx = _lib.default_context(0)
    codes = np.where(labels == "B", 2, 0).astype(np.int32)
    ctx.ripley_g_build(coords, [6.0, 12.0])
    got = ctx.ripley_g_counts(codes, 3, 0)[0]
    np.testing.assert_array_equal(got, brute_counts_g(coords, codes, 3, [6.0, 12.0]))
    assert (got[1] == 0).all() and (got[:, 1] == 0).all() and (got[0, 2] > 0).all()
    G = ripley_g_statistics(got, np.bincount(codes, minlength=3), 4.0e4)["G"]
    assert np.isnan(G[1]).all() and np.isfinite(G[0]).all() and np.isfinite(G[2]).all()


def test_small_and_empty_inputs():
    from spatialcore_amd import _lib

    res = _run(np.array([[3.0, 4.0]]), np.array(["A"]), [1.0, 2.0], area=1.0)                      # n = 1
    np.testing.assert_array_equal(res["count"], np.zeros((1, 1, 2), dtype=np.int64))
    # n = 2 at distance exactly r: the ball is closed
    xy = np.array([[0.0, 0.0], [3.0, 4.0]])
    res = _run(xy, np.array(["A", "B"]), [np.nextafter(5.0, 0.0), 5.0])
    np.testing.assert_array_equal(res["count"][:, :, 0], np.zeros((2, 2)))
    np.testing.assert_array_equal(res["count"][:, :, 1], [[0, 1], [1, 0]])
    # 257 cells, r below the smallest spacing: no entry at all, nothing is launched over the lists, every count is 0
    xy = np.stack([np.arange(257, dtype=np.float64) * 2.0, (np.arange(257) % 3).astype(np.float64) * 2.0], axis=1)
    codes = (np.arange(257) % 4).astype(np.int32)
    ctx = _lib.default_context(0)
    assert ctx.ripley_g_build(xy, [0.5, 1.5]) == 0
    assert not ctx.ripley_g_counts(codes, 4, 0).any()
    obs, sums = ctx.ripley_g_counter(codes, 4, 3, 0, 5, 2)
    assert not obs.any() and not sums[:2].any() and (sums[2:] == 5).all()
    res = _run(xy, np.array(list("wxyz"))[codes], [0.5, 1.5], n_permutations=4, seed=2, perm_batch=3)
    assert not res["count"].any() and (res["p_value"] == 1.0).all() and (res["std"] == 0).all()


def test_early_exit_and_last_entry_rows(oracle):
    """A disc of 400 cells of three types (radius 4) whose rows hold every other disc cell; ONE cell of a fourth type 9.9
    from the centre, which a disc cell meets only late in its row (its mask fills at one of the last entries, or never:
    the walk must reach the end of the row); 300 background cells far from both.  Under a permutation the rare label
    lands anywhere, and rows that met every type early end early."""
    from spatialcore_amd import _lib

    rng = np.random.default_rng(31)
    rad, ang = 4.0 * np.sqrt(rng.uniform(size=400)), rng.uniform(0, 2 * np.pi, 400)
    disc = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    back = np.stack([rng.uniform(30, 130, 300), rng.uniform(-50, 50, 300)], axis=1)
    coords = np.concatenate([disc, [[9.9, 0.0]], back])
    codes = np.concatenate([rng.integers(0, 3, 400), [3], rng.integers(0, 3, 300)]).astype(np.int32)
    radii = [1.0, 2.5, 6.0, 10.0, 14.0]
    ctx = _lib.default_context(0)
    assert ctx.ripley_g_build(coords, radii) >= 400 * 399
    want = brute_counts_g(coords, codes, 4, radii)
    assert (want[:3, 3, :3] == 0).all() and 0 < want[:3, 3, 3].sum() < want[:3, 3, 4].sum() == 400   # first met at r = 10
    perms = np.stack([oracle.counter_permutation(13, coords.shape[0], p) for p in range(9)])
    null = null_tables_g(coords, codes, 4, radii, perms)
    obs, sums = ctx.ripley_g_counter(codes, 4, 13, 0, 9, 4)
    np.testing.assert_array_equal(obs, want)
    np.testing.assert_array_equal(sums, _sum_rows(null, want))
    ctx.set_permutations(perms)
    np.testing.assert_array_equal(ctx.ripley_g_counts(codes, 4, 9), np.concatenate([null, want[None]]))


# ---- identities against the older paths --------------------------------------------------------------------------------

def test_identities_against_ripley_k_and_the_radius_graph():
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import ripley_k

    coords, labels = _structured(n=2500, seed=12)
    radii = [3.0, 6.0, 13.0, 22.0]
    g = _run(coords, labels, radii)
    ad = make_adata(coords, np.zeros((2500, 1)), labels=labels)
    ripley_k(ad, "cell_type", radii)
    k = ad.uns["ripley_k"]["count"]
    assert (g["count"] <= np.minimum(g["n_per_type"][:, None, None], k)).all()
    np.testing.assert_array_equal(g["count"] > 0, k > 0)
    assert (np.diff(g["count"], axis=2) >= 0).all()
    one = _run(coords, np.array(["only"] * 2500), radii)["count"]
    ctx = _lib.default_context(0)
    for j, r in enumerate(radii):
        indptr, _ = ctx.radius_graph(coords, r)
        assert one[0, 0, j] == np.count_nonzero(np.diff(indptr))


# ---- the null ----------------------------------------------------------------------------------------------------------

def test_null_numpy_source_three_batches(oracle, structured):
    coords, labels, cats, codes, obs = structured
    res = _run(coords, labels, STRUCTURED_RADII, n_permutations=37, seed=5, perm_batch=16)
    perms, _ = oracle.perm_table(5, 3000, 37)
    null = null_tables_g(coords, codes, len(cats), STRUCTURED_RADII, perms)
    np.testing.assert_array_equal(res["count"], obs)
    np.testing.assert_allclose(res["mean"], null.astype(float).mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(res["std"], null.astype(float).std(axis=0), rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(res["p_value"], ((null >= obs).sum(axis=0) + 1) / 38)
    np.testing.assert_array_equal(res["p_value_less"], ((null <= obs).sum(axis=0) + 1) / 38)
    assert res["n_permutations"] == 37 and res["seed"] == 5 and res["rng"] == "numpy"
    # structured labels: same-side types are nearer, opposite-side types farther than random labelling gives
    ia, ib, ic = cats.index("A"), cats.index("B"), cats.index("C")
    print("zscores A->A", res["zscore"][ia, ia], "A->B", res["zscore"][ia, ib], "A->C", res["zscore"][ia, ic],
          "C->A", res["zscore"][ic, ia])
    assert (res["zscore"][ia, ia] > 3).all() and (res["zscore"][ia, ib] > 3).all()
    assert (res["zscore"][ia, ic] < -3).all() and (res["zscore"][ic, ia] < -3).all()


def test_null_philox_source_and_disjoint_ranges(oracle, structured):
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial.neighborhoods import ripley_g_statistics

    coords, labels, cats, codes, obs = structured
    radii, T = STRUCTURED_RADII, len(cats)
    res = _run(coords, labels, radii, n_permutations=21, seed=77, perm_batch=8, rng="philox")
    perms = np.stack([oracle.counter_permutation(77, 3000, p) for p in range(21)])
    null = null_tables_g(coords, codes, T, radii, perms)
    np.testing.assert_array_equal(res["count"], obs)
    np.testing.assert_allclose(res["mean"], null.astype(float).mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(res["std"], null.astype(float).std(axis=0), rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(res["p_value"], ((null >= obs).sum(axis=0) + 1) / 22)
    np.testing.assert_array_equal(res["p_value_less"], ((null <= obs).sum(axis=0) + 1) / 22)
    # two disjoint ranges add up to the whole: what two ranks all-reduce
    ctx = _lib.default_context(0)
    ctx.ripley_g_build(coords, radii)
    c32 = codes.astype(np.int32)
    o_all, s_all = ctx.ripley_g_counter(c32, T, 77, 0, 21, 8)
    o_a, s_a = ctx.ripley_g_counter(c32, T, 77, 0, 10, 8)
    o_b, s_b = ctx.ripley_g_counter(c32, T, 77, 10, 11, 8)
    for o in (o_all, o_a, o_b):
        np.testing.assert_array_equal(o, obs)
    np.testing.assert_array_equal(s_a + s_b, s_all)
    np.testing.assert_array_equal(s_all, _sum_rows(null, obs))
    np.testing.assert_array_equal(
        ripley_g_statistics(obs, res["n_per_type"], res["area"], s_a + s_b, 21)["p_value"], res["p_value"])
    # the per-permutation tables of the table form, fed the same rows
    ctx.set_permutations(perms[:5])
    np.testing.assert_array_equal(ctx.ripley_g_counts(c32, T, 5), np.concatenate([null[:5], obs[None]]))
    np.testing.assert_array_equal(ctx.ripley_g_counts(c32, T, 2, perm_row0=3)[:2], null[3:5])


@pytest.mark.parametrize("T", [16, 23, 32, 33, 46, 64])
def test_null_at_every_permutations_per_pass_and_mask_width(oracle, T):
    """Four radii give histograms of 4 T T words: T = 16 / 23 / 32 / 46 are the smallest T at which the counting kernel
    runs 8, 4, 2 and 1 permutations per pass (the largest NP with NP * (words | 1) <= 16384; the tests above run 16);
    T = 33 is the first type in the second mask word, T = 64 the envelope's edge.  21 counter-based permutations in
    batches of 8, the last ragged: the observed table and the four sum rows equal the restatement, exactly; so do table
    rows at an offset."""
    from spatialcore_amd import _lib

    n, P, seed, radii = 1200, 21, 41, [10.0, 20.0, 35.0, 50.0]
    rng = np.random.default_rng(16)
    coords = rng.uniform(0, 250, (n, 2))
    codes = rng.integers(0, T, n).astype(np.int32)
    codes[:T] = np.arange(T)                                                # (every type occurs)
    perms = np.stack([oracle.counter_permutation(seed, n, p) for p in range(P)])
    null = null_tables_g(coords, codes, T, radii, perms)
    obs = brute_counts_g(coords, codes, T, radii)
    ctx = _lib.default_context(0)
    ctx.ripley_g_build(coords, radii)
    got_obs, got_sums = ctx.ripley_g_counter(codes, T, seed, 0, P, 8)
    np.testing.assert_array_equal(got_obs, obs)
    np.testing.assert_array_equal(got_sums, _sum_rows(null, obs))
    ctx.set_permutations(perms)
    np.testing.assert_array_equal(ctx.ripley_g_counts(codes, T, 17, perm_row0=2), np.concatenate([null[2:19], obs[None]]))


# ---- state and envelope ------------------------------------------------------------------------------------------------

def test_run_to_run_identical_and_no_stale_state():
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import ripley_k

    coords, labels = _structured(n=2000, seed=14)
    radii = [4.0, 8.0, 15.0]
    kw = dict(n_permutations=40, seed=3, perm_batch=16, rng="philox")

    def k_run():
        ad = make_adata(coords, np.zeros((2000, 1)), labels=labels)
        ripley_k(ad, "cell_type", radii, **kw)
        return ad.uns["ripley_k"]

    a = _run(coords, labels, radii, **kw)
    b = _run(coords, labels, radii, **kw)
    for key in ("count", "G", "G_poisson", "mean", "std", "zscore", "p_value", "p_value_less"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    # a ripley_k call between two ripley_g calls, and the reverse, changes neither result
    k1 = k_run()
    c = _run(coords, labels, radii, **kw)
    k2 = k_run()
    for key in ("count", "p_value", "p_value_less", "std"):
        np.testing.assert_array_equal(a[key], c[key], err_msg=key)
        np.testing.assert_array_equal(k1[key], k2[key], err_msg=key)
    # both lists live side by side on the bins of the later build ... until the next build replaces those
    ctx = _lib.default_context(0)
    _, codes = _codes(labels)
    c32 = codes.astype(np.int32)
    ctx.ripley_g_build(coords, radii)
    with pytest.raises(_lib.SpatialCoreHipError, match="no pair list"):
        ctx.ripley_counts(c32, 5, 0)
    np.testing.assert_array_equal(ctx.ripley_g_counts(c32, 5, 0)[0], a["count"])
    # ... and a neighbour search after the build leaves no stale list reachable
    ctx.knn(coords, 5)
    with pytest.raises(_lib.SpatialCoreHipError, match="no list"):
        ctx.ripley_g_counts(c32, 5, 0)
    with pytest.raises(_lib.SpatialCoreHipError, match="no list"):
        ctx.ripley_g_counter(c32, 5, 0, 0, 4, 4)


def test_shapes_beyond_the_envelope_are_refused_with_the_limit_and_the_shape():
    rng = np.random.default_rng(15)
    n = 2000
    coords = rng.uniform(0, 100, (n, 2))
    labels = np.array([f"t{v:02d}" for v in np.arange(n) % 65])
    with pytest.raises(ValueError, match=r"n_types = 65 exceeds the limit of 64 cell types"):
        _run(coords, labels, [2.0, 4.0])
    labels = np.array([f"t{v:02d}" for v in np.arange(n) % 40])
    with pytest.raises(ValueError, match=r"n_types \* n_types \* n_radii = 17600 exceeds the limit of 16384 histogram words.*"
                                         r"n_types = 40, n_radii = 11"):
        _run(coords, labels, np.linspace(1.0, 8.0, 11))
    # T T R = 16384 exactly is inside the envelope: T = 32, R = 16, one histogram per pass
    labels = np.array([f"t{v:02d}" for v in rng.integers(0, 32, n)])
    _check_counts(coords, labels, np.linspace(1.0, 12.0, 16), n_permutations=3, seed=1, rng="philox", perm_batch=2)
