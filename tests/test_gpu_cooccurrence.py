"""GPU: co_occurrence (extension, N9) against the numpy restatement of its definition.

Counts, ``n_per_type`` and ``interval`` are compared exactly (integers, and float64 thresholds from the same
arithmetic); ``occ`` with rtol 1e-6: float32 storage of the same float64 formula on the same integers.
"""
import functools

import numpy as np
import pandas as pd
import pytest

from conftest import make_adata
from cooccurrence_restated import brute_counts, occ, thresholds

pytestmark = pytest.mark.gpu

TILE = 1024      # CO_TILE of sc_cooccur.hip: target points per LDS tile
KEY = "cell_type_co_occurrence"


def _run(coords, labels, interval, **kw):
    from spatialcore_amd.spatial import co_occurrence

    ad = make_adata(coords, np.zeros((coords.shape[0], 1)), labels=labels)
    co_occurrence(ad, "cell_type", interval=interval, **kw)
    return ad.uns[KEY]


def _codes(labels, cats=None):
    cats = sorted(set(np.asarray(labels).tolist())) if cats is None else list(cats)
    return cats, np.array([cats.index(v) for v in np.asarray(labels).tolist()])


def _check(coords, labels, interval, cats=None, want=None):
    """One public call against the restatement; returns (result, expected counts, ordered pairs beyond the last threshold)."""
    res = _run(coords, labels, interval)
    cats, codes = _codes(labels, cats)
    thr = thresholds(coords, interval) if isinstance(interval, int) else np.sort(np.asarray(interval, dtype=np.float64))
    count, dropped = brute_counts(coords, codes, len(cats), thr) if want is None else want
    assert res["celltypes"] == cats
    assert res["count"].dtype == np.int64 and res["count"].shape == (len(cats), len(cats), thr.size)
    np.testing.assert_array_equal(res["interval"], thr)
    np.testing.assert_array_equal(res["count"], count)
    np.testing.assert_array_equal(res["n_per_type"], np.bincount(codes, minlength=len(cats)))
    assert res["occ"].dtype == np.float32 and res["occ"].shape == (len(cats), len(cats), thr.size - 1)
    np.testing.assert_allclose(res["occ"], occ(count), rtol=1e-6, equal_nan=True)
    return res, count, dropped


@functools.lru_cache(maxsize=None)
def _structured(n=3000, seed=21):
    """test_gpu_ripley's recipe: left half mostly A/B, right half mostly C/D, E everywhere; with the restatement's
    table for interval=50, computed once for the tests that share the input."""
    rng = np.random.default_rng(seed)
    coords = rng.uniform(0, 550, (n, 2))
    left = coords[:, 0] < 275
    labels = np.where(left, rng.choice(["A", "B", "E"], n, p=[.5, .4, .1]), rng.choice(["C", "D", "E"], n, p=[.5, .4, .1]))
    _, codes = _codes(labels)
    want = brute_counts(coords, codes, 5, thresholds(coords, 50))
    for a in (coords, labels, want[0]):
        a.setflags(write=False)
    return coords, labels, want


def test_structured_labels_default_interval():
    from spatialcore_amd import _lib

    coords, labels, want = _structured()
    res, count, dropped = _check(coords, labels, 50, want=want)
    n = coords.shape[0]
    assert (count.sum(axis=(0, 1)) > 0).all()                      # every one of the 50 bins is in use
    assert 0.1 < dropped / (n * (n - 1)) < 0.5                      # ... and so is the drop path
    np.testing.assert_array_equal(res["count"], res["count"].transpose(1, 0, 2))
    # the prefix sums are the radius graphs' nnz
    ctx = _lib.default_context(0)
    cum = np.cumsum(res["count"].sum(axis=(0, 1)))
    for j in (0, 7, 49):
        indptr, _ = ctx.radius_graph(coords, float(res["interval"][j]))
        assert cum[j] == indptr[-1]
    # same-side types co-occur at short range, opposite-side types avoid each other
    cats = res["celltypes"]
    ia, ib, ic = cats.index("A"), cats.index("B"), cats.index("C")
    assert res["occ"][ia, ib, 2] > 1.3 and res["occ"][ia, ic, 2] < 0.5


def test_chunk_edges_and_an_unused_category():
    sizes = {"one": 1, "c255": 255, "c256": 256, "c257": 257, "c513": 513}
    cats = ["c255", "c256", "ghost", "c257", "one", "c513"]          # the unused category sits in the middle
    rng = np.random.default_rng(31)
    labels = rng.permutation(np.repeat(list(sizes), list(sizes.values())))
    coords = rng.uniform(0, 300, (labels.size, 2))
    res, _, _ = _check(coords, pd.Categorical(labels, categories=cats), 24, cats=cats)
    g = cats.index("ghost")
    assert res["n_per_type"][g] == 0 and res["n_per_type"][cats.index("one")] == 1
    assert (res["count"][g] == 0).all() and (res["count"][:, g] == 0).all()
    assert np.isnan(res["occ"][g]).all() and np.isnan(res["occ"][:, g]).all()
    assert (res["count"][cats.index("one"), cats.index("one")] == 0).all()


@pytest.mark.parametrize("size", [TILE - 1, TILE, TILE + 1, TILE + 2])
def test_tile_edges(size):
    """One type of ``size`` cells between two small ones: its own (diagonal) block streams size - 1 positions behind
    the first chunk's first point -- TILE - 1, TILE, TILE + 1 for the last three sizes -- the chunks of "a" stream all
    ``size`` of it as another type, and its chunks stream "c"."""
    rng = np.random.default_rng(40 + size)
    labels = rng.permutation(np.repeat(["a", "b", "c"], [300, size, 130]))
    coords = rng.uniform(0, 200, (labels.size, 2))
    _check(coords, labels, 16)


@pytest.mark.parametrize("interval", [[0.0, 1.0, 3.0], [0.5, 3.0, 9.0]])
def test_coincident_points(interval):
    rng = np.random.default_rng(5)
    base = rng.uniform(0, 100, (400, 2))
    coords = np.concatenate([base, base[:200], base[:50], base[:50]])     # 50 spots with four cells, 150 with two
    labels = rng.choice(["x", "y", "z"], coords.shape[0])
    res, _, _ = _check(coords, labels, interval)
    coincident = 50 * 4 * 3 + 150 * 2 * 1                                  # ordered pairs with d = 0
    if interval[0] == 0.0:
        assert res["count"][:, :, 0].sum() == coincident                  # d2 = 0 <= fl(0 * 0): bin 0, and nothing else is
    else:
        assert res["count"][:, :, 0].sum() >= coincident


def test_integer_lattice_with_thresholds_on_the_ties():
    m = 45
    g = np.arange(m, dtype=np.float64)
    coords = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    labels = np.random.default_rng(6).choice(["p", "q", "r", "s"], coords.shape[0])
    thr = [1.0, np.sqrt(2.0), 2.0, 5.0, 13.0]
    res, _, _ = _check(coords, labels, thr)

    def lattice_pairs(pred):
        """Ordered pairs of lattice points whose integer squared distance satisfies pred, from the geometry alone."""
        return sum((m - abs(dx)) * (m - abs(dy)) for dx in range(-m + 1, m) for dy in range(-m + 1, m)
                   if (dx or dy) and pred(dx * dx + dy * dy))

    per_bin = res["count"].sum(axis=(0, 1))
    assert per_bin[0] == lattice_pairs(lambda d2: d2 <= 1)
    assert per_bin[1] == lattice_pairs(lambda d2: d2 == 2)                 # 2 < fl(sqrt 2 * sqrt 2): inside
    assert per_bin[2] == lattice_pairs(lambda d2: 2 < d2 <= 4)
    assert per_bin[3] == lattice_pairs(lambda d2: 4 < d2 <= 25)            # closed upper edge
    assert per_bin[4] == lattice_pairs(lambda d2: 25 < d2 <= 169)          # closed upper edge
    # the pairs ON the edge d2 = 25, on their own: a threshold one ulp below 5 splits them off
    split = _run(coords, labels, [1.0, np.sqrt(2.0), 2.0, np.nextafter(5.0, 0.0), 5.0, 13.0])
    on_edge = 4 * (m - 5) * m + 8 * (m - 3) * (m - 4)                      # (+-5, 0), (0, +-5); (+-3, +-4), (+-4, +-3)
    assert on_edge == lattice_pairs(lambda d2: d2 == 25) == 20976
    assert split["count"][:, :, 4].sum() == on_edge
    assert split["count"][:, :, 3].sum() == per_bin[3] - on_edge


def test_limits_two_thresholds_and_128_pass_129_are_refused():
    coords, labels, _ = _structured(n=1500, seed=8)
    _check(coords, labels, [3.0, 40.0])
    _check(coords, labels, 2)
    _check(coords, labels, 128)
    _check(coords, labels, np.linspace(0.0, 90.0, 128))
    with pytest.raises(ValueError, match="2 to 128 thresholds, got 129"):
        _run(coords, labels, 129)
    with pytest.raises(ValueError, match="2 to 128 thresholds, got 129"):
        _run(coords, labels, np.linspace(1.0, 90.0, 129))


def test_single_type():
    rng = np.random.default_rng(9)
    coords = rng.uniform(0, 300, (2000, 2))
    res, count, _ = _check(coords, np.array(["only"] * 2000), 20)
    assert res["count"].shape == (1, 1, 20)
    present = count[0, 0, 1:] > 0
    np.testing.assert_array_equal(res["occ"][0, 0][present], 1.0)


def test_order_independence_and_repeatability():
    coords, labels, want = _structured()
    a = _run(coords, labels, 50)
    b = _run(coords, labels, 50)
    assert a["count"].tobytes() == b["count"].tobytes() and a["occ"].tobytes() == b["occ"].tobytes()
    perm = np.random.default_rng(77).permutation(coords.shape[0])
    thr = a["interval"]                      # (the integer rule picks cells by index-stable order: pass the values)
    c = _run(coords[perm], labels[perm], thr)
    np.testing.assert_array_equal(c["count"], a["count"])
    np.testing.assert_array_equal(c["count"], want[0])
    assert c["occ"].tobytes() == a["occ"].tobytes()


def test_context_state_survives_the_call():
    from ripley_restated import brute_counts as ripley_brute
    from spatialcore_amd import _lib

    coords, labels, want = _structured()
    _, codes = _codes(labels)
    codes = codes.astype(np.int32)
    radii = [5.0, 10.0, 22.0]
    ctx = _lib.default_context(0)
    ctx.ripley_build(coords, radii)
    before = ctx.ripley_counts(codes, 5, 0)
    ctx.ripley_build(coords, radii)
    order = np.argsort(codes, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=5))])
    got = ctx.cooccurrence_counts(coords[order], off, thresholds(coords, 50))
    np.testing.assert_array_equal(got, want[0])
    after = ctx.ripley_counts(codes, 5, 0)                 # the pair list is still there, and still right
    np.testing.assert_array_equal(after, before)
    np.testing.assert_array_equal(after[0], ripley_brute(coords, codes, 5, radii))
    # ... and so is an active graph
    ctx.knn(coords, 6, fetch=False)
    ctx.graph_from_knn(1.0)
    g0 = ctx.get_graph()
    ctx.cooccurrence_counts(coords[order], off, [1.0, 2.0])
    for x, y in zip(g0, ctx.get_graph()):
        np.testing.assert_array_equal(x, y)
    # an empty type through the entry point itself, and the library's own refusals as ValueError
    off6 = np.concatenate([off[:2], off[1:]])              # type 1 empty
    got6 = ctx.cooccurrence_counts(coords[order], off6, thresholds(coords, 50))
    np.testing.assert_array_equal(np.delete(np.delete(got6, 1, axis=0), 1, axis=1), want[0])
    assert (got6[1] == 0).all() and (got6[:, 1] == 0).all()
    with pytest.raises(ValueError, match="strictly increasing"):
        ctx.cooccurrence_counts(coords[order], off, [2.0, 1.0])
    bad = coords[order].copy()
    bad[17, 1] = np.inf
    with pytest.raises(ValueError, match="point coordinate 17 is not finite"):
        ctx.cooccurrence_counts(bad, off, [1.0, 2.0])


def test_api_keys_dtypes_copy_columns_keywords_and_metadata():
    from spatialcore_amd.spatial import co_occurrence

    coords, labels, _ = _structured(n=1200, seed=3)
    cats, codes = _codes(labels)
    thr = thresholds(coords, 10)
    count, _ = brute_counts(coords, codes, 5, thr)
    # a string column; the parallelism keywords are accepted and change nothing
    ad = make_adata(coords, np.zeros((1200, 1)), labels=labels)
    out = co_occurrence(ad, "cell_type", interval=10, n_splits=4, n_jobs=8, backend="threading", show_progress_bar=False)
    assert out is ad
    res = ad.uns[KEY]
    assert set(res) == {"occ", "interval", "count", "celltypes", "n_per_type"}
    assert res["occ"].dtype == np.float32 and res["occ"].shape == (5, 5, 9)
    assert res["interval"].dtype == np.float64 and res["interval"].shape == (10,)
    assert res["count"].dtype == np.int64 and res["count"].shape == (5, 5, 10)
    assert res["n_per_type"].dtype == np.int64 and res["celltypes"] == cats
    np.testing.assert_array_equal(res["count"], count)
    op = ad.uns["spatialcore_metadata"]["operations"][-1]
    assert op["function"] == "co_occurrence" and op["parameters"]["cluster_key"] == "cell_type"
    assert op["parameters"]["interval"] == 10 and op["outputs"]["uns"] == KEY
    assert op["outputs"]["n_pairs"] == int(count.sum()) and op["outputs"]["n_intervals"] == 9
    # copy=True: the pair, and nothing written
    ad2 = make_adata(coords, np.zeros((1200, 1)), labels=labels)
    pair = co_occurrence(ad2, "cell_type", interval=10, copy=True)
    assert isinstance(pair, tuple) and len(pair) == 2 and ad2.uns == {}
    np.testing.assert_array_equal(pair[0], res["occ"])
    np.testing.assert_array_equal(pair[1], thr)
    # a categorical column with reordered categories: the table follows the categories' order
    reordered = ["D", "A", "E", "C", "B"]
    ad3 = make_adata(coords, np.zeros((1200, 1)), labels=pd.Categorical(labels, categories=reordered))
    co_occurrence(ad3, "cell_type", interval=10)
    res3 = ad3.uns[KEY]
    assert res3["celltypes"] == reordered
    ix = [cats.index(v) for v in reordered]
    np.testing.assert_array_equal(res3["count"], count[np.ix_(ix, ix)])
    np.testing.assert_array_equal(res3["n_per_type"], np.bincount(codes, minlength=5)[ix])
    np.testing.assert_allclose(res3["occ"], occ(count)[np.ix_(ix, ix)], rtol=1e-6, equal_nan=True)
