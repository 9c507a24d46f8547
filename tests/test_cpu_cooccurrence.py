"""Co-occurrence without a device: the yardstick is pinned (the numpy restatement's cumulative totals == scipy's exact
tree counts), the ratio's host arithmetic is checked on its identities, and every validation error is raised before any
device work (this suite runs on a machine without a GPU)."""
import numpy as np
import pandas as pd
import pytest

from conftest import make_adata
from cooccurrence_restated import brute_counts, occ, thresholds


def test_restated_cumulative_totals_equal_scipy_tree_counts():
    from scipy.spatial import cKDTree

    rng = np.random.default_rng(7)
    n, T = 3000, 5
    coords = rng.uniform(0, 550.0, (n, 2))          # tie-free
    codes = rng.integers(0, T, n)
    thr = thresholds(coords, 50)
    assert thr.shape == (50,) and thr.dtype == np.float64 and (np.diff(thr) > 0).all() and thr[0] > 0
    count, dropped = brute_counts(coords, codes, T, thr)
    assert count.shape == (T, T, 50) and count.dtype == np.int64
    assert count.sum() + dropped == n * (n - 1)
    tree = cKDTree(coords)
    want = np.asarray(tree.count_neighbors(tree, thr), dtype=np.int64) - n     # cumulative, closed balls, self pairs removed
    np.testing.assert_array_equal(np.cumsum(count.sum(axis=(0, 1))), want)
    np.testing.assert_array_equal(count, count.transpose(1, 0, 2))
    # per type pair as well: the type-a tree against the type-b tree
    for a, b in ((0, 0), (1, 3), (4, 2)):
        ta, tb = cKDTree(coords[codes == a]), cKDTree(coords[codes == b])
        c = np.asarray(ta.count_neighbors(tb, thr), dtype=np.int64) - (int((codes == a).sum()) if a == b else 0)
        np.testing.assert_array_equal(np.cumsum(count[a, b]), c)


def test_threshold_rule_is_stable_on_ties_and_matches_the_package():
    from spatialcore_amd.spatial.neighborhoods import co_occurrence_thresholds

    # cells 1 and 3 tie for the smallest x + y, cells 2 and 4 for the largest: the lowest index wins each time
    coords = np.array([[5.0, 5.0], [1.0, 2.0], [9.0, 8.0], [2.0, 1.0], [8.0, 9.0], [1.5, 2.5]])
    thr = thresholds(coords, 4)
    np.testing.assert_array_equal(thr, np.linspace(np.sqrt(2.0), np.sqrt(64.0 + 36.0) / 2, 4))
    np.testing.assert_array_equal(co_occurrence_thresholds(coords, 4), thr)
    rng = np.random.default_rng(3)
    xy = rng.uniform(0, 100, (500, 2))
    np.testing.assert_array_equal(co_occurrence_thresholds(xy, 50), thresholds(xy, 50))
    np.testing.assert_array_equal(co_occurrence_thresholds(xy, [9.0, 1.0, 4.0]), [1.0, 4.0, 9.0])
    with pytest.raises(ValueError, match=r"not strictly increasing: t_min = 0\.0, t_max = 0\.0"):
        co_occurrence_thresholds(np.zeros((5, 2)), 10)       # every cell on one spot: a and c coincide


def test_occ_is_symmetric_one_for_a_single_type_and_nan_for_an_unused_type():
    from spatialcore_amd.spatial.neighborhoods import co_occurrence_ratio

    rng = np.random.default_rng(11)
    coords = rng.uniform(0, 100.0, (800, 2))
    codes = rng.integers(0, 3, 800)
    thr = np.linspace(2.0, 40.0, 9)
    count, _ = brute_counts(coords, codes, 4, thr)                  # type 3 has no cell
    ratio = occ(count)
    assert ratio.shape == (4, 4, 8) and ratio.dtype == np.float32
    np.testing.assert_array_equal(ratio, ratio.transpose(1, 0, 2))
    assert np.isnan(ratio[3]).all() and np.isnan(ratio[:, 3]).all() and np.isfinite(ratio[:3, :3]).all()
    got = co_occurrence_ratio(count)
    assert got.dtype == np.float32 and got.shape == ratio.shape
    np.testing.assert_allclose(got, ratio, rtol=1e-6)
    # the formula, entry by entry, on one annulus
    co = count[:, :, 4].astype(np.float64)
    np.testing.assert_allclose(ratio[0, 1, 3], co[0, 1] * co.sum() / (co[0].sum() * co[:, 1].sum()), rtol=1e-6)
    one, _ = brute_counts(coords, np.zeros(800, dtype=int), 1, thr)
    np.testing.assert_array_equal(occ(one), np.ones((1, 1, 8), dtype=np.float32))
    np.testing.assert_array_equal(co_occurrence_ratio(one), np.ones((1, 1, 8), dtype=np.float32))


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"validation must not touch the device (Context.{name})")


@pytest.fixture
def no_device(monkeypatch):
    from spatialcore_amd import _lib

    monkeypatch.setattr(_lib, "default_context", lambda device=0: _NoDevice())


def _adata(n=50, ndim=2):
    rng = np.random.default_rng(0)
    return make_adata(rng.uniform(0, 10, (n, ndim)), np.zeros((n, 1)), labels=rng.choice(["A", "B"], n))


@pytest.mark.parametrize("kwargs, match", [
    (dict(cluster_key="nope"), "Column 'nope' not found"),
    (dict(spatial_key="nope"), r"adata.obsm\['nope'\] not found"),
    (dict(interval=1), "interval must give 2 to 128 thresholds, got 1"),
    (dict(interval=0), "interval must give 2 to 128 thresholds, got 0"),
    (dict(interval=129), "interval must give 2 to 128 thresholds, got 129"),
    (dict(interval=True), "interval must be an integer or a 1-D sequence"),
    (dict(interval="many"), "interval must be an integer or a 1-D sequence"),
    (dict(interval=[[1.0, 2.0]]), r"1-D sequence of thresholds, got shape \(1, 2\)"),
    (dict(interval=[1.0]), "interval must give 2 to 128 thresholds, got 1"),
    (dict(interval=np.arange(129.0)), "interval must give 2 to 128 thresholds, got 129"),
    (dict(interval=[1.0, 3.0, 3.0]), "strictly increasing, got 3.0 after 3.0"),
    (dict(interval=[-1.0, 1.0]), "interval must be non-negative, got -1.0"),
    (dict(interval=[1.0, np.inf]), "interval must be finite, got inf"),
    (dict(interval=[1.0, np.nan]), "interval must be finite, got nan"),
    (dict(interval=[1.0, 1e200]), "finite square, got 1e\\+200"),
])
def test_every_validation_error_is_raised_without_a_device(no_device, kwargs, match):
    from spatialcore_amd.spatial import co_occurrence

    args = dict(cluster_key="cell_type", interval=[1.0, 2.0])
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        co_occurrence(_adata(), **args)


def test_non_2d_coordinates_are_refused_without_a_device(no_device):
    from spatialcore_amd.spatial import co_occurrence

    with pytest.raises(ValueError, match=r"only 2-D coordinates.*\(50, 3\)"):
        co_occurrence(_adata(ndim=3), "cell_type")


def test_missing_labels_are_refused_without_a_device(no_device):
    from spatialcore_amd.spatial import co_occurrence

    ad = _adata()
    ad.obs["cell_type"] = pd.Series(ad.obs["cell_type"].values, index=ad.obs.index, dtype=object)
    ad.obs.iloc[3, ad.obs.columns.get_loc("cell_type")] = None
    with pytest.raises(ValueError, match="1 cells have missing labels"):
        co_occurrence(ad, "cell_type")
    ad.obs["cell_type"] = pd.Categorical(ad.obs["cell_type"])          # a categorical's missing code is -1
    with pytest.raises(ValueError, match="1 cells have missing labels"):
        co_occurrence(ad, "cell_type")


def test_thresholds_that_collapse_are_refused_without_a_device(no_device):
    from spatialcore_amd.spatial import co_occurrence

    ad = make_adata(np.ones((20, 2)), np.zeros((20, 1)), labels=np.array(["A", "B"] * 10))
    with pytest.raises(ValueError, match=r"t_min = 0\.0, t_max = 0\.0"):
        co_occurrence(ad, "cell_type", interval=10)


def test_the_name_is_exported_directly_after_ripley_k():
    from spatialcore_amd import _lib, spatial

    assert spatial.__all__.index("co_occurrence") == spatial.__all__.index("ripley_k") + 1
    assert spatial.__all__[-1] == "rank_genes_groups"
    assert callable(spatial.co_occurrence)
    assert "sc_cooccurrence_2d" in _lib.SYMBOLS and hasattr(_lib.Context, "cooccurrence_counts")
    assert _lib.K_COOCCUR == 17


def test_the_native_entry_point_validates_on_the_host():
    """Every refusal comes from the host, before a device is touched: a null context is the first one, and with a
    dummy non-null handle the argument checks are reached in the order the header lists them."""
    import ctypes

    from spatialcore_amd import _lib

    lib = _lib.load_library()
    xy = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]])
    off = np.array([0, 2, 3], dtype=np.int64)
    thr = np.array([0.5, 1.0, 2.0])
    out = np.zeros(2 * 2 * 3, dtype=np.int64)

    def call(ctx, xy=xy, off=off, T=2, thr=thr, n_thr=None):
        rc = lib.sc_cooccurrence_2d(ctx, None if xy is None else xy.ctypes.data, off.ctypes.data, T, thr.ctypes.data,
                                    thr.size if n_thr is None else n_thr, out.ctypes.data)
        return rc, lib.sc_last_error().decode()

    rc, msg = call(None)
    assert rc == _lib.SC_ERR_INVALID and "null pointer" in msg
    dummy = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))   # never dereferenced before the checks pass
    for kw, want in [
        (dict(xy=None), "null pointer"),
        (dict(T=0), "n_types=0 out of range"),
        (dict(T=65536), "n_types=65536 out of range"),
        (dict(off=np.array([1, 2, 3], dtype=np.int64)), "offsets must start at 0"),
        (dict(off=np.array([0, 3, 2], dtype=np.int64)), "offsets not monotone"),
        (dict(n_thr=1), "n_thresholds=1 out of range"),
        (dict(thr=np.arange(1.0, 130.0)), "n_thresholds=129 out of range"),
        (dict(thr=np.array([1.0, np.inf])), "not finite"),
        (dict(thr=np.array([1.0, 1e200])), "no finite square"),
        (dict(thr=np.array([-1.0, 1.0])), "is negative"),
        (dict(thr=np.array([1.0, 1.0])), "strictly increasing, got 1 after 1"),
        (dict(xy=np.array([[0.0, 0.0], [1.0, np.nan], [2.0, 2.0]])), "point coordinate 1 is not finite"),
    ]:
        rc, msg = call(dummy, **kw)
        assert rc == _lib.SC_ERR_INVALID and want in msg, (kw, msg)
