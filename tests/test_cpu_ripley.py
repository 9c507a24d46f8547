"""Ripley's K without a device: the yardstick is pinned (brute force == scipy's exact tree counts), the host
arithmetic of K / L / p-values is checked on a hand-made table, and every validation error is raised before any
device work (this suite runs on a machine without a GPU)."""
import numpy as np
import pandas as pd
import pytest

from conftest import make_adata
from ripley_restated import brute_counts, scipy_counts


def test_restated_brute_force_equals_scipy_on_uniform_points():
    rng = np.random.default_rng(7)
    n, T = 20000, 5
    coords = rng.uniform(0, 1000.0, (n, 2))
    codes = rng.integers(0, T, n)
    radii = [3.0, 6.0, 9.5, 14.0, 20.0, 27.5]
    got, want = brute_counts(coords, codes, T, radii), scipy_counts(coords, codes, T, radii)
    assert got[:, :, -1].sum() > 10 * n          # (the radii are not trivially small)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, got.transpose(1, 0, 2))


def test_restated_brute_force_equals_scipy_on_a_lattice_with_tie_radii():
    """100 x 100 integer lattice; 5, 5 sqrt 2, 10, 15, 25 are distances that occur exactly (3-4-5, 5-5, 6-8-10, ...):
    the closed ball counts them, and fl(r r) of 5 sqrt 2 decides which side 50 falls on in both codes alike."""
    g = np.arange(100, dtype=np.float64)
    coords = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    rng = np.random.default_rng(3)
    T = 4
    codes = rng.integers(0, T, coords.shape[0])
    radii = [5.0, 5.0 * np.sqrt(2.0), 10.0, 15.0, 25.0]
    got, want = brute_counts(coords, codes, T, radii), scipy_counts(coords, codes, T, radii)
    np.testing.assert_array_equal(got, want)
    # an interior lattice point has 80 others within 5 (closed): the (0,5), (3,4) ties are in
    interior = coords[(coords >= 30).all(axis=1) & (coords <= 69).all(axis=1)][:1]
    d2 = ((coords - interior) ** 2).sum(axis=1)
    assert (d2 <= 25).sum() - 1 == 80


def test_k_l_and_p_values_from_a_hand_made_table():
    from spatialcore_amd.spatial.neighborhoods import ripley_statistics

    # three types: 4 cells, 1 cell (diagonal denominator 0), 0 cells (absent category)
    n_t = np.array([4, 1, 0])
    count = np.zeros((3, 3, 2), dtype=np.int64)
    count[0, 0] = [6, 12]
    count[0, 1] = count[1, 0] = [1, 4]
    area = 50.0
    out = ripley_statistics(count, n_t, area)
    np.testing.assert_allclose(out["K"][0, 0], [50.0 * 6 / 12, 50.0 * 12 / 12])
    np.testing.assert_allclose(out["K"][0, 1], [50.0 * 1 / 4, 50.0 * 4 / 4])
    np.testing.assert_array_equal(out["K"][0, 1], out["K"][1, 0])
    assert np.isnan(out["K"][1, 1]).all()            # a single cell: n (n - 1) = 0
    assert np.isnan(out["K"][2]).all() and np.isnan(out["K"][:, 2]).all()
    np.testing.assert_allclose(out["L"][0, 0], np.sqrt(out["K"][0, 0] / np.pi))
    assert "p_value" not in out
    # P = 4 null tables for entry (0, 0, 0): 4, 6, 8, 9 against the observed 6
    null = np.array([4, 6, 8, 9])
    dev = null - 6
    sums = np.zeros((4, 3, 3, 2), dtype=np.int64)
    sums[:, 0, 0, 0] = [dev.sum(), (dev * dev).sum(), (dev >= 0).sum(), (dev <= 0).sum()]
    sums[2:] = np.where(sums[2:] == 0, 4, sums[2:])  # every other entry: null == observed in all 4
    out = ripley_statistics(count, n_t, area, sums, 4)
    assert out["mean"][0, 0, 0] == null.mean()
    np.testing.assert_allclose(out["std"][0, 0, 0], null.std(), rtol=1e-12)
    np.testing.assert_allclose(out["zscore"][0, 0, 0], (6 - null.mean()) / null.std(), rtol=1e-12)
    assert out["p_value"][0, 0, 0] == (3 + 1) / 5
    assert out["p_value_less"][0, 0, 0] == (2 + 1) / 5
    assert out["p_value"][0, 1, 1] == 1.0 and out["p_value_less"][0, 1, 1] == 1.0
    assert out["mean"][0, 1, 1] == 4 and out["std"][0, 1, 1] == 0


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"validation must not touch the device (Context.{name})")


@pytest.fixture
def no_device(monkeypatch):
    from spatialcore_amd import _lib

    monkeypatch.setattr(_lib, "default_context", lambda device=0: _NoDevice())


def _adata(n=50, ndim=2):
    rng = np.random.default_rng(0)
    ad = make_adata(rng.uniform(0, 10, (n, ndim)), np.zeros((n, 1)), labels=rng.choice(["A", "B"], n))
    return ad


@pytest.mark.parametrize("kwargs, match", [
    (dict(celltype_column="nope"), "Column 'nope' not found"),
    (dict(spatial_key="nope"), r"adata.obsm\['nope'\] not found"),
    (dict(radii=[[1.0, 2.0]]), r"radii must be 1-D, got shape \(1, 2\)"),
    (dict(radii=[]), "radii must not be empty"),
    (dict(radii=[1.0, 3.0, 3.0]), "strictly increasing, got 3.0 after 3.0"),
    (dict(radii=[2.0, 1.0]), "strictly increasing, got 1.0 after 2.0"),
    (dict(radii=[0.0, 1.0]), "radii must be > 0, got 0.0"),
    (dict(radii=[-1.0, 1.0]), "radii must be > 0, got -1.0"),
    (dict(radii=[1.0, np.inf]), "radii must be finite, got inf"),
    (dict(radii=[1.0, np.nan]), "radii must be finite, got nan"),
    (dict(radii=np.arange(1, 34)), "at most 32 radii are supported, got 33"),
    (dict(n_permutations=-1), "n_permutations must be >= 0, got -1"),
    (dict(rng="mt19937"), "rng must be 'numpy' or 'philox', got 'mt19937'"),
    (dict(comm=object(), rng="numpy"), "rng='philox'"),
    (dict(area=0.0), "area must be > 0, got 0.0"),
    (dict(area=-2.0), "area must be > 0, got -2.0"),
])
def test_every_validation_error_is_raised_without_a_device(no_device, kwargs, match):
    from spatialcore_amd.spatial import ripley_k

    args = dict(celltype_column="cell_type", radii=[1.0, 2.0])
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        ripley_k(_adata(), **args)


def test_non_2d_coordinates_are_refused_without_a_device(no_device):
    from spatialcore_amd.spatial import ripley_k

    with pytest.raises(ValueError, match=r"only 2-D coordinates.*\(50, 3\)"):
        ripley_k(_adata(ndim=3), "cell_type", [1.0])


def test_missing_labels_are_refused_without_a_device(no_device):
    from spatialcore_amd.spatial import ripley_k

    ad = _adata()
    ad.obs["cell_type"] = pd.Series(ad.obs["cell_type"].values, index=ad.obs.index, dtype=object)
    ad.obs.iloc[3, ad.obs.columns.get_loc("cell_type")] = None
    with pytest.raises(ValueError, match="1 cells have missing labels"):
        ripley_k(ad, "cell_type", [1.0])


def test_the_native_entry_points_validate_on_the_host():
    """Null pointers and bad radii are refused by the library before it touches a device (no context is needed to
    see that: a null context is itself the first refusal)."""
    from spatialcore_amd import _lib

    lib = _lib.load_library()
    for name in ("sc_ripley_build", "sc_ripley_counts", "sc_ripley_counter"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = np.zeros(1, dtype=np.int64)
    xy = np.zeros((2, 2))
    r = np.array([1.0])
    assert lib.sc_ripley_build(None, xy.ctypes.data, 2, r.ctypes.data, 1, out.ctypes.data) != 0
    lab = np.zeros(2, dtype=np.int32)
    assert lib.sc_ripley_counts(None, lab.ctypes.data, 2, 1, 0, 0, out.ctypes.data) != 0
    assert lib.sc_ripley_counter(None, lab.ctypes.data, 2, 1, 0, 0, 0, 1, out.ctypes.data, out.ctypes.data) != 0
    assert b"null pointer" in lib.sc_last_error()
