"""Ripley's G without a device: the yardstick is pinned (brute force == scipy's nearest-neighbour queries), the host
arithmetic of G / G_poisson / p-values is checked on a hand-made table, and every validation error is raised before
any device work (this suite runs on a machine without a GPU)."""
import numpy as np
import pandas as pd
import pytest

from conftest import make_adata
from ripley_g_restated import brute_counts_g, scipy_counts_g


def test_restated_brute_force_equals_scipy_on_uniform_points():
    rng = np.random.default_rng(7)
    n, T = 8000, 5
    coords = rng.uniform(0, 632.0, (n, 2))                 # the density of test_cpu_ripley's 20 000 points in 1000 x 1000
    codes = rng.integers(0, T, n)
    radii = [3.0, 6.0, 9.5, 14.0, 20.0, 27.5]
    got, want = brute_counts_g(coords, codes, T, radii), scipy_counts_g(coords, codes, T, radii)
    n_t = np.bincount(codes, minlength=T)
    assert (got[:, :, 0] > 0).all() and (got[:, :, 0] < n_t[:, None]).all()     # (neither empty nor saturated at r_1)
    assert (got <= n_t[:, None, None]).all() and (np.diff(got, axis=2) >= 0).all()
    np.testing.assert_array_equal(got, want)
    assert (got != got.transpose(1, 0, 2)).any()           # not symmetric


def test_restated_brute_force_equals_scipy_on_a_lattice_with_tie_radii():
    """100 x 100 integer lattice; 1, sqrt 2, 2, sqrt 5, 3 are distances that occur exactly: the closed ball counts them,
    and fl(r r) of sqrt 2 and sqrt 5 decides which side 2 and 5 fall on in both codes alike."""
    g = np.arange(100, dtype=np.float64)
    coords = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    T = 4
    codes = np.random.default_rng(3).integers(0, T, coords.shape[0])
    radii = [1.0, np.sqrt(2.0), 2.0, np.sqrt(5.0), 3.0]
    got, want = brute_counts_g(coords, codes, T, radii), scipy_counts_g(coords, codes, T, radii)
    np.testing.assert_array_equal(got, want)
    assert (np.diff(got, axis=2) > 0).all()                # every radius adds first contacts: none of the ties is idle


def test_g_poisson_curve_and_p_values_from_a_hand_made_table():
    from spatialcore_amd.spatial.neighborhoods import ripley_g_statistics

    # three types: 4 cells, 1 cell (it has no other cell of its own type), 0 cells (absent category)
    n_t = np.array([4, 1, 0])
    count = np.zeros((3, 3, 2), dtype=np.int64)
    count[0, 0] = [2, 4]
    count[0, 1] = [1, 3]
    count[1, 0] = [0, 1]
    area, radii = 50.0, [1.0, 2.0]
    out = ripley_g_statistics(count, n_t, area, radii=radii)
    np.testing.assert_array_equal(out["G"][0, 0], [0.5, 1.0])
    np.testing.assert_array_equal(out["G"][0, 1], [0.25, 0.75])
    np.testing.assert_array_equal(out["G"][1, 0], [0.0, 1.0])
    np.testing.assert_array_equal(out["G"][1, 1], [0.0, 0.0])      # a single cell: defined, and never met
    np.testing.assert_array_equal(out["G"][0, 2], [0.0, 0.0])      # nothing of an absent type is ever met ...
    assert np.isnan(out["G"][2]).all()                             # ... and G of an absent type is undefined: n_a = 0
    r2 = np.array([1.0, 4.0])
    np.testing.assert_allclose(out["G_poisson"][0, 1], 1 - np.exp(-(1 / 50.0) * np.pi * r2), rtol=1e-15)   # lambda = n_b / area
    np.testing.assert_allclose(out["G_poisson"][1, 0], 1 - np.exp(-(4 / 50.0) * np.pi * r2), rtol=1e-15)
    np.testing.assert_allclose(out["G_poisson"][0, 0], 1 - np.exp(-(3 / 50.0) * np.pi * r2), rtol=1e-15)   # (n_a - 1) / area
    np.testing.assert_array_equal(out["G_poisson"][1, 1], [0.0, 0.0])
    np.testing.assert_array_equal(out["G_poisson"][:, 2], np.zeros((3, 2)))
    assert "p_value" not in out and "G_poisson" not in ripley_g_statistics(count, n_t, area)
    # P = 4 null tables for entry (0, 1, 0): 0, 1, 2, 3 against the observed 1
    null = np.array([0, 1, 2, 3])
    dev = null - 1
    sums = np.zeros((4, 3, 3, 2), dtype=np.int64)
    sums[:, 0, 1, 0] = [dev.sum(), (dev * dev).sum(), (dev >= 0).sum(), (dev <= 0).sum()]
    sums[2:] = np.where(sums[2:] == 0, 4, sums[2:])                # every other entry: null == observed in all 4
    out = ripley_g_statistics(count, n_t, area, sums, 4, radii=radii)
    assert out["mean"][0, 1, 0] == null.mean()
    np.testing.assert_allclose(out["std"][0, 1, 0], null.std(), rtol=1e-12)
    np.testing.assert_allclose(out["zscore"][0, 1, 0], (1 - null.mean()) / null.std(), rtol=1e-12)
    assert out["p_value"][0, 1, 0] == (3 + 1) / 5
    assert out["p_value_less"][0, 1, 0] == (2 + 1) / 5
    assert out["p_value"][0, 0, 1] == 1.0 and out["p_value_less"][0, 0, 1] == 1.0
    assert out["mean"][0, 0, 1] == 4 and out["std"][0, 0, 1] == 0


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
    (dict(celltype_column="nope"), "Column 'nope' not found"),
    (dict(spatial_key="nope"), r"adata.obsm\['nope'\] not found.*required for Ripley's G"),
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
    from spatialcore_amd.spatial import ripley_g

    args = dict(celltype_column="cell_type", radii=[1.0, 2.0])
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        ripley_g(_adata(), **args)


def test_non_2d_coordinates_are_refused_without_a_device(no_device):
    from spatialcore_amd.spatial import ripley_g

    with pytest.raises(ValueError, match=r"only 2-D coordinates.*\(50, 3\)"):
        ripley_g(_adata(ndim=3), "cell_type", [1.0])


def test_missing_labels_are_refused_without_a_device(no_device):
    from spatialcore_amd.spatial import ripley_g

    ad = _adata()
    ad.obs["cell_type"] = pd.Series(ad.obs["cell_type"].values, index=ad.obs.index, dtype=object)
    ad.obs.iloc[3, ad.obs.columns.get_loc("cell_type")] = None
    with pytest.raises(ValueError, match="1 cells have missing labels"):
        ripley_g(ad, "cell_type", [1.0])


def test_the_native_entry_points_validate_on_the_host():
    """Null pointers are refused by the library before it touches a device (no context is needed to see that: a null
    context is itself the first refusal)."""
    from spatialcore_amd import _lib

    lib = _lib.load_library()
    for name in ("sc_ripley_g_build", "sc_ripley_g_counts", "sc_ripley_g_counter"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = np.zeros(1, dtype=np.int64)
    xy = np.zeros((2, 2))
    r = np.array([1.0])
    lab = np.zeros(2, dtype=np.int32)
    assert lib.sc_ripley_g_build(None, xy.ctypes.data, 2, r.ctypes.data, 1, out.ctypes.data) != 0
    assert b"sc_ripley_g_build: null pointer" in lib.sc_last_error()
    assert lib.sc_ripley_g_counts(None, lab.ctypes.data, 2, 1, 0, 0, out.ctypes.data) != 0
    assert b"sc_ripley_g_counts: null pointer" in lib.sc_last_error()
    assert lib.sc_ripley_g_counter(None, lab.ctypes.data, 2, 1, 0, 0, 0, 1, out.ctypes.data, out.ctypes.data) != 0
    assert b"sc_ripley_g_counter: null pointer" in lib.sc_last_error()
    assert (_lib.K_RIPLEY_G_LIST, _lib.K_RIPLEY_G_RELABEL, _lib.K_RIPLEY_G_COUNT) == (19, 20, 21)


def test_the_name_is_exported_after_ligrec_and_the_pinned_positions_hold():
    from spatialcore_amd import spatial

    assert callable(spatial.ripley_g)
    assert spatial.__all__.index("ripley_g") == spatial.__all__.index("ligrec") + 1
    assert spatial.__all__.index("co_occurrence") == spatial.__all__.index("ripley_k") + 1
    assert spatial.__all__[-1] == "rank_genes_groups"
