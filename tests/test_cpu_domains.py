"""make_spatial_domains / get_domain_summary without a device: the yardstick is pinned (the restated clearance against
a dense sampling of the boundary), every validation error is raised before the library is asked for anything, and
the host pieces -- filter expressions, platform detection, prefix generation, the summary -- are checked against
hand-made inputs (this suite runs on a machine without a GPU)."""
import logging

import numpy as np
import pandas as pd
import pytest

from conftest import make_adata
from domains_restated import (assign, boundary_sample_clearance, clearance, components, make_input,
                              reduce_and_number)


# ---- the restatement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, n_targets, n_components", [("A", 294, 63), ("B", 448, 8), ("C", 448, 111)])
def test_restated_clearance_agrees_with_boundary_sampling(name, n_targets, n_components):
    """The candidate formula (foot points + circle intersections, each kept only if no other disc holds it) against
    4000 sampled points per circle.  The nearest kept sample is never closer than the true boundary and at most one
    arc spacing farther: the bound is pi d / nang times 2."""
    xy, target, d, m = make_input(name)
    s, nang = d - m, 4000
    T = xy[target]
    assert T.shape[0] == n_targets
    comp = components(T, d)
    assert np.unique(comp).size == n_components
    np.testing.assert_array_equal(comp[np.unique(comp)], np.unique(comp))       # an id is a member of its component
    assert (comp <= np.arange(T.shape[0])).all()                                 # ... and the smallest
    got = clearance(T, xy, d, s)
    want = boundary_sample_clearance(T, xy, d, s, nang)
    np.testing.assert_array_equal(got < 0, want < 0)
    err = np.abs(got - want).max()
    print(f"input {name}: max |formula - sampling| = {err:.4f}, bound {2 * np.pi * d / nang:.4f}")
    assert err <= 2 * np.pi * d / nang
    assert (got[target] == s).all()                                              # every target is in its own region


def test_restated_counts_of_input_a():
    xy, target, d, m = make_input("A")
    comp_t, comp_q, clear = assign(xy[target], xy[~target], d, d - m)
    sizes = np.bincount(comp_t)[np.unique(comp_t)]
    assert (sizes <= 10).sum() == 55
    assert (comp_q >= 0).sum() == 237
    assert ((clear >= 0) & (clear < d - m)).sum() == 581
    rank_t, rank_q = reduce_and_number(comp_t, comp_q, 10)
    assert rank_t.max() == 8 and set(np.unique(rank_q)) <= set(range(9))
    total = np.bincount(np.concatenate([rank_t, rank_q]))[1:]
    assert (np.diff(total) <= 0).all()                                           # largest first


def test_reduce_and_number_by_hand():
    # components 0 (3 targets + 2 others), 1 (2 targets + 3 others), 4 (2 targets), 6 (1 target + 4 others)
    comp_t = np.array([0, 1, 0, 1, 4, 4, 6, 0])
    comp_q = np.array([0, 0, 1, 1, 1, -1, 6, 6, 6, 6])
    rt, rq = reduce_and_number(comp_t, comp_q, 1)          # component 6 has exactly 1 target: dropped (<=)
    np.testing.assert_array_equal(rt, [1, 2, 1, 2, 3, 3, 0, 1])     # 5, 5, 2 cells: the tie goes to the smaller id
    np.testing.assert_array_equal(rq, [1, 1, 2, 2, 2, 0, 0, 0, 0, 0])
    rt, rq = reduce_and_number(comp_t, comp_q, 0, min_total=2)      # component 4 has exactly 2 cells: dropped (<=)
    np.testing.assert_array_equal(rt, [1, 2, 1, 2, 0, 0, 3, 1])
    np.testing.assert_array_equal(rq, [1, 1, 2, 2, 2, 0, 3, 3, 3, 3])
    from spatialcore_amd.spatial.domains import _number_domains

    for args in ((1, None), (0, 2), (2, 4)):
        want = reduce_and_number(comp_t, comp_q, *args)
        got = _number_domains(comp_t, comp_q, *args)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


# ---- validation: nothing below may load the library ------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    from spatialcore_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("validation must not load the library or touch the device")

    monkeypatch.setattr(_lib, "default_context", refuse)
    monkeypatch.setattr(_lib, "load_library", refuse)


def _adata(n=60, ndim=2, scale=100.0):
    rng = np.random.default_rng(0)
    ad = make_adata(rng.uniform(0, scale, (n, ndim)), np.zeros((n, 1)), labels=np.where(np.arange(n) % 3 == 0, "T", "S"))
    ad.obs["cluster"] = (np.arange(n) % 4).astype(np.int64)
    ad.obs["is_tumor"] = np.arange(n) % 2 == 0
    ad.obs["flag_text"] = pd.Series(np.where(np.arange(n) % 5 == 0, "True", "False"), index=ad.obs.index, dtype=object)
    return ad


@pytest.mark.parametrize("kwargs, match", [
    (dict(filter_expression=None), "'filter_expression' must be provided"),
    (dict(platform="merfish"), r"Unknown platform 'merfish'. Valid platforms are: \['cosmx', 'xenium', 'visium'\]"),
    (dict(cell_dist_um=0.0), "cell_dist_um must be finite and > 0, got 0.0"),
    (dict(cell_dist_um=-3.0), "cell_dist_um must be finite and > 0, got -3.0"),
    (dict(cell_dist_um=np.inf), "cell_dist_um must be finite and > 0, got inf"),
    (dict(cell_dist_um=10.0, shrink_margin_um=0.0), "0 < shrink_margin_um <= cell_dist_um, got 0.0 with cell_dist_um=10.0"),
    (dict(cell_dist_um=10.0, shrink_margin_um=-1.0), "0 < shrink_margin_um <= cell_dist_um, got -1.0"),
    (dict(cell_dist_um=10.0, shrink_margin_um=10.5), "0 < shrink_margin_um <= cell_dist_um, got 10.5"),
    (dict(cell_dist_um=10.0, shrink_margin_um=25.0), "0 < shrink_margin_um <= cell_dist_um, got 25.0"),   # the default margin
    (dict(filter_expression="cell_type == 'nobody'"), "No cells match filter expression: 'cell_type == 'nobody''"),
    (dict(filter_expression="nope == 1"), "Column 'nope' not found in adata.obs"),
    (dict(filter_expression="cluster"), "Column 'cluster' exists but is not boolean"),
    (dict(filter_expression="cluster >>> 2"), "Could not evaluate filter expression: 'cluster >>> 2'"),
    (dict(assign_all_cells=False, min_target_cells_domain=20), "No cells were assigned to any domain"),
])
def test_every_validation_error_is_raised_without_the_library(no_library, kwargs, match):
    from spatialcore_amd.spatial import make_spatial_domains

    args = dict(filter_expression="cell_type == 'T'", cell_dist_um=30.0, shrink_margin_um=10.0)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        make_spatial_domains(_adata(), **args)


def test_missing_coordinates_undetectable_platform_and_bad_shapes(no_library):
    from spatialcore_amd.spatial import get_domain_summary, make_spatial_domains

    ad = _adata()
    del ad.obsm["spatial"]
    with pytest.raises(ValueError, match=r"adata.obsm\['spatial'\] not found. Spatial coordinates are required"):
        make_spatial_domains(ad, "cell_type == 'T'")
    with pytest.raises(ValueError, match=r"adata.obsm\['spatial'\] not found. Spatial coordinates are required"):
        make_spatial_domains(ad)                         # ... before the missing filter expression
    ad = _adata()
    ad.obsm["spatial"] = np.full((60, 2), np.nan)        # no threshold matches: the platform cannot be told
    with pytest.raises(ValueError, match="Could not auto-detect platform from coordinate ranges"):
        make_spatial_domains(ad, "cell_type == 'T'")
    with pytest.raises(ValueError, match=r"at least 2 columns, got shape \(60, 1\)"):
        make_spatial_domains(_adata(ndim=1), "cell_type == 'T'", cell_dist_um=30.0, shrink_margin_um=10.0)
    with pytest.raises(ValueError, match=r"only 2-D coordinates.*\(60, 3\)"):
        make_spatial_domains(_adata(ndim=3), "cell_type == 'T'", cell_dist_um=30.0, shrink_margin_um=10.0)
    with pytest.raises(NotImplementedError, match="CL:0000236 & is_tumor"):
        make_spatial_domains(_adata(), "CL:0000236 & is_tumor", cell_dist_um=30.0, shrink_margin_um=10.0)
    with pytest.raises(ValueError, match="Column 'spatial_domain' not found in adata.obs"):
        get_domain_summary(_adata())


def test_validation_leaves_the_input_untouched(no_library):
    from spatialcore_amd.spatial import make_spatial_domains

    ad = _adata()
    cols = list(ad.obs.columns)
    with pytest.raises(ValueError):
        make_spatial_domains(ad, "cell_type == 'nobody'", cell_dist_um=30.0, shrink_margin_um=10.0)
    assert list(ad.obs.columns) == cols and "_filter" not in ad.obs.columns


# ---- host pieces -------------------------------------------------------------------------------------------------------

def test_filter_expressions():
    from spatialcore_amd.spatial.domains import _evaluate_filter_expression as ev

    ad = _adata()
    i = np.arange(60)
    np.testing.assert_array_equal(np.asarray(ev("cell_type == 'T'", ad)), i % 3 == 0)
    np.testing.assert_array_equal(np.asarray(ev('cell_type == "T"', ad)), i % 3 == 0)
    np.testing.assert_array_equal(np.asarray(ev("cell_type == T", ad)), i % 3 == 0)
    np.testing.assert_array_equal(np.asarray(ev("  cell_type==T ", ad)), i % 3 == 0)
    # the unquoted value stays a string, as in the reference: an integer column equals no string
    assert not np.asarray(ev("cluster == 1", ad)).any()
    ad.obs["cluster_name"] = ad.obs["cluster"].astype(str)
    np.testing.assert_array_equal(np.asarray(ev("cluster_name == 1", ad)), i % 4 == 1)
    np.testing.assert_array_equal(np.asarray(ev("is_tumor", ad)), i % 2 == 0)
    got = ev("flag_text", ad)
    assert got.dtype == bool or set(got.unique()) <= {True, False}
    np.testing.assert_array_equal(np.asarray(got, dtype=bool), i % 5 == 0)
    np.testing.assert_array_equal(np.asarray(ev("(cluster >= 2) & is_tumor", ad)), (i % 4 >= 2) & (i % 2 == 0))
    np.testing.assert_array_equal(np.asarray(ev("is_tumor | (cell_type == 'T')", ad)), (i % 3 == 0) | (i % 2 == 0))
    with pytest.raises(ValueError, match="Column 'cluster' exists but is not boolean. Use equality syntax like \"cluster == 'value'\""):
        ev("cluster", ad)
    with pytest.raises(NotImplementedError, match="'CL:0000236'"):
        ev("CL:0000236", ad)


@pytest.mark.parametrize("max_coord, want", [(15000.0, "xenium"), (15000.5, "visium"), (50000.0, "visium"),
                                             (50000.5, "cosmx"), (120000.0, "cosmx"), (3.0, "xenium")])
def test_platform_detection_at_the_thresholds(max_coord, want):
    from spatialcore_amd.spatial.domains import PLATFORM_DEFAULTS, _detect_platform, _get_platform_defaults

    ad = _adata(scale=1.0)
    ad.obsm["spatial"][7, 1] = -max_coord              # the largest ABSOLUTE coordinate decides
    assert _detect_platform(ad) == want
    assert _get_platform_defaults(want.upper()) == PLATFORM_DEFAULTS[want]
    assert PLATFORM_DEFAULTS == {"cosmx": 400.0, "xenium": 50.0, "visium": 200.0}
    del ad.obsm["spatial"]
    assert _detect_platform(ad) is None


def test_prefix_generation():
    from spatialcore_amd.spatial.domains import _generate_domain_prefix as gen

    assert gen("CL:0000236") == "CL_0000236"
    assert gen("is_tumor & CL:0000236") == "CL_0000236"
    assert gen("cell_type == 'B cell'") == "B_cell"
    assert gen("metagene_cluster == 1") == "1"
    assert gen("is_tumor") == "is_tumor"
    assert gen("(cluster >= 2) & is_tumor_and_more") == "_cluster____2____is_"
    assert gen("") == "domain"


def test_domain_summary_by_hand():
    from spatialcore_amd.spatial import get_domain_summary

    xy = np.array([[0., 0.], [2., 0.], [4., 6.], [10., 10.], [20., 30.], [1., 1.], [7., 7.], [30., 10.]])
    ad = make_adata(xy, np.zeros((8, 1)))
    ad.obs["dom"] = pd.Series(["D_2", "D_1", "D_1", np.nan, "D_2", "D_1", None, "D_3"], index=ad.obs.index, dtype=object)
    df = get_domain_summary(ad, "dom")
    assert list(df.columns) == ["domain", "n_cells", "percent", "centroid_x", "centroid_y"]
    assert df["domain"].tolist() == ["D_1", "D_2", "D_3"]                  # by n_cells, largest first
    assert df["n_cells"].tolist() == [3, 2, 1]
    np.testing.assert_allclose(df["percent"].values, [37.5, 25.0, 12.5])    # of all 8 cells, the NaN rows included
    np.testing.assert_allclose(df["centroid_x"].values, [7. / 3., 10.0, 30.0])
    np.testing.assert_allclose(df["centroid_y"].values, [7. / 3., 15.0, 10.0])
    del ad.obsm["spatial"]
    with pytest.raises(ValueError, match=r"adata.obsm\['spatial'\] not found. Available keys: \[\]"):
        get_domain_summary(ad, "dom")


# ---- the native symbol ---------------------------------------------------------------------------------------------------

def test_the_native_entry_point_is_declared_exported_and_validates_on_the_host():
    import os

    from spatialcore_amd import _lib
    from spatialcore_amd import spatial

    assert spatial.__all__.index("make_spatial_domains") + 1 == spatial.__all__.index("get_domain_summary")
    assert spatial.__all__.index("get_domain_summary") < spatial.__all__.index("calculate_domain_distances")
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "spatialcore_hip.h")).read()
    assert "int sc_domains_2d(sc_ctx *ctx, const double *xy_targets, int64_t n_targets" in header
    lib = _lib.load_library()
    assert "sc_domains_2d" in _lib.SYMBOLS and hasattr(lib, "sc_domains_2d")
    xy = np.zeros((2, 2))
    out = np.zeros(2, dtype=np.int32)
    # a null context is the first refusal: no device is needed to see it
    assert lib.sc_domains_2d(None, xy.ctypes.data, 2, None, 0, 1.0, 0.5, out.ctypes.data, None, None) == _lib.SC_ERR_INVALID
    assert b"sc_domains_2d: null pointer" in lib.sc_last_error()
