"""spatialcore_amd.preprocessing without a GPU: the restatement of the device's order against the definition on every case,
the separation the selection test relies on, the ranking and batch rules on hand-made variances, every refusal that
happens before the device is reached, and the ctypes surface."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest
from scipy import sparse

import hvg_restated as R
from conftest import ROOT, make_adata

TOL = 1e-10     # tests/test_gpu_hvg.py: the device against textbook()


def _adata(X, **obs):
    ad = make_adata(np.zeros((X.shape[0], 2)), X.copy() if hasattr(X, "copy") else X)
    for k, v in obs.items():
        ad.obs[k] = v
    return ad


# ---- 1. the restatements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_ordered_against_textbook(case):
    """The split form in fp64 stays 100x below TOL and the same form in float32 100x above it, on every case."""
    _, _, n, G, _, theta, clip, _ = case
    X = R.matrix(case)
    want = R.textbook(X, theta, clip)
    got = R.ordered(X, theta, clip)
    e64, e32 = R.rel_err(got["var"], want), R.rel_err(R.ordered(X, theta, clip, dtype=np.float32)["var"], want)
    print(f"{case[0]}: ordered fp64 {e64:.2e}, float32 {e32:.2e}")
    assert e64 <= TOL / 100 and e32 >= TOL * 100
    assert np.all(got["var"][want == 0] == 0)
    A = X.toarray().astype(np.float64)
    assert R.rel_err(got["sum"], A.sum(axis=0)) <= 1e-14 and R.rel_err(got["sumsq"], (A * A).sum(axis=0)) <= 1e-14
    if case[1] != "real":
        s1, s2, _, _ = R.moments(X)
        np.testing.assert_array_equal(got["sum"], s1)
        np.testing.assert_array_equal(got["sumsq"], s2)


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_no_two_genes_sit_closer_than_the_tolerance(case):
    """What makes the device's selection comparable with the textbook's without exclusions."""
    gap = R.smallest_gap(R.textbook(R.matrix(case), case[5], case[6]))
    print(f"{case[0]}: smallest relative gap {gap:.2e}")
    assert gap >= 100 * TOL


def test_cases_hit_the_edges_they_name():
    by = {c[0]: c for c in R.CASES}
    for name in ("1023x255", "1024x256", "1025x257"):
        X = R.matrix(by[name])
        n, G = X.shape
        z, mu = R.raw_residuals(X)
        hit = np.argwhere(z > np.sqrt(n))
        assert hit.tolist() == [[int(np.flatnonzero(X[:, 1].toarray().ravel())[0]), 1]]      # +clip engages on the single count
        assert X[:, 0].nnz == n and X[:, G // 2].nnz == 0
    assert (1025 - 1) % R.COL_CHUNK == 0 and -(-1025 // R.COL_CHUNK) == 3                    # a last chunk of one entry
    assert [R.slice_rows(n) for n in (5, 1024, 1025, R.SLICE * R.MAX_SLICES, R.SLICE * R.MAX_SLICES + 1)] == [1024, 1024, 1024, 1024, 2048]
    for name in ("300x9-clip3", "777x37-clip3", "2000x200-clip3"):
        X = R.matrix(by[name])
        z, mu = R.raw_residuals(X)
        assert (z > 3).any() and (name == "300x9-clip3" or (z < -3).any())
        assert np.all(mu[z < -3] > 9)                                                        # -clip needs mu of about 10
    X = R.matrix(by["2049x40"])
    assert np.diff(X.indptr).min() == 0 and X[:, 20].nnz == 0                                # an empty cell and an empty gene
    assert R.matrix(by["777x37-f32-real"]).dtype == np.float32
    assert R.matrix(by["5x3"]).shape == (5, 3)
    # the constants are those of the sources
    hip = open(os.path.join(ROOT, "spatialcore_amd", "csrc", "sc_hvg.hip")).read()
    col = open(os.path.join(ROOT, "spatialcore_amd", "csrc", "sc_colsort.h")).read()
    assert f"HVG_SLICE = {R.SLICE};" in hip and f"HVG_MAX_SLICES = {R.MAX_SLICES};" in hip and f"HVG_BLK = {R.BLK};" in hip
    assert f"COL_CHUNK = {R.COL_CHUNK};" in col


def test_textbook_keeps_an_empty_cell_at_zero_and_counts_it():
    A = np.array([[3, 0, 1], [0, 0, 0], [1, 2, 0], [4, 1, 1]], dtype=np.float64)
    z, mu = R.raw_residuals(A)
    assert not z[1].any() and np.all(np.isfinite(z))
    got = R.textbook(A)
    B = np.delete(A, 1, axis=0)
    zb, _ = R.raw_residuals(B)
    # the other cells' residuals do not change; the variance runs over four cells, not three
    np.testing.assert_array_equal(z[[0, 2, 3]], zb)
    np.testing.assert_allclose(got, np.var(np.vstack([zb[:1], np.zeros((1, 3)), zb[1:]]), axis=0), rtol=1e-15)


# ---- 2. the ranking rules ------------------------------------------------------------------------------------------------------
def test_single_ranking_ties_and_all_genes():
    from spatialcore_amd.preprocessing import hvg

    var = np.array([2.0, 5.0, 2.0, 0.0, 7.0, 5.0, 0.0])
    np.testing.assert_array_equal(hvg.rank_by_variance(var), [3, 1, 4, 5, 0, 2, 6])
    np.testing.assert_array_equal(hvg.rank_by_variance(var), R.ranks(var))
    out = hvg.select_single(var, 3)
    np.testing.assert_array_equal(out["highly_variable"], [False, True, False, False, True, True, False])
    np.testing.assert_array_equal(out["highly_variable_rank"], [np.nan, 1, np.nan, np.nan, 0, 2, np.nan])
    assert out["highly_variable_rank"].dtype == np.float64 and out["highly_variable"].dtype == bool
    for n_top in (1, 4, 7, 8, 2000):
        out = hvg.select_single(var, n_top)
        hv, rk = R.select(var, n_top)
        np.testing.assert_array_equal(out["highly_variable"], hv)
        np.testing.assert_array_equal(out["highly_variable_rank"], rk)
        assert out["highly_variable"].sum() == min(n_top, 7)
    with pytest.raises(ValueError, match="finite"):
        hvg.rank_by_variance(np.array([1.0, np.nan]))
    rng = np.random.default_rng(0)
    var = rng.integers(0, 6, 60).astype(np.float64)          # many ties
    np.testing.assert_array_equal(hvg.rank_by_variance(var), R.ranks(var))


def test_batch_rule_by_hand():
    from spatialcore_amd.preprocessing import hvg

    #          g0   g1   g2   g3   g4   g5
    V = np.array([[9.0, 8.0, 7.0, 1.0, 2.0, 0.0],        # ranks 0 1 2 4 3 5
                  [1.0, 8.0, 9.0, 7.0, 0.0, 0.0],        # ranks 3 1 0 2 4 5
                  [9.0, 1.0, 8.0, 0.0, 7.0, 0.0]])       # ranks 0 3 1 5 2 4
    out = hvg.select_batches(V, 3)
    # ranks below 3: g0 {0, 0}, g1 {1, 1}, g2 {2, 0, 1}, g3 {2}, g4 {2}, g5 {}
    np.testing.assert_array_equal(out["highly_variable_nbatches"], [2, 2, 3, 1, 1, 0])
    np.testing.assert_array_equal(out["highly_variable_intersection"], [False, False, True, False, False, False])
    # medians 0, 1, 1, 2, 2, NaN: order g0, then g2 before g1 (3 batches against 2), then g3 before g4 (index)
    np.testing.assert_array_equal(out["highly_variable"], [True, True, True, False, False, False])
    np.testing.assert_array_equal(out["highly_variable_rank"], [0.0, 1.0, 1.0, np.nan, np.nan, np.nan])
    np.testing.assert_array_equal(out["residual_variances"], V.mean(axis=0))
    out4 = hvg.select_batches(V, 4)
    # ranks below 4: g0 {0, 3, 0} -> 0; g1 {1, 1, 3} -> 1; g2 {2, 0, 1} -> 1; g3 {2} -> 2; g4 {3, 2} -> 2.5; g5 {}
    np.testing.assert_array_equal(out4["highly_variable_rank"], [0.0, 1.0, 1.0, 2.0, np.nan, np.nan])
    np.testing.assert_array_equal(out4["highly_variable_nbatches"], [3, 3, 3, 1, 2, 0])
    everything = hvg.select_batches(V, 6)
    assert everything["highly_variable"].all() and everything["highly_variable_intersection"].all()
    assert not np.isnan(everything["highly_variable_rank"]).any()
    assert hvg.select_batches(V, 2000)["highly_variable"].all()
    one = hvg.select_batches(V[:1], 2)
    np.testing.assert_array_equal(one["highly_variable"], hvg.select_single(V[0], 2)["highly_variable"])
    np.testing.assert_array_equal(one["highly_variable_rank"], hvg.select_single(V[0], 2)["highly_variable_rank"])


@pytest.mark.parametrize("seed", range(6))
def test_batch_rule_against_the_restatement(seed):
    from spatialcore_amd.preprocessing import hvg

    rng = np.random.default_rng(seed)
    B, G = int(rng.integers(1, 5)), int(rng.integers(3, 40))
    V = rng.integers(0, 8, (B, G)).astype(np.float64)       # ties inside every batch
    for n_top in (1, 2, G // 2 + 1, G, G + 3):
        got, want = hvg.select_batches(V, n_top), R.select_batches(V, n_top)
        np.testing.assert_array_equal(got["highly_variable_nbatches"], want["nbatches"])
        np.testing.assert_array_equal(got["highly_variable_intersection"], want["intersection"])
        np.testing.assert_array_equal(got["highly_variable"], want["highly_variable"])
        np.testing.assert_array_equal(got["highly_variable_rank"], want["rank"])
        assert got["highly_variable"].sum() == min(n_top, G)


def test_moments_from_sums():
    from spatialcore_amd.preprocessing import hvg

    X = R.matrix(R.CASES[3])
    s1, s2, means, variances = R.moments(X)
    m, v = hvg.moments_from_sums(s1, s2, X.shape[0])
    np.testing.assert_array_equal(m, means)
    np.testing.assert_array_equal(v, variances)
    A = X.toarray()
    np.testing.assert_allclose(m, A.mean(axis=0), rtol=1e-14)
    np.testing.assert_allclose(v, A.var(axis=0, ddof=1), rtol=1e-11, atol=0)


# ---- 3. refusals before the device is reached --------------------------------------------------------------------------------
def test_argument_refusals_need_no_device():
    from spatialcore_amd.preprocessing import highly_variable_genes as hvg

    X = R.matrix(R.CASES[1])
    n, G = X.shape
    ad = _adata(X)
    for bad in ("seurat", "seurat_v3", "cell_ranger", None):
        with pytest.raises(ValueError, match="only flavor is 'pearson_residuals'"):
            hvg(ad, flavor=bad)
    for bad in (0, -3, 2.5, True, "10", None):
        with pytest.raises(ValueError, match="n_top_genes must be an integer >= 1"):
            hvg(ad, n_top_genes=bad)
    for bad in (0, -1.0, float("nan"), "100", None, True):
        with pytest.raises(ValueError, match="theta must be a number > 0"):
            hvg(ad, theta=bad)
    for bad in (0, -2.0, float("nan"), "3"):
        with pytest.raises(ValueError, match="clip must be a number > 0"):
            hvg(ad, clip=bad)
    with pytest.raises(ValueError, match="subset must be True or False"):
        hvg(ad, subset=1)
    with pytest.raises(ValueError, match="copy must be True or False"):
        hvg(ad, copy="yes")
    with pytest.raises(ValueError, match="layer='counts' is not in adata.layers"):
        hvg(ad, layer="counts")
    with pytest.raises(ValueError, match="batch_key='batch' is not a column"):
        hvg(ad, batch_key="batch")
    with pytest.raises(ValueError, match="batch 'c' .* has 1 cell; every batch needs at least 2"):
        hvg(_adata(X, batch=np.array(["a", "b"] * (n // 2 - 1) + ["a", "c"])), batch_key="batch")
    with pytest.raises(ValueError, match="has missing values"):
        hvg(_adata(X, batch=np.array([1.0, np.nan] * (n // 2))), batch_key="batch")
    zero_batch = X.tolil()
    zero_batch[:4] = 0
    with pytest.raises(ValueError, match="batch 'z' is all zero"):
        hvg(_adata(zero_batch.tocsr(), batch=np.array(["z"] * 4 + ["a"] * (n - 4))), batch_key="batch")
    neg = X.toarray()
    neg[3, 2] = -1
    with pytest.raises(ValueError, match="need raw counts; the expression matrix has negative entries"):
        hvg(_adata(neg))
    nan = X.toarray()
    nan[0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        hvg(_adata(nan))
    with pytest.raises(ValueError, match="all zero: there is nothing to rank"):
        hvg(_adata(sparse.csr_matrix((n, G), dtype=np.float64)))
    with pytest.raises(ValueError, match="needs 2 <= cells"):
        hvg(_adata(X[:1]))
    with pytest.raises(ValueError, match="at most 32768 genes"):
        hvg(_adata(sparse.csr_matrix((3, 32769), dtype=np.float32)))
    with pytest.raises(ValueError, match="must be real"):
        hvg(_adata(X.toarray().astype(np.complex128)))
    assert "means" not in ad.var and "hvg" not in ad.uns                    # nothing was written


def test_warnings_are_raised_before_the_device(caplog):
    """Non-integer values and empty cells are legal; each draws one warning, then the call goes on to the device (which
    this test does not need)."""
    from spatialcore_amd import _lib
    from spatialcore_amd.preprocessing import highly_variable_genes as hvg

    log = logging.getLogger("spatialcore_amd")
    log.addHandler(caplog.handler)
    try:
        hvg(_adata(R.matrix(R.CASES[5])))
    except _lib.SpatialCoreHipError:
        assert _lib.device_count() == 0          # no device: the call got as far as creating the context
    finally:
        log.removeHandler(caplog.handler)
    text = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("not integers" in m for m in text) == 1
    assert sum("1 cell(s) without a count" in m for m in text) == 1


# ---- 4. the surface ----------------------------------------------------------------------------------------------------------------
def test_ctypes_surface_and_all():
    import spatialcore_amd
    from spatialcore_amd import _lib, preprocessing

    assert preprocessing.__all__ == ["highly_variable_genes"] and callable(preprocessing.highly_variable_genes)
    assert "preprocessing" in spatialcore_amd.__all__ and spatialcore_amd.preprocessing is preprocessing
    lib = _lib.load_library()
    assert "sc_hvg_pearson" in _lib.SYMBOLS and hasattr(lib, "sc_hvg_pearson") and hasattr(_lib.Context, "hvg_pearson")
    assert len(_lib.SYMBOLS["sc_hvg_pearson"]) == 13
    header = open(os.path.join(ROOT, "include", "spatialcore_hip.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"#define SC_K_(HVG_\w+|COUNT_) (\d+)", header)}
    assert (ids["HVG_SETUP"], ids["HVG_DENSE"], ids["HVG_SPARSE"]) == (_lib.K_HVG_SETUP, _lib.K_HVG_DENSE, _lib.K_HVG_SPARSE)
    assert ids["COUNT_"] == _lib.K_HVG_SPARSE + 1
    # the entry point refuses on the host, before any HIP call: no context, no device
    out = np.zeros(4)
    p = out.ctypes.data_as(ctypes.c_void_p)
    ptr, idx, val = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.array([1.0, 2.0])
    rc = lib.sc_hvg_pearson(None, ptr.ctypes.data_as(ctypes.c_void_p), idx.ctypes.data_as(ctypes.c_void_p),
                            val.ctypes.data_as(ctypes.c_void_p), _lib.SC_F64, 2, 2, 100.0, 1.5, p, p, p, p)
    assert rc == _lib.SC_ERR_INVALID and b"sc_hvg_pearson: null pointer" in lib.sc_last_error()
    makefile = open(os.path.join(ROOT, "spatialcore_amd", "csrc", "Makefile")).read()
    assert "sc_hvg.hip" in makefile.split("SRCS =")[1].split("\n")[0] and "asan_hvg:" in makefile
