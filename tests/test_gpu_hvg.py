"""spatialcore_amd.preprocessing on the device: the exact fields on integer counts, the residual variances against the
definition and, bit for bit, against the restatement in the device's order, the selection, the batch rule, the public
surface and the chain into pca.

Cases (tests/hvg_restated.py: CASES) are the smallest at which the kernels can go wrong; each names its edge there, against
sc_hvg.hip's 1024-cell slices and 256-gene blocks and sc_colsort.h's 512-entry column chunks.

TOL = 1e-10, per gene, relative to the textbook value.  Measured on the CPU with these recipes (numpy alone, every case of
CASES): the split form in the device's order in fp64 (hvg_restated.ordered) differs from the two-pass textbook variance by
at most 2.9e-14; the same form carried in float32 differs by at least 3.9e-6 on every case (the figures of the first
measurement, on a serial-order split form at 300x9, 777x37 and 2000x200 with the default clip and clip = 3, were 4.5e-14
and 4.9e-6).  1e-10 sits 3400x above the first figure and 39000x below the second; tests/test_cpu_hvg.py asserts both
margins (>= 100x) on every case.  The device is also compared with ordered() itself: both sides use correctly rounded
division and square root and round every product and sum separately, so the comparison is bit for bit.

The selection is compared with the textbook's without exclusions: the smallest relative gap between two positive textbook
variances is 6.0e-7 (2000x200) and at least 7.9e-7 elsewhere, >= 100 TOL on every case (asserted in tests/test_cpu_hvg.py)."""
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import sparse

import hvg_restated as R
import pca_restated
from conftest import make_adata

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
BY_NAME = {c[0]: c for c in R.CASES}


def _adata(X, **obs):
    ad = make_adata(np.zeros((X.shape[0], 2)), X.copy())
    for k, v in obs.items():
        ad.obs[k] = v
    return ad


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


@functools.lru_cache(maxsize=None)
def _device(name):
    """(sum x, sum x^2, residual mean, residual variance) of one sc_hvg_pearson on the case's canonical CSR."""
    case = BY_NAME[name]
    X = R.matrix(case)
    clip = float(np.sqrt(X.shape[0])) if case[6] is None else case[6]
    out = tuple(a.copy() for a in _ctx().hvg_pearson(X.indptr, X.indices, X.data, X.shape[1], case[5], clip))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _textbook(name):
    case = BY_NAME[name]
    return R.textbook(R.matrix(case), case[5], case[6])


@functools.lru_cache(maxsize=None)
def _public(name, n_top):
    from spatialcore_amd.preprocessing import highly_variable_genes

    case = BY_NAME[name]
    return highly_variable_genes(_adata(R.matrix(case)), n_top_genes=n_top, theta=case[5], clip=case[6])


# ---- 1. the exact fields -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.CASES if c[1] != "real"])
def test_sums_means_and_variances_are_exact_on_counts(name):
    X = R.matrix(BY_NAME[name])
    s1, s2, means, variances = R.moments(X)
    got = _device(name)
    np.testing.assert_array_equal(got[0], s1)
    np.testing.assert_array_equal(got[1], s2)
    ad = _public(name, 5)
    np.testing.assert_array_equal(ad.var["means"].values, means)
    np.testing.assert_array_equal(ad.var["variances"].values, variances)


# ---- 2. against the definition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.IDS)
def test_residual_variances_against_textbook(name):
    want, got = _textbook(name), _device(name)[3]
    err = R.rel_err(got, want)
    print(f"hvg {name}: device against textbook {err:.2e}")
    assert err <= TOL
    assert np.all(got[want == 0] == 0) and np.all(got >= 0)
    G = got.size
    if G >= 4:
        assert got[G // 2] == 0.0 and _device(name)[2][G // 2] == 0.0          # the all-zero gene


# ---- 3. against the restatement in the device's order ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.IDS)
def test_device_equals_ordered_bit_for_bit(name):
    case = BY_NAME[name]
    want = R.ordered(R.matrix(case), case[5], case[6])
    got = _device(name)
    for key, a in zip(("sum", "sumsq", "mean", "var"), got):
        np.testing.assert_array_equal(a, want[key], err_msg=key)


# ---- 4. the selection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.IDS)
def test_selection_equals_the_textbook_selection(name):
    G = BY_NAME[name][3]
    for n_top in sorted({1, max(1, G // 4), G, G + 5}):
        ad = _public(name, n_top)
        hv, rank = R.select(_textbook(name), n_top)
        np.testing.assert_array_equal(ad.var["highly_variable"].values, hv)
        np.testing.assert_array_equal(ad.var["highly_variable_rank"].values, rank)
        np.testing.assert_array_equal(ad.var["residual_variances"].values, _device(name)[3])
        assert ad.var["highly_variable"].values.dtype == bool and ad.var["highly_variable_rank"].values.dtype == np.float64
        assert ad.var["highly_variable"].sum() == min(n_top, G)
    if G >= 4:
        assert _public(name, G).var["highly_variable_rank"].values[G // 2] == G - 1        # the all-zero gene ranks last


# ---- 5. the same bytes ---------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import hvg_restated as R
from spatialcore_amd import _lib
ctx = _lib.default_context(0)
out = {{}}
for case in R.CASES:
    if case[0] in {names!r}:
        X = R.matrix(case)
        clip = float(np.sqrt(X.shape[0])) if case[6] is None else case[6]
        out[case[0]] = np.stack(ctx.hvg_pearson(X.indptr, X.indices, X.data, X.shape[1], case[5], clip))
np.savez(sys.argv[1], **out)
"""


def test_two_calls_and_a_child_on_four_hardware_queues_give_the_same_bytes(tmp_path):
    """A second call here, and a fresh child held to GPU_MAX_HW_QUEUES=4 (this process asked for 24)."""
    names = ["2000x200-clip3", "1025x257", "777x37-f32-real"]
    for name in names:
        case = BY_NAME[name]
        X = R.matrix(case)
        clip = float(np.sqrt(X.shape[0])) if case[6] is None else case[6]
        again = _ctx().hvg_pearson(X.indptr, X.indices, X.data, X.shape[1], case[5], clip)
        assert np.stack(again).tobytes() == np.stack(_device(name)).tobytes()
    script = tmp_path / "hvg_child.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), names=names))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    run = subprocess.run([sys.executable, str(script), str(tmp_path / "child.npz")], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    child = np.load(tmp_path / "child.npz")
    for name in names:
        assert child[name].tobytes() == np.stack(_device(name)).tobytes()


# ---- 6. batches --------------------------------------------------------------------------------------------------------------------------
def test_batch_columns_equal_the_restated_rule_on_textbook_variances():
    from spatialcore_amd.preprocessing import highly_variable_genes

    X = R.matrix(BY_NAME["777x37"])
    n, G = X.shape
    batch = np.where(np.random.default_rng(5).random(n) < 0.4, "b_late", "a_early")      # interleaved rows, sorted category order
    rows = [np.flatnonzero(batch == b) for b in ("a_early", "b_late")]
    V = np.stack([R.textbook(X[r]) for r in rows])                                       # own sums, own n, own default clip
    assert min(R.smallest_gap(v) for v in V) >= 100 * TOL
    for n_top in (6, G):
        ad = highly_variable_genes(_adata(X, batch=batch), n_top_genes=n_top, batch_key="batch")
        want = R.select_batches(V, n_top)
        np.testing.assert_array_equal(ad.var["highly_variable_nbatches"].values, want["nbatches"])
        np.testing.assert_array_equal(ad.var["highly_variable_intersection"].values, want["intersection"])
        np.testing.assert_array_equal(ad.var["highly_variable"].values, want["highly_variable"])
        np.testing.assert_array_equal(ad.var["highly_variable_rank"].values, want["rank"])
        assert R.rel_err(ad.var["residual_variances"].values, want["residual_variances"]) <= TOL
        _, _, means, variances = R.moments(X)                                            # over all cells
        np.testing.assert_array_equal(ad.var["means"].values, means)
        np.testing.assert_array_equal(ad.var["variances"].values, variances)
        assert ad.uns["hvg"]["params"]["batch_key"] == "batch"
    # a batch's variances are those of a call on its rows alone
    ctx = _ctx()
    per = [ctx.hvg_pearson(X[r].indptr, X[r].indices, X[r].data, G, 100.0, float(np.sqrt(r.size)))[3] for r in rows]
    np.testing.assert_array_equal(ad.var["residual_variances"].values, np.stack(per).mean(axis=0))


# ---- 7. the public surface -----------------------------------------------------------------------------------------------------------------
def test_subset_copy_layer_and_metadata():
    from spatialcore_amd.preprocessing import highly_variable_genes

    X = R.matrix(BY_NAME["777x37"])
    n, G = X.shape
    ad = _adata(sparse.csr_matrix(X.shape, dtype=np.float64))
    ad.layers["counts"] = X.copy()
    out = highly_variable_genes(ad, n_top_genes=8, layer="counts", copy=True)
    assert out is not ad and "means" not in ad.var and "hvg" not in ad.uns and "spatialcore_metadata" not in ad.uns
    assert list(out.var.columns) == ["means", "variances", "residual_variances", "highly_variable_rank", "highly_variable"]
    assert out.uns["hvg"] == {"flavor": "pearson_residuals", "computed_on": "counts",
                              "params": {"n_top_genes": 8, "theta": 100.0, "clip": None, "batch_key": None}}
    np.testing.assert_array_equal(out.var["residual_variances"].values, _device("777x37")[3])
    op = out.uns["spatialcore_metadata"]["operations"][-1]
    assert op["function"] == "highly_variable_genes" and op["outputs"]["uns"] == "hvg"
    assert op["outputs"]["var"] == list(out.var.columns)
    assert op["parameters"]["n_genes"] == G and op["parameters"]["n_selected"] == 8 and op["parameters"]["layer"] == "counts"
    # in place on X, dense input, csc input: the same columns
    same = _adata(X)
    assert highly_variable_genes(same, n_top_genes=8) is same and same.uns["hvg"]["computed_on"] == "adata.X"
    for other in (make_adata(np.zeros((n, 2)), X.toarray()), make_adata(np.zeros((n, 2)), X.tocsc())):
        highly_variable_genes(other, n_top_genes=8)
        for col in out.var.columns:
            np.testing.assert_array_equal(other.var[col].values, out.var[col].values)
    # subset: a new object cut to the selected genes, in gene order, with their columns
    cut = highly_variable_genes(_adata(X), n_top_genes=8, subset=True)
    keep = np.flatnonzero(out.var["highly_variable"].values)
    assert cut.shape == (n, 8) and list(cut.var_names) == [f"g{i}" for i in keep]
    np.testing.assert_array_equal(cut.X.toarray(), X.toarray()[:, keep])
    assert cut.var["highly_variable"].all() and sorted(cut.var["highly_variable_rank"]) == list(range(8))
    assert cut.uns["hvg"]["flavor"] == "pearson_residuals"
    # theta = inf and an explicit clip reach the device
    poisson = highly_variable_genes(_adata(X), n_top_genes=8, theta=float("inf"), clip=3.0)
    assert R.rel_err(poisson.var["residual_variances"].values, R.textbook(X, float("inf"), 3.0)) <= TOL


def test_empty_cells_and_real_values_warn_and_count(caplog):
    from spatialcore_amd.preprocessing import highly_variable_genes

    log = logging.getLogger("spatialcore_amd")
    log.addHandler(caplog.handler)
    try:
        ad = highly_variable_genes(_adata(R.matrix(BY_NAME["777x37-f32-real"])), n_top_genes=5)
    finally:
        log.removeHandler(caplog.handler)
    text = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("not integers" in m for m in text) == 1 and sum("1 cell(s) without a count" in m for m in text) == 1
    assert np.all(np.isfinite(ad.var["residual_variances"].values))
    np.testing.assert_array_equal(ad.var["residual_variances"].values, _device("777x37-f32-real")[3])


def test_library_refusals_reach_python():
    """What only the library checks: a CSR the Python layer never builds."""
    ctx = _ctx()
    with pytest.raises(ValueError, match="sc_hvg_pearson: row 0 is not canonical"):
        ctx.hvg_pearson(np.array([0, 2, 2]), np.array([1, 1]), np.array([1.0, 2.0]), 3, 100.0, 2.0)
    with pytest.raises(ValueError, match="stored value 1 is negative"):
        ctx.hvg_pearson(np.array([0, 2, 2]), np.array([0, 1]), np.array([1.0, -2.0]), 3, 100.0, 2.0)
    with pytest.raises(ValueError, match="theta must be > 0"):
        ctx.hvg_pearson(np.array([0, 2, 2]), np.array([0, 1]), np.array([1.0, 2.0]), 3, 0.0, 2.0)


# ---- 8. the chain ------------------------------------------------------------------------------------------------------------------------
def test_selected_genes_feed_pca_on_a_matrix_pca_alone_refuses():
    from spatialcore_amd.pca import pca
    from spatialcore_amd.preprocessing import highly_variable_genes

    n, G = 300, 4200
    rng = np.random.default_rng(3)
    background = sparse.random(n, G - 40, density=0.02, random_state=rng, data_rvs=lambda k: 1.0 + rng.poisson(1.0, k), dtype=np.float64)
    X = sparse.hstack([pca_restated.counts(n, 40, 11), background]).tocsr()      # a block of structured genes among the sparse ones
    ad = _adata(X)
    with pytest.raises(ValueError, match="select genes first"):
        pca(ad, 10, normalize=True)
    highly_variable_genes(ad, n_top_genes=200)
    selected = list(ad.var_names[ad.var["highly_variable"].values])
    assert len(selected) == 200
    pca(ad, 10, genes=selected, normalize=True)
    assert ad.obsm["X_pca"].shape == (n, 10) and np.all(np.isfinite(ad.obsm["X_pca"]))
    assert ad.uns["pca"]["genes"] == selected
    assert [op["function"] for op in ad.uns["spatialcore_metadata"]["operations"]] == ["highly_variable_genes", "pca"]
