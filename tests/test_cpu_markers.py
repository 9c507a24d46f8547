"""rank_genes_groups without a device: the restatement is pinned against scipy's own Mann-Whitney test, the host
arithmetic (wilcoxon_tables) against the restatement, every argument error is raised before the library is asked for
anything, and the native entry point is declared, exported and bound."""
import os

import numpy as np
import pandas as pd
import pytest
from scipy.stats import mannwhitneyu

from conftest import make_adata
from wilcoxon_restated import group_table, integer_tables

N_CELLS, N_GROUPS = 6000, 5
GENE_KINDS = ["poisson", "lognorm", "normal", "all_zero", "zeros_rounded_normal", "constant"]


def _six_genes():
    rng = np.random.default_rng(7)
    n = N_CELLS
    counts = rng.poisson(1.3, n).astype(np.float64)
    depth = rng.uniform(0.5, 2.0, n)
    X = np.stack([counts,
                  np.log1p(rng.poisson(2.0, n) / depth),
                  rng.normal(0.0, 1.0, n),
                  np.zeros(n),
                  np.where(rng.uniform(size=n) < 0.3, 0.0, np.round(rng.normal(0.0, 2.0, n), 1)),
                  np.full(n, 2.5)], axis=1)
    code = rng.choice(N_GROUPS, n, p=[0.4, 0.3, 0.2, 0.07, 0.03]).astype(np.int32)
    return X, code


@pytest.fixture(scope="module")
def six():
    X, code = _six_genes()
    return X, code, integer_tables(X, code, N_GROUPS)


def _tables(t, **kw):
    from spatialcore_amd.spatial.markers import wilcoxon_tables

    return wilcoxon_tables(t["rank2"], t["tie_nonzero"], t["nnz"], t["sums"], t["n_neg"], t["group_n"], **kw)


# ---- the restatement against scipy's Mann-Whitney U -------------------------------------------------------------------

def test_restatement_agrees_with_mannwhitneyu(six):
    X, code, t = six
    N = N_CELLS
    for k in range(N_GROUPS):
        own = code == k
        n1 = int(own.sum())
        want = group_table(X, code, k, tie_correct=True)
        for g, kind in enumerate(GENE_KINDS):
            res = mannwhitneyu(X[own, g], X[~own, g], use_continuity=False, method="asymptotic")
            assert 2 * res.statistic == t["rank2"][g, k] - n1 * (n1 + 1), (kind, k)       # U = R - n1 (n1 + 1) / 2, exactly
            if kind in ("all_zero", "constant"):        # sd = 0: scipy divides by it, the table says score 0, p 1
                assert want["score64"][g] == 0.0 and want["pvals_all"][g] == 1.0
            else:
                np.testing.assert_allclose(want["pvals_all"][g], res.pvalue, rtol=1e-10, err_msg=f"{kind} group {k}")
        # the zero block's identity: all ties = non-zero ties + n_zero^3 - n_zero
        n_zero = N - t["nnz"].sum(axis=1)
        for g in range(len(GENE_KINDS)):
            assert t["tie_all"][g] == int(t["tie_nonzero"][g]) + int(n_zero[g]) ** 3 - int(n_zero[g])


# ---- wilcoxon_tables against the restatement -------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [
    dict(),
    dict(tie_correct=True),
    dict(tie_correct=True, corr_method="bonferroni"),
    dict(rankby_abs=True, n_genes=3),
    dict(n_genes=2, tie_correct=True),
    dict(log1p_base=2.0),
    dict(log1p_base=10.0, rankby_abs=True),
])
def test_wilcoxon_tables_against_the_restatement(six, kw):
    X, code, t = six
    got = _tables(t, **kw)
    n_out = kw.get("n_genes") or len(GENE_KINDS)
    assert got["order"].shape == (N_GROUPS, n_out) and got["scores"].dtype == np.float32
    assert got["logfoldchanges"].dtype == np.float32 and got["pvals"].dtype == np.float64
    for k in range(N_GROUPS):
        want = group_table(X, code, k, **kw)
        np.testing.assert_array_equal(got["order"][k], want["order"])
        np.testing.assert_array_equal(got["scores"][k], want["scores"])
        np.testing.assert_allclose(got["pvals"][k], want["pvals"], rtol=1e-12)
        np.testing.assert_allclose(got["pvals_adj"][k], want["pvals_adj"], rtol=1e-12)
        np.testing.assert_allclose(got["logfoldchanges"][k], want["logfoldchanges"], rtol=1e-5)
        np.testing.assert_allclose(got["pts"][k], want["pts"], rtol=1e-15)
        np.testing.assert_allclose(got["pts_rest"][k], want["pts_rest"], rtol=1e-15)


def test_report_subset_and_two_group_form(six):
    X, code, t = six
    got = _tables(t, report=[3, 1])
    for row, k in enumerate((3, 1)):
        np.testing.assert_array_equal(got["scores"][row], group_table(X, code, k)["scores"])
    # reference=<group>: the ranking is taken over two groups only (every other cell coded -1)
    two = np.where(code == 4, 0, np.where(code == 2, 1, -1)).astype(np.int32)
    t2 = integer_tables(X, two, 2)
    got = _tables(t2, report=[0], tie_correct=True)
    want = group_table(X, two, 0, tie_correct=True)
    np.testing.assert_array_equal(got["scores"][0], want["scores"])
    np.testing.assert_allclose(got["pvals"][0], want["pvals"], rtol=1e-12)
    for g in (0, 1, 2, 4):
        res = mannwhitneyu(X[code == 4, g], X[code == 2, g], use_continuity=False, method="asymptotic")
        np.testing.assert_allclose(want["pvals_all"][g], res.pvalue, rtol=1e-10)


def test_equal_scores_are_ordered_by_gene_position():
    # genes 0 / 2 / 4 are the same column, as are 1 / 3: equal scores in every group
    rng = np.random.default_rng(3)
    a, b = rng.poisson(2.0, 400).astype(np.float64), rng.normal(size=400)
    X = np.stack([a, b, a, b, a, np.zeros(400)], axis=1)
    code = (np.arange(400) % 3).astype(np.int32)
    t = integer_tables(X, code, 3)
    for kw in (dict(), dict(rankby_abs=True), dict(n_genes=4)):
        got = _tables(t, **kw)
        for k in range(3):
            order = list(got["order"][k])
            for first, then in ((0, 2), (2, 4), (1, 3)):      # equal scores are adjacent, the earlier gene first
                assert then not in order or (first in order and order.index(first) + 1 == order.index(then))
            np.testing.assert_array_equal(order, group_table(X, code, k, **kw)["order"])
    # an all-zero gene: score 0, p 1, and the adjustment keeps it at 1
    got = _tables(t, tie_correct=True)
    at = list(got["order"][0]).index(5)
    assert got["scores"][0][at] == 0.0 and got["pvals"][0][at] == 1.0 and got["pvals_adj"][0][at] == 1.0


def test_tie_sums_beyond_64_bits_stay_exact():
    # one constant non-zero gene over 3 * 10^6 cells: T = n^3 - n = 2.7e19 > 2^64; c must come out as exactly 0
    n = 3_000_000
    from spatialcore_amd.spatial.markers import wilcoxon_tables

    T = n ** 3 - n
    assert T > 2 ** 64
    group_n = np.array([n // 3, n - n // 3])
    rank2 = (group_n * (n + 1))[None, :]
    got = wilcoxon_tables(rank2, np.array([T], dtype=object), group_n[None, :], 2.0 * group_n[None, :], np.zeros(1), group_n,
                          tie_correct=True)
    assert (got["scores"] == 0.0).all() and (got["pvals"] == 1.0).all()


# ---- argument errors: nothing below may load the library ------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    from spatialcore_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("validation must not load the library or touch the device")

    monkeypatch.setattr(_lib, "default_context", refuse)
    monkeypatch.setattr(_lib, "load_library", refuse)


def _adata(n=40):
    rng = np.random.default_rng(0)
    ad = make_adata(rng.uniform(0, 100, (n, 2)), rng.poisson(1.0, (n, 4)).astype(np.float64))
    lab = np.array(["a", "b", "c"], dtype=object)[np.arange(n) % 3]
    lab[0] = "solo"
    ad.obs["domain"] = pd.Series(lab, index=ad.obs.index, dtype=object)
    return ad


@pytest.mark.parametrize("kwargs, match", [
    (dict(method="t-test"), "only method='wilcoxon' is supported, got 't-test'"),
    (dict(method="logreg"), "only method='wilcoxon' is supported"),
    (dict(corr_method="holm"), "corr_method must be one of"),
    (dict(groupby="nope"), "Column 'nope' not found in adata.obs"),
    (dict(genes=["g0", "missing"]), r"Genes not found in adata.var_names: \['missing'\]"),
    (dict(genes=["g0", "g0"]), "genes must not contain a name twice"),
    (dict(groups=["a", "z"]), r"groups \['z'\] not found"),
    (dict(groups="a"), "groups must be 'all' or a sequence of labels"),
    (dict(reference="z"), "reference = z needs to be one of groupby"),
    (dict(groups=["a"], reference="a"), "no group is left to test"),
    (dict(), "groups solo since they only contain one sample"),             # groups="all" reports the 1-cell group
    (dict(groups=["a", "b"], reference="solo"), "groups solo since they only contain one sample"),
    (dict(groups=["a"], n_genes=0), "n_genes must be >= 1, got 0"),
    (dict(groups=["a"], gene_batch=0), "gene_batch must be >= 1, got 0"),
])
def test_argument_errors_are_raised_without_the_library(no_library, kwargs, match):
    from spatialcore_amd.spatial import rank_genes_groups

    args = dict(groupby="domain")
    args.update(kwargs)
    ad = _adata()
    with pytest.raises(ValueError, match=match):
        rank_genes_groups(ad, **args)
    assert "rank_genes_groups" not in ad.uns


# ---- the native symbol ----------------------------------------------------------------------------------------------------

def test_the_native_entry_point_is_declared_exported_and_validates_on_the_host():
    from spatialcore_amd import _lib, spatial

    assert spatial.__all__[-1] == "rank_genes_groups"
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "spatialcore_hip.h")).read()
    assert "int sc_ranksum(sc_ctx *ctx, const int32_t *group_code, int64_t n, int32_t n_groups, int64_t *rank2_out," in header
    assert "---- N8" in header
    lib = _lib.load_library()
    assert "sc_ranksum" in _lib.SYMBOLS and hasattr(lib, "sc_ranksum") and hasattr(_lib.Context, "ranksum")
    code = np.zeros(4, dtype=np.int32)
    out = np.zeros(8, dtype=np.int64)
    # a null context is the first refusal: no device is needed to see it
    assert lib.sc_ranksum(None, code.ctypes.data, 4, 2, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                          out.ctypes.data, out.ctypes.data) == _lib.SC_ERR_INVALID
    assert b"sc_ranksum: null pointer" in lib.sc_last_error()
