"""GPU: sc_ranksum and rank_genes_groups against the scipy.stats.rankdata restatement (tests/wilcoxon_restated.py).

The integer outputs (rank sums, tie sums, non-zero and negative counts, group sizes) are compared with ==.  The value
sums: == for integer-valued data (exact in any order), rtol 1e-12 and nothing else for data of one sign per gene, and
for the one case with both signs in a gene the bound n_k * eps * sum |x| per (gene, group) against math.fsum (a
relative bound on a cancelling sum means nothing).  Final tables: scores at float32 equality, p-values at rtol 1e-12
-- both are host arithmetic on identical integers.
"""
import math

import numpy as np
import pandas as pd
import pytest
from scipy import sparse
from scipy.stats import mannwhitneyu

from conftest import make_adata, synth
from wilcoxon_restated import dense, group_table, integer_tables

pytestmark = pytest.mark.gpu

INT_KEYS = ("rank2", "nnz", "n_neg", "group_n")


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


def _ranksum(X, code, n_groups):
    ctx = _ctx()
    ctx.set_expression(X, np.arange(X.shape[1], dtype=np.int32))
    return ctx.ranksum(code, n_groups)


def _assert_tables(got, want, label="", sums="rtol", data=None):
    """``sums``: "exact" for integer-valued data (every partial sum is an integer below 2^53: exact in any order),
    "rtol" = 1e-12 relative and nothing else, "signed" for values of both signs, where a relative bound on a sum that
    cancels means nothing: per (gene, group) against math.fsum with the bound n_k * eps * sum |x| that any order of
    n_k fp64 additions keeps (``data`` = (X, code))."""
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{label} {k}")
    assert [int(t) for t in got["tie_nonzero"]] == [int(t) for t in want["tie_nonzero"]], label
    if sums == "exact":
        np.testing.assert_array_equal(got["sums"], want["sums"], err_msg=f"{label} sums")
    elif sums == "rtol":
        np.testing.assert_allclose(got["sums"], want["sums"], rtol=1e-12, atol=0.0, err_msg=f"{label} sums")
    else:
        X, code = dense(data[0]).astype(np.float64), data[1]
        eps = np.finfo(np.float64).eps
        for g in range(X.shape[1]):
            for k in range(want["group_n"].size):
                x = X[code == k, g]
                err = abs(got["sums"][g, k] - math.fsum(x))
                assert err <= x.size * eps * math.fsum(np.abs(x)), (label, g, k, err)


def _codes(n, seed, n_groups=5):
    """Uneven groups; the last one has exactly 2 cells."""
    rng = np.random.default_rng(seed)
    p = np.arange(n_groups - 1, 0, -1, dtype=np.float64)
    code = rng.choice(n_groups - 1, n, p=p / p.sum()).astype(np.int32)
    code[rng.choice(n, 2, replace=False)] = n_groups - 1
    assert np.bincount(code, minlength=n_groups)[-1] == 2
    return code


def _adata(X, code, names=None):
    n = X.shape[0]
    ad = make_adata(np.random.default_rng(1).uniform(0, 100, (n, 2)), X)
    width = len(str(int(np.max(code))))
    lab = np.array([None if c < 0 else (names[c] if names else f"d{c:0{width}d}") for c in code], dtype=object)
    ad.obs["domain"] = pd.Series(lab, index=ad.obs.index, dtype=object)
    return ad


def _assert_group(res, group, want):
    np.testing.assert_array_equal(res["names"][group], np.array([f"g{i}" for i in want["order"]], dtype=object))
    assert res["scores"][group].dtype == np.float32 and res["pvals"][group].dtype == np.float64
    np.testing.assert_array_equal(res["scores"][group], want["scores"])
    np.testing.assert_allclose(res["pvals"][group], want["pvals"], rtol=1e-12)
    np.testing.assert_allclose(res["pvals_adj"][group], want["pvals_adj"], rtol=1e-12)
    np.testing.assert_allclose(res["logfoldchanges"][group], want["logfoldchanges"], rtol=1e-5)


# ---- 1: raw counts, CSR and dense --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def counts():
    _, X = synth(6000, 24, 5, dtype=np.float32, sparse_x=True)
    code = _codes(6000, 2)
    return X, code, integer_tables(X, code, 5)


@pytest.mark.parametrize("form", ["csr", "dense"])
def test_raw_counts_csr_and_dense(counts, form):
    X, code, want = counts
    got = _ranksum(X if form == "csr" else dense(X), code, 5)
    _assert_tables(got, want, form, sums="exact")


def test_final_tables_of_raw_counts(counts):
    from spatialcore_amd.spatial import rank_genes_groups

    X, code, _ = counts
    ad = _adata(X, code)
    rank_genes_groups(ad, "domain", tie_correct=True, pts=True)
    res = ad.uns["rank_genes_groups"]
    assert res["params"] == {"groupby": "domain", "reference": "rest", "method": "wilcoxon", "use_raw": False, "layer": None,
                             "corr_method": "benjamini-hochberg"}
    assert res["names"].dtype.names == ("d0", "d1", "d2", "d3", "d4")          # d4 has 2 cells: the smallest legal group
    for k in range(5):
        want = group_table(X, code, k, tie_correct=True)
        _assert_group(res, f"d{k}", want)
        np.testing.assert_allclose(res["pts"][f"d{k}"].values, want["pts"], rtol=1e-15)
        np.testing.assert_allclose(res["pts_rest"][f"d{k}"].values, want["pts_rest"], rtol=1e-15)
    assert list(res["pts"].index) == [f"g{i}" for i in range(24)]


# ---- 2: log-normalised float32: a large zero block, almost tie-free non-zeros ------------------------------------------

def test_normalised_float32():
    _, X = synth(6000, 24, 6, normalize=True)
    assert X.dtype == np.float32
    code = _codes(6000, 3)
    _assert_tables(_ranksum(X, code, 5), integer_tables(X, code, 5))


# ---- 3: negatives and ties on both sides of zero, fp64 that is not float32-exact: the two-pass sort -------------------

def test_signed_fp64_values_take_the_two_pass_sort():
    rng = np.random.default_rng(8)
    n, G = 6000, 18
    X = np.round(rng.normal(0.0, 1.5, (n, G)), 1)             # multiples of 0.1: ties, and no float32 holds 0.1
    X[rng.uniform(size=(n, G)) < 0.35] = 0.0
    X[:, 5] = np.abs(X[:, 5])
    X[:, 6] = -np.abs(X[:, 6])
    assert (X.astype(np.float32).astype(np.float64) != X).any() and (X < 0).any()
    code = _codes(n, 4)
    want = integer_tables(X, code, 5)
    assert want["n_neg"][6] > 0 and want["n_neg"][5] == 0
    _assert_tables(_ranksum(X, code, 5), want, "dense fp64", sums="signed", data=(X, code))
    _assert_tables(_ranksum(sparse.csr_matrix(X), code, 5), want, "csr fp64", sums="signed", data=(X, code))
    # the same tie structure as float32 input: another matrix (0.1f != 0.1), the one-pass sort
    X32 = X.astype(np.float32)
    _assert_tables(_ranksum(X32, code, 5), integer_tables(X32, code, 5), "float32", sums="signed", data=(X32, code))


# ---- 4: an all-zero gene and a constant non-zero gene ---------------------------------------------------------------------

def test_all_zero_and_constant_genes():
    from spatialcore_amd.spatial import rank_genes_groups

    rng = np.random.default_rng(9)
    n = 3000
    X = np.stack([np.zeros(n), np.full(n, 3.25), rng.poisson(1.0, n).astype(np.float64), np.full(n, -1.5)], axis=1)
    code = _codes(n, 5, 4)
    want = integer_tables(X, code, 4)
    assert int(want["tie_nonzero"][1]) == n ** 3 - n and int(want["tie_nonzero"][0]) == 0
    _assert_tables(_ranksum(X, code, 4), want, sums="exact")       # multiples of 0.25 below 2^53
    ad = _adata(X, code)
    rank_genes_groups(ad, "domain", tie_correct=True)
    res = ad.uns["rank_genes_groups"]
    for k in range(4):
        want = group_table(X, code, k, tie_correct=True)
        _assert_group(res, f"d{k}", want)
        flat = np.isin(res["names"][f"d{k}"], ["g0", "g1", "g3"])
        assert (res["scores"][f"d{k}"][flat] == 0).all() and (res["pvals"][f"d{k}"][flat] == 1).all()     # sd = 0


# ---- 5: run seams ------------------------------------------------------------------------------------------------------------

RUNS = [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16385]


@pytest.mark.parametrize("neighbour", [False, True])
def test_tie_runs_across_chunk_seams(neighbour):
    rng = np.random.default_rng(10)
    n = 40000
    vals = np.concatenate([np.full(t, 1.0 + j) for j, t in enumerate(RUNS)] + [np.zeros(n - sum(RUNS))])
    assert vals.size == n and sum(RUNS) == 32705
    x = rng.permutation(vals)
    cols = [x]
    if neighbour:       # a gene in front whose non-zero count is no multiple of any chunk: the gene boundary falls inside one
        before = np.where(rng.uniform(size=n) < 0.3337, rng.poisson(3.0, n) + 1.0, 0.0)
        cols = [before, x, rng.permutation(vals) * -1.0]
    X = np.stack(cols, axis=1).astype(np.float32)
    code = rng.choice(3, n, p=[0.5, 0.3, 0.2]).astype(np.int32)
    want = integer_tables(X, code, 3)
    gene = 1 if neighbour else 0
    assert int(want["tie_nonzero"][gene]) == sum(t ** 3 - t for t in RUNS)
    _assert_tables(_ranksum(X, code, 3), want, sums="exact")
    _assert_tables(_ranksum(X.astype(np.float64) * 0.1, code, 3), integer_tables(X.astype(np.float64) * 0.1, code, 3), "fp64")


# ---- 6: gene counts around the tile, batches ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def forty():
    _, Xc = synth(3000, 20, 12, dtype=np.float32, sparse_x=False)
    _, Xn = synth(3000, 20, 13, sparse_x=False, normalize=True)
    X = np.concatenate([Xc, Xn], axis=1)[:, np.random.default_rng(0).permutation(40)]
    code = _codes(3000, 6, 4)
    alone = [_ranksum(X[:, [g]], code, 4) for g in range(40)]
    return X, code, alone


@pytest.mark.parametrize("n_loaded", [1, 15, 16, 17, 33])
def test_a_gene_gives_the_same_bits_whatever_it_is_loaded_with(forty, n_loaded):
    X, code, alone = forty
    got = _ranksum(X[:, :n_loaded], code, 4)
    for g in range(n_loaded):
        for k in ("rank2", "nnz", "sums", "n_neg"):
            assert got[k][g].tobytes() == alone[g][k][0].tobytes(), (g, k)
        assert int(got["tie_nonzero"][g]) == int(alone[g]["tie_nonzero"][0])


def test_gene_batches_do_not_change_the_result(forty):
    from spatialcore_amd.spatial import rank_genes_groups

    X, code, _ = forty
    one, many = _adata(X, code), _adata(X, code)
    rank_genes_groups(one, "domain", groups=["d0", "d1", "d2"], tie_correct=True, pts=True)
    rank_genes_groups(many, "domain", groups=["d0", "d1", "d2"], tie_correct=True, pts=True, gene_batch=16)
    a, b = one.uns["rank_genes_groups"], many.uns["rank_genes_groups"]
    for field in ("scores", "logfoldchanges", "pvals", "pvals_adj"):
        assert a[field].tobytes() == b[field].tobytes(), field
    assert a["names"].tolist() == b["names"].tolist()
    assert a["pts"].equals(b["pts"]) and a["pts_rest"].equals(b["pts_rest"])
    _assert_group(b, "d1", group_table(X, code, 1, tie_correct=True))


# ---- 7: group counts ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_groups", [1, 2, 300])
def test_group_counts(n_groups):
    _, X = synth(5000, 6, 14, dtype=np.float32)
    rng = np.random.default_rng(n_groups)
    code = rng.integers(0, n_groups, 5000).astype(np.int32)
    got = _ranksum(X, code, n_groups)
    _assert_tables(got, integer_tables(X, code, n_groups), sums="exact")
    if n_groups == 300:
        assert got["nnz"][:, 256:].sum() > 0          # codes beyond one byte arrive


# ---- 8: excluded cells; reference=<group> end to end -------------------------------------------------------------------------

def test_excluded_cells_and_a_reference_group():
    from spatialcore_amd.spatial import rank_genes_groups

    _, X = synth(4000, 10, 15, normalize=True)
    code = _codes(4000, 7, 5)
    masked = np.where(code == 1, -1, np.where(code > 1, code - 1, code)).astype(np.int32)
    _assert_tables(_ranksum(X, masked, 4), integer_tables(X, masked, 4))
    ad = _adata(X, code)
    rank_genes_groups(ad, "domain", groups=["d0", "d1"], reference="d2", tie_correct=True)
    res = ad.uns["rank_genes_groups"]
    assert res["names"].dtype.names == ("d0", "d1") and res["params"]["reference"] == "d2"
    D = dense(X).astype(np.float64)
    for k in (0, 1):
        two = np.where(code == k, 0, np.where(code == 2, 1, -1))
        want = group_table(X, two, 0, tie_correct=True)
        _assert_group(res, f"d{k}", want)
        pos = {name: i for i, name in enumerate(res["names"][f"d{k}"])}
        for g in range(10):
            ref = mannwhitneyu(D[code == k, g], D[code == 2, g], use_continuity=False, method="asymptotic")
            np.testing.assert_allclose(res["pvals"][f"d{k}"][pos[f"g{g}"]], ref.pvalue, rtol=1e-10)


# ---- 9: missing labels and a selection of groups against the rest ---------------------------------------------------------

def test_missing_labels_and_selected_groups_against_the_rest():
    from spatialcore_amd.spatial import rank_genes_groups

    _, X = synth(4000, 10, 16, dtype=np.float32)
    code = _codes(4000, 8, 5)
    code[::17] = -1                                            # cells without a label still count in "rest"
    ad = _adata(X, code)
    assert ad.obs["domain"].isna().sum() == (code < 0).sum()
    rank_genes_groups(ad, "domain", groups=["d2", "d0"], n_genes=4, rankby_abs=True, corr_method="bonferroni")
    res = ad.uns["rank_genes_groups"]
    assert res["names"].dtype.names == ("d0", "d2") and res["names"].shape == (4,)
    for k in (0, 2):
        everyone = np.where(code == k, 0, 1)                   # group k against every other cell
        _assert_group(res, f"d{k}", group_table(X, everyone, 0, n_genes=4, rankby_abs=True, corr_method="bonferroni"))


# ---- 10: determinism ---------------------------------------------------------------------------------------------------------------

def test_two_identical_calls_give_identical_bytes(counts):
    X, code, _ = counts
    a, b = _ranksum(X, code, 5), _ranksum(X, code, 5)
    for k in INT_KEYS + ("sums",):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["tie_nonzero"].tolist() == b["tie_nonzero"].tolist()


# ---- 11: errors --------------------------------------------------------------------------------------------------------------------

def test_documented_errors():
    from spatialcore_amd import _lib

    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.SpatialCoreHipError, match="sc_ranksum: no expression loaded"):
            fresh.ranksum(np.zeros(10, dtype=np.int32), 2)
    finally:
        fresh.close()
    ctx = _ctx()
    X = np.random.default_rng(0).poisson(1.0, (500, 3)).astype(np.float64)
    ctx.set_expression(X, np.arange(3, dtype=np.int32))
    code = np.zeros(500, dtype=np.int32)
    code[123] = 2
    with pytest.raises(ValueError, match=r"group code 2 of cell 123 outside \[-1, 2\)"):
        ctx.ranksum(code, 2)
    code[123] = -2
    with pytest.raises(ValueError, match="group code -2 of cell 123"):
        ctx.ranksum(code, 2)
    with pytest.raises(ValueError, match=r"n_groups=4097 outside \[1, 4096\]"):
        ctx.ranksum(np.zeros(500, dtype=np.int32), 4097)
    with pytest.raises(ValueError, match=r"n_groups=0 outside \[1, 4096\]"):
        ctx.ranksum(np.zeros(500, dtype=np.int32), 0)
    with pytest.raises(ValueError, match="499 group codes for 500 loaded cells"):
        ctx.ranksum(np.zeros(499, dtype=np.int32), 1)
    for value in (np.nan, np.inf):
        X[77, 1] = value
        ctx.set_expression(X, np.arange(3, dtype=np.int32))
        with pytest.raises(ValueError, match="sc_ranksum: gene 1 has a non-finite value"):
            ctx.ranksum(np.zeros(500, dtype=np.int32), 1)


# ---- 12: a tie sum above 2^64 ---------------------------------------------------------------------------------------------------

def test_a_tie_sum_beyond_64_bits():
    n = 3_000_000
    X = np.full((n, 1), 2.5, dtype=np.float32)
    code = (np.arange(n) % 3 == 0).astype(np.int32)
    got = _ranksum(X, code, 2)
    assert n ** 3 - n > 2 ** 64 and int(got["tie_nonzero"][0]) == n ** 3 - n
    group_n = np.bincount(code)
    np.testing.assert_array_equal(got["group_n"], group_n)
    np.testing.assert_array_equal(got["rank2"][0], group_n * (n + 1))           # every cell has rank (n + 1) / 2
    np.testing.assert_array_equal(got["nnz"][0], group_n)
    np.testing.assert_array_equal(got["sums"][0], 2.5 * group_n)                # exact: multiples of 2.5 below 2^53


# ---- 13: genes= in another order, a layer, a log1p base, a categorical column, copy=True ------------------------------

def test_gene_subset_layer_log1p_base_categories_and_copy():
    from spatialcore_amd.spatial import rank_genes_groups

    _, X = synth(3000, 12, 17, sparse_x=False, normalize=True)
    code = _codes(3000, 9, 4)
    ad = make_adata(np.zeros((3000, 2)), np.zeros((3000, 12), dtype=np.float32))       # X itself holds nothing
    ad.layers["lognorm"] = sparse.csr_matrix(X)
    ad.uns["log1p"] = {"base": 2.0}
    # categories in an order of their own ("10" sorts before "2" as text), one of them unused
    cats = ["2", "10", "unused", "1", "3"]
    ad.obs["domain"] = pd.Categorical(np.array(["2", "10", "1", "3"])[code], categories=cats)
    picked = [7, 2, 11, 0, 5]                                                           # not ascending
    out = rank_genes_groups(ad, "domain", genes=[f"g{i}" for i in picked], layer="lognorm", tie_correct=True, pts=True,
                            copy=True)
    assert "rank_genes_groups" not in ad.uns and out is not ad
    res = out.uns["rank_genes_groups"]
    assert res["names"].dtype.names == ("2", "10", "1", "3") and res["params"]["layer"] == "lognorm"
    assert list(res["pts"].index) == [f"g{i}" for i in picked]
    for k, name in enumerate(("2", "10", "1", "3")):
        want = group_table(X[:, picked], code, k, tie_correct=True, log1p_base=2.0)
        np.testing.assert_array_equal(res["names"][name], np.array([f"g{picked[i]}" for i in want["order"]], dtype=object))
        np.testing.assert_array_equal(res["scores"][name], want["scores"])
        np.testing.assert_allclose(res["pvals_adj"][name], want["pvals_adj"], rtol=1e-12)
        np.testing.assert_allclose(res["logfoldchanges"][name], want["logfoldchanges"], rtol=1e-5)
        np.testing.assert_allclose(res["pts"][name].values, want["pts"], rtol=1e-15)
