"""rank_genes_groups without a device: the restatement is pinned against scipy's own Mann-Whitney test, the host
arithmetic (wilcoxon_tables) against the restatement, every argument error is raised before the library is asked for
anything, and the native entry point is declared, exported and bound.  It also builds the inputs of the kernel-edge tests
(tests/test_gpu_markers_edges.py, the two-batch case of tests/test_gpu_fullsize.py) and asserts here, without a device,
that each of them reaches the edge it is about."""
import os

import numpy as np
import pandas as pd
import pytest
from scipy.stats import mannwhitneyu

from conftest import make_adata
from wilcoxon_restated import group_table, integer_tables, integer_tables_bincount

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


# ---- inputs of tests/test_gpu_markers_edges.py and of the at-size batch test, and what they have to reach ---------------

RS_CHUNK, RS_TABLE, RS_PIECE = 2048, 4096, 256          # sc_ranksum.hip's chunk of sorted pairs, LDS table, piece of cells
ROUNDS_GROUPS = [300, 1365, 1366, 2048, 2049, 4096]     # genes per table round: 13, 3, 2, 2, 1, 1
# (n_groups, further all-zero genes).  With 13 genes per round every window of rounds_input() is followed by a gene that
# has pairs, so at 300 groups the second round starts at w0 + per as if next_gene were not there; with gene 13 empty as
# well the second round of the first chunk has to start at gene 14.
ROUNDS_CASES = [(300, ()), (300, (13,))] + [(k, ()) for k in ROUNDS_GROUPS[1:]]
PIECE_SIZES = [0, 1, 255, 256, 257, 0, 512, 513, 2]


def signed_fp64_input(n=6000):
    """The matrix and codes of test_gpu_markers.py::test_signed_fp64_values_take_the_two_pass_sort, cut to n cells."""
    from test_gpu_markers import _codes

    rng = np.random.default_rng(8)
    X = np.round(rng.normal(0.0, 1.5, (6000, 18)), 1)
    X[rng.uniform(size=(6000, 18)) < 0.35] = 0.0
    X[:, 5] = np.abs(X[:, 5])
    X[:, 6] = -np.abs(X[:, 6])
    return X[:n], _codes(6000, 4)[:n]


def rounds_input(also_zero=()):
    """3000 cells x 48 sparse float32 count genes, seven of them all zero: 4948 pairs in three chunks of k_rs_runs."""
    rng = np.random.default_rng(31)
    n, G = 3000, 48
    X = np.where(rng.uniform(size=(n, G)) < 0.04, rng.poisson(2.0, (n, G)) + 1.0, 0.0).astype(np.float32)
    X[:, [5, 6, 7, 8, 9, 20, 47] + list(also_zero)] = 0.0
    return X


def rounds_codes(n_groups, n=3000):
    code = np.random.default_rng(n_groups).integers(0, n_groups, n).astype(np.int32)
    code[0] = n_groups - 1
    return code


def rounds_walk(pairs_per_gene, n_groups):
    """The table rounds of k_rs_runs restated: per chunk of RS_CHUNK sorted pairs (gene-major), the first gene of every
    round's window.  A window holds RS_TABLE // n_groups genes; the next one starts at the first later gene that has a
    pair in the chunk."""
    gene_of = np.repeat(np.arange(len(pairs_per_gene)), pairs_per_gene)
    per = RS_TABLE // n_groups
    chunks = []
    for c0 in range(0, gene_of.size, RS_CHUNK):
        present = np.unique(gene_of[c0:c0 + RS_CHUNK])
        starts, w0 = [], present[0]
        while True:
            starts.append(int(w0))
            later = present[present >= w0 + min(present[-1] - w0 + 1, per)]
            if later.size == 0:
                break
            w0 = later[0]
        chunks.append(starts)
    return chunks


def piece_input():
    """Groups of PIECE_SIZES cells and 300 excluded ones, 17 raw-count float32 genes, in two cell orders: shuffled, and
    with every group's cells contiguous.  Returns ((X, code) shuffled, (X, code) contiguous)."""
    rng = np.random.default_rng(41)
    code = np.concatenate([np.full(s, k) for k, s in enumerate(PIECE_SIZES)] + [np.full(300, -1)]).astype(np.int32)
    code = code[rng.permutation(code.size)]
    X = rng.poisson(np.exp(rng.uniform(np.log(0.05), np.log(4.0), 17)), (code.size, 17)).astype(np.float32)
    by_group = np.argsort(np.where(code < 0, len(PIECE_SIZES), code), kind="stable")
    return (X, code), (X[by_group], code[by_group])


def mixed_class_input():
    """3000 cells x 33 genes as float64: float32-exact counts, except genes 20 and 32 (multiples of 0.1 of both signs)."""
    rng = np.random.default_rng(51)
    n = 3000
    X = rng.poisson(np.exp(rng.uniform(np.log(0.05), np.log(4.0), 33)), (n, 33)).astype(np.float64)
    for g in (20, 32):
        X[:, g] = np.where(rng.uniform(size=n) < 0.3, 0.0, np.round(rng.normal(0.0, 1.5, n), 1))
    return X


BATCH_PRIMES = [11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113,
                127, 131, 137, 139, 149, 151]


def closed_form_gene(n, g):
    """Gene g of the two-batch input as integers: ((a_g i + b_g) mod n) // 3 with a_g a prime >= 11, coprime to
    n = 2^x 3 5^y 7^z: i -> (a_g i + b_g) mod n is a bijection, so every value 0 .. n / 3 - 1 occurs exactly three times."""
    assert n % 3 == 0 and all(n % a for a in BATCH_PRIMES)
    i = np.arange(n, dtype=np.int64)
    return ((BATCH_PRIMES[g] * i + (7919 * g + 1) % n) % n) // 3


def closed_form_tables(n, code, n_groups, G=32):
    """What sc_ranksum returns for the genes closed_form_gene(n, 0 .. G - 1), without a sort: the three cells of value v
    hold the sorted positions 3 v + 1 .. 3 v + 3, so 2 * rank = 6 v + 4 (the zero block is the run v = 0); n / 3 - 1
    non-zero runs of three.  ``sums`` is the exact integer sum of the unscaled values.  (Sums of 6 v + 4 stay below
    n * 2 n < 2^53: the float64 accumulator of bincount is exact.)"""
    code = np.asarray(code).astype(np.int64)
    assert (code >= 0).all() and 2 * n * n < 2 ** 53
    group_n = np.bincount(code, minlength=n_groups).astype(np.int64)
    rank2 = np.zeros((G, n_groups), dtype=np.int64)
    nnz = np.zeros((G, n_groups), dtype=np.int64)
    sums = np.zeros((G, n_groups), dtype=np.float64)
    for g in range(G):
        v = closed_form_gene(n, g)
        rank2[g] = np.bincount(code, weights=6 * v + 4, minlength=n_groups).astype(np.int64)
        nnz[g] = group_n - np.bincount(code[v == 0], minlength=n_groups)
        sums[g] = np.bincount(code, weights=v, minlength=n_groups)
    return {"rank2": rank2, "tie_nonzero": np.array([24 * (n // 3 - 1)] * G, dtype=object), "nnz": nnz, "sums": sums,
            "n_neg": np.zeros(G, dtype=np.int64), "group_n": group_n}


def _assert_same_tables(a, b, sums_rtol):
    assert set(a) == set(b)
    for k in ("rank2", "nnz", "n_neg", "group_n"):
        assert a[k].dtype == b[k].dtype == np.int64
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert [int(t) for t in a["tie_nonzero"]] == [int(t) for t in b["tie_nonzero"]] and a["tie_all"] == b["tie_all"]
    np.testing.assert_allclose(a["sums"], b["sums"], rtol=sums_rtol, atol=0.0)


def test_bincount_restatement_equals_the_masked_one():
    X, code = signed_fp64_input(600)
    assert (X < 0).any() and (X.astype(np.float32).astype(np.float64) != X).any()
    _assert_same_tables(integer_tables_bincount(X, code, 5), integer_tables(X, code, 5), 1e-15)
    X, code = rounds_input(), rounds_codes(300)
    _assert_same_tables(integer_tables_bincount(X, code, 300), integer_tables(X, code, 300), 1e-15)
    # excluded cells and an empty group
    code = np.where(code % 7 == 0, -1, code % 4 * 2).astype(np.int32)
    _assert_same_tables(integer_tables_bincount(X, code, 8), integer_tables(X, code, 8), 1e-15)


def test_rounds_input_takes_several_table_rounds_at_every_group_count():
    X = rounds_input()
    pairs = (X != 0).sum(axis=0)
    assert X.dtype == np.float32 and pairs.sum() == 4948 and (pairs[[5, 6, 7, 8, 9, 20, 47]] == 0).all()
    live = pairs[pairs > 0]
    assert live.size == 41 and live.min() == 99 and live.max() == 143
    gene_of = np.repeat(np.arange(48), pairs)
    spans = [(int(gene_of[c]), int(gene_of[min(c + RS_CHUNK, 4948) - 1])) for c in range(0, 4948, RS_CHUNK)]
    assert spans == [(0, 23), (23, 40), (40, 46)]              # genes 23 and 40 straddle a seam; 5 .. 9 lie inside chunk 0
    want = {300: [2, 2, 1], 1365: [7, 6, 3], 1366: [10, 9, 4], 2048: [10, 9, 4], 2049: [18, 18, 7], 4096: [18, 18, 7]}
    for n_groups, also_zero in ROUNDS_CASES:
        per = RS_TABLE // n_groups
        walk = rounds_walk((rounds_input(also_zero) != 0).sum(axis=0), n_groups)
        if not also_zero:
            assert [len(starts) for starts in walk] == want[n_groups], n_groups
        assert max(len(starts) for starts in walk) >= 2
        steps = [b - a for starts in walk for a, b in zip(starts, starts[1:])]
        # some window starts past w0 + per: next_gene jumps a gap (at 300 groups only with gene 13 empty: see ROUNDS_CASES)
        assert any(step != per for step in steps) == ((n_groups, also_zero) != (300, ())), (n_groups, also_zero, walk)
        code = rounds_codes(n_groups)
        assert code.max() == n_groups - 1 and code.min() >= 0
    assert (np.bincount(rounds_codes(4096), minlength=4096) == 0).sum() > 1000


def test_piece_and_mixed_class_inputs_are_what_they_claim():
    (Xa, ca), (Xb, cb) = piece_input()
    for code in (ca, cb):
        assert np.bincount(code[code >= 0], minlength=9).tolist() == PIECE_SIZES and (code < 0).sum() == 300
    ranked = cb[cb >= 0]
    assert (np.diff(ranked) >= 0).all() and not (np.diff(ca[ca >= 0]) >= 0).all()      # contiguous groups / shuffled
    assert (np.diff(cb) != 0).sum() == 7                        # seven occupied groups and the excluded block: 7 seams
    assert Xa.dtype == np.float32 and (Xa == np.rint(Xa)).all() and ((Xa != 0).sum(axis=0) > 0).all()
    a, b = integer_tables(Xa, ca, 9), integer_tables(Xb, cb, 9)
    for k in ("rank2", "nnz", "sums", "n_neg", "group_n"):
        np.testing.assert_array_equal(a[k], b[k])
    X = mixed_class_input()
    exact = (X.astype(np.float32).astype(np.float64) == X).all(axis=0)
    assert np.flatnonzero(~exact).tolist() == [20, 32]
    assert all((X[:, g] < 0).any() and (X[:, g] > 0).any() and (X[:, g] == 0).any() for g in (20, 32))


def test_closed_form_of_the_two_batch_input():
    from test_gpu_markers import _codes

    n = 4200
    code = _codes(n, 11)
    X = np.stack([closed_form_gene(n, g) for g in range(32)], axis=1).astype(np.float64)
    for g in range(32):
        assert np.bincount(X[:, g].astype(np.int64), minlength=n // 3).tolist() == [3] * (n // 3)
    got, want = closed_form_tables(n, code, 5), integer_tables(X, code, 5)
    for k in ("rank2", "nnz", "sums", "n_neg", "group_n"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert [int(t) for t in got["tie_nonzero"]] == [int(t) for t in want["tie_nonzero"]]
    # the at-size arithmetic: one tile of 16 genes fits the pair budget of a sort batch, two do not
    big = 4_200_000
    assert big == 2 ** 6 * 3 * 5 ** 5 * 7 and 16 * (big - 3) == 67_199_952 <= 2 ** 27 < 2 * 16 * (big - 3) == 134_399_904
    assert big // 3 - 1 == 1_399_999 < 2 ** 24                 # every unscaled value is a float32


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
