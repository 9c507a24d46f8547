"""CPU: the restatement of the ligand-receptor test (tests/ligrec_restated.py) against pandas, the quantisation error
bound on log-normalised input, the host arithmetic of ``ligrec`` and its request checks.  No GPU: every ``ligrec`` call
here is rejected before any device work."""
import numpy as np
import pandas as pd
import pytest

import ligrec_restated as lr
from conftest import make_adata, synth


def _labels(n, K, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, K, n)
    codes[:K] = np.arange(K)          # no empty cluster
    return codes


def test_restated_sums_match_pandas_groupby():
    rng = np.random.default_rng(0)
    n, K = 60, 4
    X = np.column_stack([rng.poisson(2.0, n), rng.poisson(0.3, n), np.zeros(n), rng.normal(0, 3, n), rng.uniform(0, 1e-3, n)])
    codes = _labels(n, K, 1)
    s = lr.shifts(X)
    assert list(s[:3]) == [0, 0, 0] and s[3] != 0 and s[4] == 32 - (-9)      # 2^-10 <= max < 2^-9 for uniform(0, 1e-3)
    S, N, n_c = lr.tables(X, codes, K, s)
    frame = pd.DataFrame(X).groupby(codes)
    want_mean = frame.mean().to_numpy()
    got_mean = np.ldexp(S.astype(np.float64), -s.astype(np.int64)[None, :]) / n_c[:, None]
    np.testing.assert_array_equal(got_mean[:, :3], want_mean[:, :3])          # counts: exact
    # floats: half a grid step 2^-s per value, plus the rounding of pandas' own float64 sum (n = 60 values)
    bound = np.ldexp(0.5, -s[3:].astype(np.int64)) + 64 * 2.0 ** -53 * np.abs(X[:, 3:]).max(axis=0)
    assert np.all(np.abs(got_mean[:, 3:] - want_mean[:, 3:]) <= bound[None, :])
    np.testing.assert_array_equal(N, pd.DataFrame(X > 0).groupby(codes).sum().to_numpy())
    np.testing.assert_array_equal(n_c, frame.size().to_numpy())


def test_restated_comparison_is_the_comparison_of_means():
    """On tiny integer input the exact integer decision equals the comparison of the permuted and observed means taken as
    exact fractions."""
    from fractions import Fraction

    rng = np.random.default_rng(3)
    n, K = 12, 3
    X = rng.poisson(1.5, (n, 3)).astype(np.float64)
    X[:, 2] = X[:, 2] / 4 + 0.125                                              # a float gene: another shift
    codes = _labels(n, K, 4)
    perms = np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(20)])
    pairs = [(0, 1), (1, 0), (2, 2), (0, 2)]
    r = lr.restated(X, codes, K, pairs, perms)
    assert r["shift"][2] != 0
    n_c = r["group_n"]

    def mean(labels, c, g):
        return sum(Fraction(float(X[i, g])) for i in range(n) if labels[i] == c) / int(n_c[c])

    for i, (L, R) in enumerate(pairs):
        for a in range(K):
            for b in range(K):
                obs = mean(codes, a, L) + mean(codes, b, R)
                want = sum(1 for p in perms if mean(codes[p], a, L) + mean(codes[p], b, R) >= obs)
                assert r["count_ge"][i, a, b] == want
    assert np.all(r["count_ge"] >= 1)                                          # the identity row always counts


def test_quantised_mean_error_on_log_normalised_float32():
    """|restated mean - np.mean in float64| <= 2^(e_g - 33) + 64 * 2^-53 * max|x|: half a grid step per value, plus numpy's
    pairwise summation."""
    _, X = synth(3000, 12, seed=5, sparse_x=False, normalize=True)
    assert X.dtype == np.float32
    codes = _labels(X.shape[0], 5, 6)
    s = lr.shifts(X)
    assert np.all(s != 0)
    S, _, n_c = lr.tables(X, codes, 5, s)
    got = np.ldexp(S.astype(np.float64), -s.astype(np.int64)[None, :]) / n_c[:, None]
    X64 = X.astype(np.float64)
    top = np.abs(X64).max(axis=0)
    bound = np.ldexp(1.0, (32 - s.astype(np.int64)) - 33) + 64 * 2.0 ** -53 * top
    for c in range(5):
        diff = np.abs(got[c] - X64[codes == c].mean(axis=0))
        print("cluster", c, "max |diff|", diff.max(), "bound", bound.min())
        assert np.all(diff <= bound)


def test_host_statistics_match_restatement():
    from spatialcore_amd.spatial.neighborhoods import ligrec_adjust, ligrec_shifts, ligrec_statistics
    from scipy import sparse

    rng = np.random.default_rng(7)
    n, K = 200, 4
    X = np.column_stack([rng.poisson(0.4, n), rng.poisson(3.0, n), rng.normal(0, 1, n), np.log1p(rng.poisson(1.0, n) / 3.0),
                         np.zeros(n)])
    codes = _labels(n, K, 8)
    pairs = [(0, 1), (2, 3), (3, 3), (4, 0), (1, 2)]
    perms = np.stack([rng.permutation(n) for _ in range(25)])
    r = lr.restated(X, codes, K, pairs, perms, threshold=0.3)
    np.testing.assert_array_equal(ligrec_shifts(X), r["shift"])
    np.testing.assert_array_equal(ligrec_shifts(sparse.csr_matrix(X)), r["shift"])
    cps = [(a, b) for a in range(K) for b in range(K)]
    ge = r["count_ge"].reshape(len(pairs), K * K)
    means, pvals = ligrec_statistics(r["sum"], r["nnz"], r["group_n"], r["shift"], pairs, cps, ge, len(perms), 0.3)
    np.testing.assert_array_equal(means, r["means"])
    np.testing.assert_array_equal(pvals, r["pvalues"])
    assert np.isnan(pvals).any() and not np.isnan(pvals).all()
    for method in ("fdr_bh", "bonferroni"):
        for axis in ("clusters", "interactions"):
            np.testing.assert_array_equal(ligrec_adjust(pvals, method, axis), lr.adjust(pvals, method, axis))
    bh = ligrec_adjust(pvals, "fdr_bh", "clusters")
    ok = ~np.isnan(pvals)
    assert np.all(bh[ok] >= pvals[ok]) and np.all(bh[ok] <= 1) and np.array_equal(np.isnan(bh), ~ok)
    assert ligrec_statistics(r["sum"], r["nnz"], r["group_n"], r["shift"], pairs, cps, ge, 0, 0.3)[1] is None


def test_threshold_edge_keeps_one_in_a_hundred():
    """A cluster of 100 cells with exactly one expressing: kept at threshold 0.01 (1 / 100 >= 0.01), dropped at 0.011."""
    from spatialcore_amd.spatial.neighborhoods import ligrec_statistics

    n = 150
    codes = np.array([0] * 100 + [1] * 50)
    X = np.zeros((n, 2))
    X[7, 0] = 3.0
    X[100:, 1] = 1.0
    pairs, perms = [(0, 1)], np.stack([np.arange(n)] * 4)
    for threshold, kept in ((0.01, True), (0.011, False)):
        r = lr.restated(X, codes, 2, pairs, perms, threshold=threshold)
        _, pvals = ligrec_statistics(r["sum"], r["nnz"], r["group_n"], r["shift"], pairs, [(0, 1)], r["count_ge"][:, 0, 1][:, None],
                                     4, threshold)
        assert np.isnan(pvals[0, 0]) != kept and np.isnan(r["pvalues"][0, 1]) != kept
        if kept:
            assert pvals[0, 0] == 1.0


class _Comm:
    world, rank = 2, 0


def _adata(n=40, G=4, K=3):
    rng = np.random.default_rng(11)
    X = rng.poisson(1.0, (n, G)).astype(np.float64)
    return make_adata(rng.uniform(0, 10, (n, 2)), X, labels=np.array(list("abc"))[_labels(n, K, 12)])


@pytest.mark.parametrize("kwargs, match", [
    (dict(interactions=[("g0", "nope"), ("zz", "g1")]), "no interaction is left"),
    (dict(interactions=None), "interactions is required"),
    (dict(interactions=[("g0", "g1")], comm=_Comm()), "rng='philox'"),
    (dict(interactions=[("g0", "g1")], corr_axis="genes"), "corr_axis"),
    (dict(interactions=[("g0", "g1")], corr_method="holm"), "corr_method"),
    (dict(interactions=[("g0", "g1")], clusters=["a", "q"]), "not categories"),
    (dict(interactions=[("g0", "g1")], clusters=[("a", "b"), ("b", "q")]), "not categories"),
    (dict(interactions=[("g0", "g1")], n_perms=-1), "n_perms"),
    (dict(interactions=[("g0", "g1")], rng="mt"), "rng must be"),
    (dict(interactions=[("g0", "g1")], gene_batch=1), "gene_batch"),
    (dict(interactions=pd.DataFrame({"ligand": ["g0"], "receptor": ["g1"]})), "'source' and 'target'"),
])
def test_request_checks(kwargs, match):
    from spatialcore_amd.spatial import ligrec

    with pytest.raises(ValueError, match=match):
        ligrec(_adata(), "cell_type", **kwargs)
    with pytest.raises(ValueError, match="not found in adata.obs"):
        ligrec(_adata(), "nothing", interactions=[("g0", "g1")])


def test_shift_spread_beyond_30_names_the_genes():
    from spatialcore_amd.spatial import ligrec

    ad = _adata()
    ad.X[:, 1] = ad.X[:, 1] * 1e-12 + 1e-13          # a float gene with max < 2^-36: shift >= 68, against shift 0
    with pytest.raises(ValueError, match=r"interaction \(g0, g1\).*differ by more than 30"):
        ligrec(ad, "cell_type", interactions=[("g2", "g3"), ("g0", "g1")])
    ad.X[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ligrec(ad, "cell_type", interactions=[("g2", "g3")])


def test_interaction_parsing_and_batches():
    from spatialcore_amd.spatial.neighborhoods import _ligrec_batches, _ligrec_cluster_pairs, _ligrec_interactions

    frame = pd.DataFrame({"source": ["g0", "g1", "g0", "g9"], "target": ["g1", "g1", "g1", "g0"], "db": ["x", "y", "z", "w"]})
    pairs, meta, dropped = _ligrec_interactions(frame, pd.Index(["g0", "g1", "g2"]))
    assert pairs == [("g0", "g1"), ("g1", "g1")] and dropped == 1
    assert list(meta["db"]) == ["x", "y"] and list(meta.index) == pairs
    assert _ligrec_interactions([("g0", "g1"), ("g0", "g1")], pd.Index(["g0", "g1"]))[:2] == ([("g0", "g1")], None)
    pairs_idx = [(0, 1), (1, 2), (3, 4), (4, 4), (0, 5)]
    for cap in (2, 3, 4, 6):
        batches = _ligrec_batches(pairs_idx, cap)
        assert sorted(i for _, rows in batches for i in rows) == list(range(5))
        for genes, rows in batches:
            assert len(genes) <= cap and all(pairs_idx[i][0] in genes and pairs_idx[i][1] in genes for i in rows)
    assert _ligrec_cluster_pairs(None, ["a", "b"]) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert _ligrec_cluster_pairs(["b"], ["a", "b"]) == [(1, 1)]
    assert _ligrec_cluster_pairs([("b", "a"), ("b", "a")], ["a", "b"]) == [(1, 0)]


def test_exports():
    from spatialcore_amd import _lib, spatial

    assert "ligrec" in spatial.__all__ and callable(spatial.ligrec)
    assert _lib.K_LIGREC == 18
    assert "sc_ligrec_counts" in _lib.SYMBOLS and "sc_ligrec_counter" in _lib.SYMBOLS
