"""The restatement of Getis-Ord and local Geary (tests/local_stats_restated.py) pinned to the textbook formulas, and the
request validation of the two public functions -- all without a device.  Only then is the restatement fit to judge the
GPU (tests/test_gpu_local_stats.py)."""
import numpy as np
import pytest

import local_stats_restated as ls
from conftest import make_adata

EPS32 = float(np.finfo(np.float32).eps)
N, K = 700, 6


@pytest.fixture(scope="module")
def lists(oracle):
    return oracle.knn_bruteforce(ls.uniform_coords(N, 2), K)


def inputs():
    return (("counts", ls.count_matrix(N, 5, 3)), ("lognorm", ls.lognorm_matrix(N, 5, 4)))


def arrays(X, graph):
    ip, ix, w = graph
    z, lag, _, zero = ls.local_moran_arrays(X, X.dtype.type, ip, ix, w.astype(np.float32))
    assert not zero.any()
    return z, lag


def test_star_graph_holds_the_self_edge_mid_row(lists):
    ip, ix, w = ls.stat_graph("getis_star", lists, K)
    rows = ix.reshape(N, K + 1)
    assert (rows == np.arange(N)[:, None]).sum(axis=1).tolist() == [1] * N and (np.diff(rows, axis=1) > 0).all()
    assert ((rows[:, 0] < np.arange(N)) & (rows[:, -1] > np.arange(N))).any()
    assert (w == float(np.float32(1) / np.float32(K + 1))).all()


def test_gi_star_is_the_textbook_formula(lists):
    """Gi* = (sum_j w_ij x_j - xbar W_i) / (s sqrt((n S1_i - W_i^2) / (n - 1))) on x = z with xbar = 0 and s = 1 (z units:
    what a z-score has by construction), every sum in float64.  The float32 accumulation of the neighbourhood sum and
    the float32 store are then the only differences: deg products and deg sums of relative error eps32 / 2 each and one
    store, below (deg + 1) eps32 sum_e w_e |z_e| / den_i."""
    graph = ls.stat_graph("getis_star", lists, K)
    ip, ix, w = graph
    for name, X in inputs():
        z, lag = arrays(X, graph)
        got = ls.getis_values(ip, ix, w, z, lag, True).astype(np.float64)
        z64 = z.astype(np.float64)
        W, S1 = ls.row_weight_sums(ip, ix, w)
        den = np.sqrt((N * S1 - W * W) / (N - 1))[:, None]
        want = (ls.row_sequential(ip, ix, w, z64) - 0.0 * W[:, None]) / (1.0 * den)
        bound = (np.diff(ip)[:, None] + 1) * EPS32 * ls.row_sequential(ip, ix, w, np.abs(z64)) / den
        assert (np.abs(got - want) <= bound).all(), name
        assert np.abs(got).max() > 1.0
        # with the float64 mean and sd of the float32 z instead of 0 and 1: two more terms, |xbar| W / (s den) and |1 / s - 1| |G|
        xbar, s = z64.mean(axis=0), z64.std(axis=0)
        textbook = (ls.row_sequential(ip, ix, w, z64) - xbar * W[:, None]) / (s * den)
        assert (np.abs(got - textbook) <= bound + np.abs(xbar) * W[:, None] / (s * den) + np.abs(1 / s - 1) * np.abs(want) + 1e-15).all(), name


def test_gi_reduces_to_ord_and_getis(lists):
    """Gi with x_bar(i), s(i) taken over the other n - 1 cells, from the raw definition in float64 on x = z with sum z = 0
    and sum z^2 = n: the same number as the mi / vi form, within the float32 accumulation and store plus the distance
    of the float32 z-scores' moments from 0 and 1 (below 1e-5 here)."""
    graph = ls.stat_graph("getis", lists, K)
    ip, ix, w = graph
    for name, X in inputs():
        z, lag = arrays(X, graph)
        got = ls.getis_values(ip, ix, w, z, lag, False).astype(np.float64)
        z64 = z.astype(np.float64)
        W, S1 = ls.row_weight_sums(ip, ix, w)
        xbar_i = (z64.sum(axis=0) - z64) / (N - 1)
        s2_i = ((z64 ** 2).sum(axis=0) - z64 ** 2) / (N - 1) - xbar_i ** 2
        den = np.sqrt(s2_i) * np.sqrt(((N - 1) * S1 - W * W) / (N - 2))[:, None]
        want = (ls.row_sequential(ip, ix, w, z64) - W[:, None] * xbar_i) / den
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg=name)


def test_geary_is_the_expanded_square(lists):
    """C_i = z_i^2 W_i - 2 z_i lag_i + lag(z^2)_i in float64.  The float32 form rounds d (eps32 / 2), d d (once more, on
    twice the error), the product with w and deg sums: 4.5 eps32 at 6 edges, below 8 eps32 sum_e w_e (|z_i| + |z_e|)^2."""
    graph = ls.stat_graph("geary", lists, K)
    ip, ix, w = graph
    for name, X in inputs():
        z, _ = arrays(X, graph)
        got = ls.geary_values(ip, ix, w, z).astype(np.float64)
        z64 = z.astype(np.float64)
        W, _ = ls.row_weight_sums(ip, ix, w)
        want = z64 ** 2 * W[:, None] - 2 * z64 * ls.row_sequential(ip, ix, w, z64) + ls.row_sequential(ip, ix, w, z64 ** 2)
        a = np.abs(z64)
        bound = 8 * EPS32 * (a ** 2 * W[:, None] + 2 * a * ls.row_sequential(ip, ix, w, a) + ls.row_sequential(ip, ix, w, a ** 2))
        assert (np.abs(got - want) <= bound).all(), name
        assert (got >= 0).all() and got.max() > 1.0


def test_geary_expectation_is_the_permutation_mean(lists):
    """The mean of the permuted C over 400 permutations approaches E_i: within 5 standard errors of that mean, per cell
    and gene.  On a graph with unequal weights, unequal degrees and empty rows too."""
    rng = np.random.default_rng(5)
    perms = np.stack([rng.permutation(N) for _ in range(400)])
    X = ls.lognorm_matrix(N, 3, 4, lam=(2.0, 6.0))
    for graph in (ls.stat_graph("geary", lists, K), ls.thinned_csr(lists, seed=4, empty_every=9)):
        ip, ix, w = graph
        z, _ = arrays(X, graph)
        sims = np.stack([ls.geary_values(ip, ix, w, z[p]) for p in perms]).astype(np.float64)
        E = ls.geary_expectation(ip, ix, w)[:, None]
        se = sims.std(axis=0, ddof=1) / np.sqrt(len(perms))
        assert (np.abs(sims.mean(axis=0) - E) <= 5 * se).all()
        empty = np.diff(ip) == 0
        assert (E[empty] == 0).all() and (sims[:, empty] == 0).all()
    ip, ix, w = ls.stat_graph("getis_star", lists, K)     # a self edge contributes nothing to C and nothing to E
    assert np.allclose(ls.geary_expectation(ip, ix, w), 2.0 * N / (N - 1) * K / (K + 1), rtol=1e-6)


@pytest.mark.parametrize("stat", ls.STATS)
def test_counts_identity_and_ties(lists, stat):
    """An identity permutation adds exactly 1 to both tails everywhere; ge + le - P is the number of exact ties.  On
    count_matrix(700, 17, 12) with k = 6 and P = 9 at least 3 % of all comparisons are exact ties (measured: 5.7 to
    6.5 % over the three statistics), so the tie path is what the GPU tests exercise."""
    P = 9
    X = ls.count_matrix(N, 17, 12)
    graph = ls.stat_graph(stat, lists, K)
    ip, ix, w = graph
    rng = np.random.default_rng(6)
    perms = np.stack([rng.permutation(N) for _ in range(P)]).astype(np.int32)
    want = ls.restated(stat, X, graph, perms)
    obs = want["stat"] if stat == "geary" else want["lag"]
    ties = sum((ls.simulated(stat, ip, ix, w, want["z"][p]) == obs).astype(np.int64) for p in perms)
    np.testing.assert_array_equal(want["ge"] + want["le"] - P, ties)
    share = ties.sum() / (P * ties.size)
    print(f"{stat}: exact ties in {100 * share:.2f} % of comparisons")
    assert share >= 0.03
    with_ident = np.concatenate([perms[:4], np.arange(N, dtype=np.int32)[None], perms[4:]])
    ge2, le2 = ls.two_tail_counts(stat, ip, ix, w, want["z"], obs, with_ident)
    np.testing.assert_array_equal(ge2, want["ge"] + 1)
    np.testing.assert_array_equal(le2, want["le"] + 1)
    # the fold of a one-sided count is not the two-tail level wherever ties sit on one side
    folded, level = np.minimum(want["ge"], P - want["ge"]), np.minimum(want["ge"], want["le"])
    assert (folded != level).mean() > 0.1


def test_classes():
    G = np.array([[1.0, -2.0, 0.0, 3.0], [-1.0, 2.0, 5.0, -3.0]], dtype=np.float32)
    padj = np.array([[0.01, 0.01, 0.01, 0.05], [0.2, 0.049, 0.01, 0.01]], dtype=np.float32)
    zero = np.array([False, False, False, False])
    assert ls.spot_classes(G, padj, 0.05, zero).tolist() == [[1, 2, 0, 0], [0, 1, 1, 2]]
    assert ls.spot_classes(G, None, 0.05, np.array([True, False, False, False])).tolist() == [[0, 2, 0, 1], [0, 1, 1, 2]]
    C = np.array([[0.5, 0.5, 0.5, 2.0], [1.0, 0.5, 0.5, 0.5]], dtype=np.float32)
    E = np.array([1.0, 1.0])
    z = np.array([[1, -1, 1, 1], [1, 0, -1, 1]], dtype=np.float32)
    lag = np.array([[1, -1, -1, 1], [1, 1, -1, 1]], dtype=np.float32)
    assert ls.geary_classes(C, E, z, lag, None, 0.05, zero).tolist() == [[1, 2, 3, 4], [0, 3, 2, 1]]
    assert ls.geary_classes(C, E, z, lag, padj, 0.05, zero).tolist() == [[1, 2, 3, 0], [0, 3, 2, 1]]


# ---- request validation of the public functions: before the first device call --------------------------------------------

def functions():
    from spatialcore_amd.spatial import local_gearys_c, local_getis_ord
    return local_getis_ord, local_gearys_c


@pytest.fixture
def no_device(monkeypatch):
    from spatialcore_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a device context was asked for before the request was validated")
    monkeypatch.setattr(_lib, "default_context", refuse)


@pytest.mark.parametrize("which", [0, 1])
def test_request_validation(no_device, which):
    fn = functions()[which]
    ad = make_adata(ls.uniform_coords(50, 1), ls.count_matrix(50, 4, 1))
    with pytest.raises(ValueError, match=r"adata.obsm\['nowhere'\] not found"):
        fn(ad, spatial_key="nowhere")
    with pytest.raises(ValueError, match="Invalid fdr_correction: 'holm'"):
        fn(ad, fdr_correction="holm")
    with pytest.raises(ValueError, match="n_permutations must be <= 65535, got 65536"):
        fn(ad, n_permutations=65536)
    with pytest.raises(ValueError, match="n_permutations must be >= 0, got -1"):
        fn(ad, n_permutations=-1)
    with pytest.raises(ValueError, match="n_neighbors must be >= 1"):
        fn(ad, n_neighbors=0)
    with pytest.raises(ValueError, match="Genes not found"):
        fn(ad, genes=["nope"])
    with pytest.raises(AssertionError, match="a device context was asked for"):
        fn(ad, n_permutations=65535)          # the largest request passes validation


def test_exports_and_defaults():
    import inspect

    from spatialcore_amd import spatial
    getis, geary = functions()
    assert "local_getis_ord" in spatial.__all__ and "local_gearys_c" in spatial.__all__
    pg, pc = inspect.signature(getis).parameters, inspect.signature(geary).parameters
    assert pg["star"].default is True and pg["key_added"].default == "local_getis" and pc["key_added"].default == "local_geary"
    assert [k for k in pg if k != "star"] == list(pc)
    assert pg["device"].kind is inspect.Parameter.KEYWORD_ONLY
