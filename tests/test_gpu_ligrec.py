"""GPU: ligrec (extension, N10) against the plain restatement of its definition (tests/ligrec_restated.py).

Every comparison is exact: ``==`` on every integer (sum, nnz, group_n, every null table, count_ge), ``==`` on ``means`` and
NaN-pattern-equal plus ``==`` on ``pvalues``.  There is no reference fixture: the reference has no such function and
squidpy is not a dependency, so the definition in include/spatialcore_hip.h, restated in ligrec_restated.py, is the pin.
"""
import numpy as np
import pandas as pd
import pytest

import ligrec_restated as lr
from conftest import make_adata, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from spatialcore_amd import _lib

    with _lib.Context(0) as c:
        yield c


def _codes(n, K, seed, singleton=False):
    """Labels in [0, K) with every cluster present while n allows it; ``singleton``: cluster K - 1 has exactly one cell."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, K - 1 if (singleton and K > 1) else K, n)
    codes[:min(n, K)] = np.arange(min(n, K))
    if singleton and K > 1 and n >= K:
        codes[codes == K - 1] = 0
        codes[K - 1] = K - 1
    return codes.astype(np.int32)


def _mixed(n, G, seed):
    """G genes of mixed value classes within every 16-gene tile: all zeros, counts up to 255, with a 256, with 65535, with
    65536, float32 log-normalised, float64 with negatives, sparse counts; one cell of all zeros."""
    rng = np.random.default_rng(seed)
    cols = []
    for g in range(G):
        kind = g % 8
        if kind == 0 and g > 0:
            col = np.zeros(n)
        elif kind in (0, 1):
            col = np.minimum(rng.poisson(3.0, n), 255).astype(np.float64)
            col[rng.integers(0, n)] = 255
        elif kind == 2:
            col = rng.poisson(0.2, n).astype(np.float64)
            col[rng.integers(0, n)] = 256
        elif kind == 3:
            col = rng.poisson(40.0, n).astype(np.float64)
            col[rng.integers(0, n)] = 65535
        elif kind == 4:
            col = rng.poisson(0.05, n).astype(np.float64)
            col[rng.integers(0, n)] = 65536
        elif kind == 5:
            col = np.log1p(rng.poisson(1.0, n) / rng.uniform(0.5, 1.5, n)).astype(np.float32).astype(np.float64)
        elif kind == 6:
            col = rng.normal(0, 2.5, n)
        else:
            col = rng.poisson(0.02, n).astype(np.float64)
        cols.append(col)
    X = np.column_stack(cols)
    if n > 2:
        X[n // 2, :] = 0.0
    return X


def _pairs(X, seed, count=8):
    """Interactions over the genes of X: a gene with itself, one gene in several interactions, the rest at random; a pair
    whose shifts differ by more than 30 (a raw-count gene with a float gene below 2) is left out, as the entry point
    refuses it."""
    G = X.shape[1]
    s = lr.shifts(X)
    rng = np.random.default_rng(seed)
    pairs = [(0, 0), (0, G - 1), (G - 1, 0), (G // 2, 0), (G - 1, G - 1)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(0, G, (count, 2))]
    return [(a, b) for a, b in dict.fromkeys(pairs) if abs(int(s[a]) - int(s[b])) <= 30]


def _table(n, P, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(P)]).astype(np.int32) if P else np.zeros((0, n), np.int32)


def _check(ctx, X, codes, K, pairs, perms, row0=0, rows=None):
    """ctx.ligrec_counts on rows [row0, row0 + rows) of the uploaded table against the restatement."""
    rows = len(perms) - row0 if rows is None else rows
    want = lr.restated(X, codes, K, pairs, perms[row0:row0 + rows])
    ctx.set_expression(X, np.arange(X.shape[1]))
    if len(perms):
        ctx.set_permutations(perms)
    got = ctx.ligrec_counts(codes, K, want["shift"], [l for l, _ in pairs], [r for _, r in pairs], rows, row0, return_null_sums=True)
    for key in ("sum", "nnz", "group_n", "null_sums", "count_ge"):
        assert got[key].dtype == np.int64
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    return got, want


# n, K, G, n_perm, singleton cluster -- every n, K, G and n_perm of the issue, the K at which the kernel changes its
# permutations per pass (32 | 33, 64 | 65) and an n beyond one 8192-cell workgroup range
SHAPES = [
    (1, 1, 1, 1, False),
    (2, 2, 1, 15, False),
    (255, 3, 16, 16, True),
    (256, 17, 17, 17, False),
    (257, 2, 33, 33, True),
    (4099, 96, 17, 17, True),
    (4099, 3, 33, 0, False),
    (700, 32, 16, 17, False),
    (700, 33, 17, 9, False),
    (700, 64, 16, 9, True),
    (700, 65, 17, 5, False),
    (8193, 17, 33, 16, False),
    (16385, 3, 1, 1, False),
]


@pytest.mark.parametrize("n, K, G, P, singleton", SHAPES)
def test_counts_match_restatement(ctx, n, K, G, P, singleton):
    X = _mixed(n, G, seed=n + G)
    codes = _codes(n, K, seed=K, singleton=singleton)
    if singleton:
        assert np.bincount(codes, minlength=K)[K - 1] == 1
    got, want = _check(ctx, X, codes, K, _pairs(X, seed=P), _table(n, P, seed=n + P))
    if P:
        assert got["count_ge"].max() <= P


def test_perm_row0_and_float32_sparse(ctx):
    from scipy import sparse

    n, K = 1500, 5
    _, Xs = synth(n, 20, seed=3, normalize=True)
    assert Xs.dtype == np.float32 and sparse.issparse(Xs)
    X = Xs.toarray().astype(np.float64)
    codes = _codes(n, K, 9)
    pairs, perms = _pairs(X, 1), _table(n, 30, 2)
    want = lr.restated(X, codes, K, pairs, perms[7:7 + 18])
    ctx.set_expression(Xs, np.arange(20))
    ctx.set_permutations(perms)
    got = ctx.ligrec_counts(codes, K, want["shift"], [l for l, _ in pairs], [r for _, r in pairs], 18, 7, return_null_sums=True)
    for key in ("sum", "nnz", "group_n", "null_sums", "count_ge"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    again = ctx.ligrec_counts(codes, K, want["shift"], [l for l, _ in pairs], [r for _, r in pairs], 18, 7, return_null_sums=True)
    for key in ("sum", "nnz", "group_n", "null_sums", "count_ge"):          # two calls in a row are identical
        np.testing.assert_array_equal(got[key], again[key], err_msg=key)


def test_ties_count(ctx):
    """The identity and a permutation that only swaps cells inside clusters tie with the observed table and count; one
    that moves mass out of the cluster does not."""
    n = 10
    codes = np.array([0] * 5 + [1] * 5, dtype=np.int32)
    X = np.zeros((n, 1))
    X[:5, 0] = [4, 0, 2, 7, 1]
    inside = np.array([1, 0, 3, 2, 4, 9, 8, 7, 6, 5])
    out = np.arange(n)
    out[[3, 8]] = [8, 3]                           # the cell holding 7 trades labels with a cell of cluster 1
    perms = np.stack([np.arange(n), inside, out]).astype(np.int32)
    got, _ = _check(ctx, X, codes, 2, [(0, 0)], perms)
    np.testing.assert_array_equal(got["null_sums"][:, :, 0], [[14, 0], [14, 0], [7, 7]])
    assert got["count_ge"][0, 0, 0] == 2 and got["count_ge"][0, 1, 1] == 3
    assert got["count_ge"][0, 0, 1] == 3 and got["count_ge"][0, 1, 0] == 3     # 5 * (-7) + 5 * 7 = 0: a tie, counted


def test_comparison_needs_128_bits(ctx):
    """n = 140 001, clusters of 70 000 and 70 001, one float gene with q = 2^31 in every cell of the first cluster.  The
    permutation that moves all of that mass makes n_b * dS exceed 2^63: Python integers decide."""
    n0, n1 = 70000, 70001
    n = n0 + n1
    codes = np.array([0] * n0 + [1] * n1, dtype=np.int32)
    X = np.zeros((n, 1))
    X[:n0, 0] = 0.5
    move = np.arange(n)
    move[:n0], move[n0:2 * n0] = np.arange(n0, 2 * n0), np.arange(n0)
    perms = np.stack([np.arange(n), move]).astype(np.int32)
    got, want = _check(ctx, X, codes, 2, [(0, 0)], perms)
    assert want["shift"][0] == 32 and want["sum"][0, 0] == n0 << 31
    assert n1 * abs(int(want["null_sums"][1, 0, 0]) - int(want["sum"][0, 0])) > 2 ** 63
    # (0, 1): 70001 * (-70000 * 2^31) + 70000 * (70000 * 2^31) < 0 -- two terms beyond 2^63 of opposite sign
    np.testing.assert_array_equal(got["count_ge"][0], [[1, 1], [1, 2]])


def test_counter_form_equals_counts_form(ctx):
    from spatialcore_amd import _lib

    n, K, G, P, seed = 3001, 7, 20, 40, 12345
    X = _mixed(n, G, 4)
    codes = _codes(n, K, 5)
    pairs = _pairs(X, 6)
    perms = _lib.perm_counter_host(seed, n, P)
    got, want = _check(ctx, X, codes, K, pairs, perms)
    args = (codes, K, want["shift"], [l for l, _ in pairs], [r for _, r in pairs])
    for batch in (16, 64):                          # 16 + 16 + 8 rows, and batch > n_perm
        r = ctx.ligrec_counter(*args, seed, 0, P, batch)
        for key in ("sum", "nnz", "group_n", "count_ge"):
            np.testing.assert_array_equal(r[key], want[key], err_msg=f"{key} batch={batch}")
    a = ctx.ligrec_counter(*args, seed, 0, 13, 16)
    b = ctx.ligrec_counter(*args, seed, 13, 27, 16)
    np.testing.assert_array_equal(a["count_ge"] + b["count_ge"], want["count_ge"])
    zero = ctx.ligrec_counter(*args, seed, 0, 0, 16)
    np.testing.assert_array_equal(zero["sum"], want["sum"])
    assert not zero["count_ge"].any()


def test_gene_results_do_not_depend_on_company(ctx):
    n, K, G = 2000, 6, 40
    X = _mixed(n, G, 8)
    codes = _codes(n, K, 9)
    perms = _table(n, 20, 10)
    pairs = [(3, 6), (6, 6), (11, 3)]             # counts with a float64 gene, the float gene with itself, counts with counts
    got, want = _check(ctx, X, codes, K, pairs, perms)
    sub = [3, 6, 11]
    ctx.set_expression(X, np.array(sub))
    alone = ctx.ligrec_counts(codes, K, want["shift"][sub], [0, 1, 2], [1, 1, 0], 20, return_null_sums=True)
    np.testing.assert_array_equal(alone["sum"], got["sum"][:, sub])
    np.testing.assert_array_equal(alone["nnz"], got["nnz"][:, sub])
    np.testing.assert_array_equal(alone["null_sums"], got["null_sums"][:, :, sub])
    np.testing.assert_array_equal(alone["count_ge"], got["count_ge"])


def test_leaves_graph_pair_list_and_expression(ctx):
    n, K = 1200, 4
    coords, X = synth(n, 18, seed=13, sparse_x=False)
    codes = _codes(n, K, 14)
    perms = _table(n, 6, 15)
    ctx.knn(coords, 6, fetch=False)
    ctx.graph_from_knn(1.0)
    ctx.ripley_build(coords, [8.0, 15.0])
    ctx.set_expression(X, np.arange(18))
    ctx.set_permutations(perms)

    def state():
        return (ctx.enrichment_counts(codes, K, 6), ctx.ripley_counts(codes, K, 6), ctx.get_graph(), *ctx.expr_stats())

    before = state()
    s = lr.shifts(X)
    r1 = ctx.ligrec_counts(codes, K, s, [0, 1], [2, 1], 6)
    r2 = ctx.ligrec_counter(codes, K, s, [0, 1], [2, 1], 3, 0, 6, 4)
    ctx.set_permutations(perms)                     # (the counter form leaves no table, like its siblings)
    after = state()
    for a, b in zip(before[:2] + before[3:], after[:2] + after[3:]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(before[2], after[2]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(r1["sum"], r2["sum"])
    np.testing.assert_array_equal(ctx.ligrec_counts(codes, K, s, [0, 1], [2, 1], 6)["count_ge"], r1["count_ge"])


def test_errors(ctx):
    from spatialcore_amd import _lib

    n, K = 300, 3
    X = _mixed(n, 5, 1)
    codes = _codes(n, K, 2)
    s = lr.shifts(X)
    ctx.set_expression(X, np.arange(5))
    with pytest.raises(ValueError, match=r"n_types must be 1\.\.96, got 97"):
        ctx.ligrec_counts(codes, 97, s, [0], [1], 0)
    bad = codes.copy()
    bad[17] = K
    with pytest.raises(ValueError, match="label 3 of cell 17 out of range"):
        ctx.ligrec_counts(bad, K, s, [0], [1], 0)
    with pytest.raises(ValueError, match="299 labels for 300 loaded cells"):
        ctx.ligrec_counts(codes[:-1], K, s, [0], [1], 0)
    with pytest.raises(ValueError, match="outside the 5 loaded genes"):
        ctx.ligrec_counts(codes, K, s, [0], [5], 0)
    spread = s.copy()
    spread[1] = s[0] + 31
    with pytest.raises(ValueError, match="differ by more than 30"):
        ctx.ligrec_counts(codes, K, spread, [0], [1], 0)
    Xn = X.copy()
    Xn[5, 2] = np.nan
    ctx.set_expression(Xn, np.arange(5))
    with pytest.raises(ValueError, match="gene 2 has a value that is not finite"):
        ctx.ligrec_counts(codes, K, s, [0], [1], 0)
    Xb = X.copy()
    Xb[5, 3] = 2.0 ** 33                          # with shift 0 of a count gene: rint(x) leaves (-2^32, 2^32)
    ctx.set_expression(Xb, np.arange(5))
    with pytest.raises(ValueError, match="gene 3 has a value"):
        ctx.ligrec_counter(codes, K, s, [0], [1], 1, 0, 4, 4)
    with _lib.Context(0) as fresh:
        with pytest.raises(_lib.SpatialCoreHipError, match="no expression loaded"):
            fresh.ligrec_counts(codes, K, s[:1], [0], [0], 0)


# ---- the public function -------------------------------------------------------------------------------------------


def _public_case(n=1800, G=60, K=5, seed=21, normalize=False):
    coords, X = synth(n, G, seed=seed, normalize=normalize)
    labels = np.array([f"c{k}" for k in range(K)])[_codes(n, K, seed + 1)]
    rng = np.random.default_rng(seed + 2)
    names = [f"g{i}" for i in range(G)]
    inter = [(names[a], names[b]) for a, b in rng.integers(0, G, (40, 2))] + [("g1", "g1"), ("g1", "g2"), ("g2", "g1")]
    inter = list(dict.fromkeys(inter))
    return coords, X, labels, inter


def _want(X, labels, inter, perms, threshold=0.01, cluster_pairs=None):
    cats = sorted(set(labels.tolist()))
    codes = np.array([cats.index(v) for v in labels.tolist()])
    dense = np.asarray(X.toarray() if hasattr(X, "toarray") else X, dtype=np.float64)
    pairs = [(int(a[1:]), int(b[1:])) for a, b in inter]
    return cats, lr.restated(dense, codes, len(cats), pairs, perms, threshold, cluster_pairs)


def _frames_equal(res, cats, want, inter, cluster_pairs=None, pvalues=None):
    cps = cluster_pairs or [(a, b) for a in range(len(cats)) for b in range(len(cats))]
    index = pd.MultiIndex.from_tuples(inter, names=["source", "target"])
    columns = pd.MultiIndex.from_tuples([(cats[a], cats[b]) for a, b in cps], names=["cluster_1", "cluster_2"])
    for key in ("means", "count_ge") + (("pvalues",) if want["pvalues"] is not None else ()):
        assert res[key].index.equals(index) and res[key].columns.equals(columns), key
    np.testing.assert_array_equal(res["means"].to_numpy(), want["means"])
    ge = want["count_ge"][:, [a for a, _ in cps], [b for _, b in cps]]
    assert res["count_ge"].to_numpy().dtype == np.int64
    np.testing.assert_array_equal(res["count_ge"].to_numpy(), ge)
    if want["pvalues"] is None:
        assert "pvalues" not in res
        return
    expect = want["pvalues"] if pvalues is None else pvalues
    got = res["pvalues"].to_numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(expect))
    np.testing.assert_array_equal(got[~np.isnan(got)], expect[~np.isnan(expect)])


@pytest.mark.parametrize("rng_name, sparse_x, normalize", [("numpy", True, False), ("numpy", False, True),
                                                           ("philox", True, True), ("philox", False, False)])
def test_public_function_matches_restatement(rng_name, sparse_x, normalize):
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import ligrec

    coords, X, labels, inter = _public_case(normalize=normalize)
    if not sparse_x:
        X = X.toarray()
    n, P, seed = X.shape[0], 37, 5
    if rng_name == "numpy":
        g = np.random.default_rng(seed)
        perms = np.stack([g.permutation(n) for _ in range(P)])
    else:
        perms = _lib.perm_counter_host(seed, n, P)
    cats, want = _want(X, labels, inter, perms, threshold=0.2)
    frame = pd.DataFrame({"source": [a for a, _ in inter] + ["g0", "nope"], "target": [b for _, b in inter] + ["zz", "g0"]})
    frame["note"] = np.arange(len(frame))
    frame = pd.concat([frame, frame.iloc[:3]])                          # duplicates are dropped
    ad = make_adata(coords, X, labels=labels)
    out = ligrec(ad, "cell_type", frame, n_perms=P, threshold=0.2, seed=seed, rng=rng_name, perm_batch=16)
    assert out is ad
    res = ad.uns["cell_type_ligrec"]
    _frames_equal(res, cats, want, inter)
    assert np.isnan(res["pvalues"].to_numpy()).any()
    assert list(res["metadata"]["note"]) == list(range(len(inter))) and res["metadata"].index.equals(res["means"].index)
    assert (res["n_perms"], res["seed"], res["rng"], res["clusters"]) == (P, seed, rng_name, cats)


def test_public_gene_batches_clusters_correction_copy_and_no_perms():
    from spatialcore_amd.spatial import ligrec

    coords, X, labels, inter = _public_case()
    n, P, seed = X.shape[0], 21, 8
    g = np.random.default_rng(seed)
    perms = np.stack([g.permutation(n) for _ in range(P)])
    cats, want = _want(X, labels, inter, perms, threshold=0.2)
    results = []
    for gene_batch in (16, 48, None):
        ad = make_adata(coords, X, labels=labels)
        ligrec(ad, "cell_type", inter, n_perms=P, threshold=0.2, seed=seed, gene_batch=gene_batch, perm_batch=8, key_added="lr")
        _frames_equal(ad.uns["lr"], cats, want, inter)
        results.append(ad.uns["lr"])
    for key in ("means", "count_ge", "pvalues"):
        assert results[0][key].equals(results[1][key]) and results[0][key].equals(results[2][key])

    cps = [(0, 1), (3, 3), (4, 0)]
    cats, sub = _want(X, labels, inter, perms, threshold=0.2, cluster_pairs=cps)
    ad = make_adata(coords, X, labels=labels)
    ligrec(ad, "cell_type", inter, clusters=[(cats[a], cats[b]) for a, b in cps], n_perms=P, threshold=0.2, seed=seed)
    _frames_equal(ad.uns["cell_type_ligrec"], cats, sub, inter, cluster_pairs=cps)
    cps2 = [(a, b) for a in (1, 2) for b in (1, 2)]
    ad = make_adata(coords, X, labels=labels)
    ligrec(ad, "cell_type", inter, clusters=[cats[1], cats[2]], n_perms=P, threshold=0.2, seed=seed)
    _frames_equal(ad.uns["cell_type_ligrec"], cats, _want(X, labels, inter, perms, 0.2, cps2)[1], inter, cluster_pairs=cps2)

    for axis in ("clusters", "interactions"):
        for method in ("fdr_bh", "bonferroni"):
            ad = make_adata(coords, X, labels=labels)
            ligrec(ad, "cell_type", inter, n_perms=P, threshold=0.2, seed=seed, corr_method=method, corr_axis=axis)
            _frames_equal(ad.uns["cell_type_ligrec"], cats, want, inter, pvalues=lr.adjust(want["pvalues"], method, axis))

    ad = make_adata(coords, X, labels=labels)
    out = ligrec(ad, "cell_type", inter, n_perms=P, threshold=0.2, seed=seed, copy=True)
    assert out is not ad and "cell_type_ligrec" not in ad.uns
    _frames_equal(out.uns["cell_type_ligrec"], cats, want, inter)

    ad = make_adata(coords, X, labels=labels)
    ligrec(ad, "cell_type", inter, n_perms=0, threshold=0.2)
    cats, none = _want(X, labels, inter, perms[:0], threshold=0.2)
    _frames_equal(ad.uns["cell_type_ligrec"], cats, none, inter)
    assert not ad.uns["cell_type_ligrec"]["count_ge"].to_numpy().any()
