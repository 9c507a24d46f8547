"""GPU: the per-cell permutation counts of local Moran and local Lee against their plain restatement
(tests/local_restated.py, pinned to scipy, the oracle and the goldens by tests/test_cpu_local_restated.py).

Every comparison is ``==`` unless a test says otherwise.  The permutation tables are the tests' own (rows of numpy's
stream plus hand-made rows, uploaded with ``set_permutations``), so the expected counts never come from the library.
The edges: 16-gene tiles and 128-gene code-row groups; the quads of 4 and launches of 32 permutations of the code-row
kernels and the batches of 8 of the float-row kernels; 32 / 64 cells per workgroup and the 512-cell blocks of the
column compaction; unequal weights, unequal degrees, empty rows, negative values; the value 31 / 32 switch between the
two forms; the LDS switch of the histogram between 767 and 768 permutations; a count above 65535 in its 32-bit word; the
batches of 16 of local Lee.
"""
import numpy as np
import pytest
from scipy import sparse

import local_restated as lr
from conftest import make_adata, synth

pytestmark = pytest.mark.gpu

K = 6
FIELDS = ("z", "lag", "I", "count")
_TABLES = {}


@pytest.fixture(scope="module")
def ctx():
    # the process-wide context the public functions use (see tests/test_gpu_kernels.py)
    from spatialcore_amd import _lib

    c = _lib.default_context(0)
    yield c
    c.set_permgen_mode(0)


def table(oracle, n, rows, seed=77):
    """``rows`` consecutive permutations of numpy's stream, computed once per (n, rows, seed) and never written to."""
    key = (n, rows, seed)
    if key not in _TABLES:
        _TABLES[key] = oracle.perm_table(seed, n, rows)[0]
        _TABLES[key].setflags(write=False)
    return _TABLES[key]


def knn_graph(ctx, coords, k=K):
    """The row-normalised kNN graph on the device; returns its CSR arrays, built here from the neighbour lists."""
    idx = ctx.knn(coords, k)
    ctx.graph_from_knn(lr.knn_weight(k))
    return lr.knn_csr(idx, lr.knn_weight(k))


def csr_graph(ctx, graph, n):
    ctx.set_graph_csr(*graph, n)
    return graph


def native(ctx, X, perms, n_perm=None, row0=0):
    n, G = X.shape
    ctx.set_expression(X, np.arange(G))
    ctx.set_permutations(perms)
    return ctx.local_moran(n, len(perms) - row0 if n_perm is None else n_perm, row0)


def restated(X, graph, perms):
    ip, ix, w = graph
    w32 = w.astype(np.float32)
    assert (w32.astype(np.float64) == w).all()
    z, lag, I, zero = lr.local_moran_arrays(X, X.dtype.type, ip, ix, w32)
    return {"z": z, "lag": lag, "I": I, "zero_var": zero, "count": lr.local_moran_counts(ip, ix, w32, z, I, perms)}


def assert_same(got, want, note=""):
    np.testing.assert_array_equal(got["zero_var"], want["zero_var"], err_msg=f"zero_var {note}")
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{f} {note}")


def both_forms(monkeypatch):
    """Yields "code" then "float": under the second, count data takes the float-row kernels too."""
    yield "code"
    monkeypatch.setenv("SC_LM_FLOAT_ROWS", "1")
    yield "float"
    monkeypatch.delenv("SC_LM_FLOAT_ROWS")


# ---- native local_moran against the restatement ----------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 15, 16, 17, 100, 127, 128, 129, 150])
def test_gene_edges(ctx, oracle, monkeypatch, G):
    """One tile, a ragged tile, seven tiles, one code-row group, a ragged second one; a zero-variance column and an
    all-zero column in the last tile.  The histogram of the counts too."""
    n, P = 1500, 6
    X = lr.count_matrix(n, G, 100 + G, zero_var=1 if G > 1 else None, all_zero=G - 1 if G > 1 else None)
    graph = knn_graph(ctx, lr.uniform_coords(n, 1))
    perms = table(oracle, n, P)
    want = restated(X, graph, perms)
    if G > 1:
        assert want["zero_var"][1] and want["zero_var"][G - 1] and want["zero_var"].sum() == 2
    for form in both_forms(monkeypatch):
        assert_same(native(ctx, X, perms), want, form)
        hist = ctx.local_moran_hist(P)
        np.testing.assert_array_equal(hist, lr.count_hist(want["count"], P), err_msg=form)
        assert (hist.sum(axis=1) == n).all()


@pytest.mark.parametrize("P", [1, 3, 4, 5, 31, 32, 33, 65])
def test_permutation_edges_code_rows(ctx, oracle, P):
    """Quads of 4 permutations, at most 32 per launch: ragged quads, one full launch, a second and a third launch."""
    n, G = 1500, 17
    X = lr.count_matrix(n, G, 7)
    graph = knn_graph(ctx, lr.uniform_coords(n, 1))
    perms = table(oracle, n, 65)[:P]
    assert_same(native(ctx, X, perms), restated(X, graph, perms))


@pytest.mark.parametrize("data", ["lognorm", "counts"])
@pytest.mark.parametrize("P", [1, 7, 8, 9, 17])
def test_permutation_edges_float_rows(ctx, oracle, monkeypatch, P, data):
    """Batches of 8 permutations; on the count matrix the exact ties reach k_local_count_sorted too."""
    n, G = 1500, 17
    if data == "counts":
        monkeypatch.setenv("SC_LM_FLOAT_ROWS", "1")
        X = lr.count_matrix(n, G, 7)
    else:
        X = lr.lognorm_matrix(n, G, 8)
    graph = knn_graph(ctx, lr.uniform_coords(n, 1))
    perms = table(oracle, n, 65)[:P]
    assert_same(native(ctx, X, perms), restated(X, graph, perms))


@pytest.mark.parametrize("n", [33, 63, 64, 65, 511, 512, 513])
def test_cell_edges(ctx, oracle, monkeypatch, n):
    """32 cells per workgroup of the code-row kernels, 64 of the float-row kernels, 512 per block of the compaction."""
    G, P = 17, 9
    X = lr.count_matrix(n, G, n, zero_var=2)
    graph = knn_graph(ctx, lr.uniform_coords(n, n))
    perms = table(oracle, n, P)
    want = restated(X, graph, perms)
    for form in both_forms(monkeypatch):
        assert_same(native(ctx, X, perms), want, form)
    Xf = lr.lognorm_matrix(n, G, n + 1)
    assert_same(native(ctx, Xf, perms), restated(Xf, graph, perms), "lognorm")


GRAPHS = {"unequal": dict(), "equal-weights-unequal-degrees": dict(equal_weights=True),
          "empty-rows-equal-weights": dict(equal_weights=True, empty_every=9), "empty-rows-unequal": dict(empty_every=9)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", sorted(GRAPHS))
def test_weights_and_rows(ctx, oracle, kind, dtype):
    """Graphs through set_graph_csr: unequal weights (k_local_count_u8<MORAN, false>), one weight with unequal degrees, rows
    without edges; count data and a matrix with negative non-integer values."""
    n, G, P = 700, 17, 9
    coords = lr.uniform_coords(n, 3)
    idx = ctx.knn(coords, K)
    graph = csr_graph(ctx, lr.thinned_csr(idx, seed=6, **GRAPHS[kind]), n)
    deg = np.diff(graph[0])
    assert deg.min() < deg.max()
    perms = table(oracle, n, P)
    rng = np.random.default_rng(9)
    for name, X in (("counts", lr.count_matrix(n, G, 12, dtype=dtype)),
                    ("negative", (rng.normal(0.0, 2.0, (n, G)) * (rng.uniform(size=(n, G)) < 0.6)).astype(dtype))):
        want = restated(X, graph, perms)
        got = native(ctx, X, perms)
        assert_same(got, want, name)
        if "empty" in kind:
            empty = deg == 0
            assert empty.any()
            assert (got["lag"][empty] == 0).all() and (got["I"][empty] == 0).all() and (got["count"][empty] == P).all()
    assert (X < 0).any() and (X != np.round(X)).any()


def test_value_edge(ctx, oracle):
    """A maximum of exactly 31 still travels as code rows; one entry of 32, or one of 0.5, sends the call to the float
    rows.  Each against the restatement."""
    n, G, P = 700, 17, 9
    X = lr.count_matrix(n, G, 13)
    X[5, 2] = 31
    assert X.max() == 31
    graph = knn_graph(ctx, lr.uniform_coords(n, 3))
    perms = table(oracle, n, P)
    assert_same(native(ctx, X, perms), restated(X, graph, perms), "max 31")
    for v in (32.0, 0.5):
        Xv = X.copy()
        Xv[11, 3] = v
        assert_same(native(ctx, Xv, perms), restated(Xv, graph, perms), f"one entry {v}")


@pytest.mark.parametrize("data", ["counts", "lognorm"])
def test_hand_made_rows(ctx, oracle, monkeypatch, data):
    """The identity, a reversal and one random row five times among rows of numpy's stream.  Under the identity
    I_perm is I itself: every identity row adds exactly 1 to every count, whatever the data."""
    n, G = 700, 17
    X = lr.count_matrix(n, G, 14) if data == "counts" else lr.lognorm_matrix(n, G, 15)
    graph = knn_graph(ctx, lr.uniform_coords(n, 3))
    one = np.random.default_rng(2).permutation(n).astype(np.int32)
    ident = np.arange(n, dtype=np.int32)
    base = np.concatenate([table(oracle, n, 3), ident[None, ::-1], np.tile(one, (5, 1))])
    with_ident = np.concatenate([ident[None], base[:4], ident[None], base[4:]])
    want, want2 = restated(X, graph, base), restated(X, graph, with_ident)
    for form in (both_forms(monkeypatch) if data == "counts" else ["float"]):
        got, got2 = native(ctx, X, base), native(ctx, X, with_ident)
        assert_same(got, want, form)
        assert_same(got2, want2, form)
        np.testing.assert_array_equal(got2["count"], got["count"] + 2)


def test_processing_order(ctx, oracle, monkeypatch):
    """A CSR graph takes the neighbour search's bin order when the last search had as many points as the graph has
    rows, the identity otherwise: the outputs must not depend on which."""
    n, G, P = 1500, 17, 9
    coords = lr.uniform_coords(n, 1)
    graph = lr.thinned_csr(ctx.knn(coords, K), seed=6)
    perms = table(oracle, n, P)
    for data, X in (("counts", lr.count_matrix(n, G, 7)), ("lognorm", lr.lognorm_matrix(n, G, 8))):
        want = restated(X, graph, perms)
        for form in (both_forms(monkeypatch) if data == "counts" else ["float"]):
            ctx.knn(coords, K, fetch=False)
            csr_graph(ctx, graph, n)
            in_bin_order = native(ctx, X, perms)
            ctx.knn(lr.uniform_coords(n + 1, 5), K, fetch=False)
            csr_graph(ctx, graph, n)
            in_identity_order = native(ctx, X, perms)
            assert_same(in_bin_order, want, f"{data} {form} bin order")
            assert_same(in_identity_order, want, f"{data} {form} identity order")


def test_perm_row0(ctx, oracle, monkeypatch):
    """Rows [5, 5 + P) of a longer table give the counts of those rows."""
    n, G, P = 700, 17, 13
    X = lr.count_matrix(n, G, 14)
    graph = knn_graph(ctx, lr.uniform_coords(n, 3))
    perms = table(oracle, n, 5 + P + 3)
    want = restated(X, graph, perms[5:5 + P])
    for form in both_forms(monkeypatch):
        assert_same(native(ctx, X, perms, P, 5), want, form)


def test_counts_above_16_bits(ctx, oracle, monkeypatch):
    """A local Moran count is one whole 32-bit word: 20 rows of numpy's stream tiled 3277 times are P = 65540
    permutations -- 2048 full code-row launches and one of 4, 8192 full float-row batches and one of 4.  Counts are
    additive over rows, so the expected counts are the restatement's of the 20 rows times 3277.  On a row without edges
    lag = I = 0 and every permutation satisfies |0| >= |0|: those counts are P itself, above 65535.  The histogram and the
    p of the classification read the same words."""
    n, G, rows, reps = 40, 2, 20, 3277
    P = rows * reps
    assert P == 65540
    X = lr.count_matrix(n, G, 23)
    idx = ctx.knn(lr.uniform_coords(n, 5), K)
    graph = csr_graph(ctx, lr.thinned_csr(idx, seed=6, empty_every=17), n)
    empty = np.diff(graph[0]) == 0
    assert empty[8] and empty[25]
    base = table(oracle, n, rows)
    want = restated(X, graph, base)
    want["count"] = want["count"] * reps
    assert want["count"].dtype == np.int32 and not want["zero_var"].any()
    assert (want["count"][empty] == P).all() and P > 65535
    assert ((want["count"] > 0) & (want["count"] < P)).any()
    perms = np.tile(base, (reps, 1))
    levels = np.tile(lr.pvalue32(np.arange(P + 1), P), (G, 1))
    for form in both_forms(monkeypatch):
        assert_same(native(ctx, X, perms), want, form)
        np.testing.assert_array_equal(ctx.local_moran_hist(P), lr.count_hist(want["count"], P), err_msg=form)
        p, _, _ = ctx.local_moran_classify(n, levels, levels, np.zeros(G, dtype=bool), 0.05)
        np.testing.assert_array_equal(p, levels[np.arange(G)[None, :], want["count"]], err_msg=form)


# ---- local_moran_hist and local_moran_classify -----------------------------------------------------------------------

@pytest.mark.parametrize("G", [5, 17, 33])
@pytest.mark.parametrize("P", [767, 768])
def test_hist_lds_switch(ctx, oracle, P, G):
    """16 (P + 1) counters fit the workgroup's LDS up to P = 767; from 768 on the histogram goes to global atomics."""
    n = 300
    X = lr.count_matrix(n, G, 16)
    graph = knn_graph(ctx, lr.uniform_coords(n, 4))
    perms = table(oracle, n, 768)[:P]
    want = restated(X, graph, perms)
    assert_same(native(ctx, X, perms), want)
    hist = ctx.local_moran_hist(P)
    assert hist.shape == (G, P + 1) and (hist.sum(axis=1) == n).all()
    np.testing.assert_array_equal(hist, lr.count_hist(want["count"], P))


def test_classify(ctx, oracle):
    """p and adjusted p looked up by count in tables the test owns (entries exactly equal to alpha among them), random
    flags, exact zeros of z (a gene whose mean is one of its values: at 512 cells every partial sum of the mean is
    exact) and of lag (rows without edges).  Then without permutations."""
    n, G, P, alpha = 512, 33, 9, 0.3
    rng = np.random.default_rng(17)
    X = lr.count_matrix(n, G, 18)
    X[:, 20] = np.repeat([1, 2, 3, 2], n // 4)[rng.permutation(n)]          # mean exactly 2
    idx = ctx.knn(lr.uniform_coords(n, 6), K)
    graph = csr_graph(ctx, lr.thinned_csr(idx, seed=6, empty_every=9), n)
    perms = table(oracle, n, P)
    want = restated(X, graph, perms)
    assert (want["z"][:, 20] == 0).any() and (want["lag"] == 0).any() and not want["zero_var"].any()
    assert_same(native(ctx, X, perms), want)
    p_tab = rng.uniform(0, 1, (G, P + 1)).astype(np.float32)
    padj_tab = rng.uniform(0, 0.6, (G, P + 1)).astype(np.float32)
    padj_tab[rng.uniform(size=padj_tab.shape) < 0.2] = np.float32(alpha)
    force_ns = rng.uniform(size=G) < 0.2
    assert force_ns.any() and not force_ns.all()
    p, padj, q = ctx.local_moran_classify(n, p_tab, padj_tab, force_ns, alpha)
    gene = np.arange(G)[None, :]
    np.testing.assert_array_equal(p, p_tab[gene, want["count"]])
    np.testing.assert_array_equal(padj, padj_tab[gene, want["count"]])
    want_q = lr.classify(want["z"], want["lag"], padj_tab[gene, want["count"]], alpha, force_ns)
    np.testing.assert_array_equal(q, want_q)
    assert (padj == np.float32(alpha)).any() and len(np.unique(want_q)) == 5
    ctx.set_expression(X, np.arange(G))
    got0 = ctx.local_moran(n, 0)
    for f in ("z", "lag", "I"):
        np.testing.assert_array_equal(got0[f], want[f])
    p0, padj0, q0 = ctx.local_moran_classify(n, None, None, force_ns, alpha)
    assert p0 is None and padj0 is None
    np.testing.assert_array_equal(q0, lr.classify(want["z"], want["lag"], None, alpha, force_ns))


# ---- local Lee -------------------------------------------------------------------------------------------------------

def lee_graph_on_device(ctx, kind, coords, n):
    idx = ctx.knn(coords, lr.LEE_K)
    graph = lr.lee_graph(kind, idx)
    if kind == "knn":
        ctx.graph_from_knn(lr.knn_weight(lr.LEE_K))
    else:
        csr_graph(ctx, graph, n)
        assert (np.diff(graph[0]) == 0).any()
    return graph


@pytest.mark.parametrize("kind", lr.LEE_GRAPHS)
@pytest.mark.parametrize("n", lr.LEE_SIZES)
def test_lee_local(ctx, oracle, n, kind):
    """256 cells per workgroup; batches of 16 permutations: less than one, one, the accumulating second batch, ragged
    last batches; rows from 0 and from 7.  The counts are the restatement's on the device's own z-scores and L."""
    sx, sy = lr.LEE_PAIR
    coords, X = lr.lee_input(n)
    ip, ix, w = lee_graph_on_device(ctx, kind, coords, n)
    ctx.set_expression(X, np.arange(X.shape[1]))
    perms = table(oracle, n, lr.LEE_TABLE_ROWS, lr.LEE_TABLE_SEED)
    ctx.set_permutations(perms)
    zy = ctx.lee_local(n, sy, sx)["zx"]
    deg = np.diff(ip)
    for P in lr.LEE_PERMS:
        for row0 in lr.LEE_ROW0:
            out = ctx.lee_local(n, sx, sy, P, row0)
            zx, lag, L = out["zx"], out["lag"], out["L_local"]
            np.testing.assert_allclose(zx, lr.zscores64(X[:, sx]), rtol=1e-9, atol=0)
            np.testing.assert_allclose(zy, lr.zscores64(X[:, sy]), rtol=1e-9, atol=0)
            np.testing.assert_array_equal(L, zx * lag)
            # a sum of deg terms in any order: within deg u sum |w_e zy_e| of the row-sequential one
            bound = deg * 2.0 ** -53 * lr.row_sequential(ip, ix, w, np.abs(zy))
            assert (np.abs(lag - lr.row_sequential(ip, ix, w, zy)) <= bound).all()
            want = lr.lee_local_counts(ip, ix, w, zx, zy, L, perms[row0:row0 + P])
            np.testing.assert_array_equal(out["count"], want, err_msg=f"P={P} row0={row0}")
            assert (out["count"][deg == 0] == P).all()


@pytest.mark.parametrize("kind", lr.LEE_GRAPHS)
@pytest.mark.parametrize("Pg,Pl", lr.LEE_SEEDED)
def test_lee_local_seeded(ctx, oracle, Pg, Pl, kind):
    """One generator state for the rows of the global statistic and the rows of the per-cell counts: the counts are the
    restatement's on rows [Pg, Pg + Pl) of numpy's stream and numpy's z-scores (no near tie on this input:
    tests/test_cpu_local_restated.py)."""
    from spatialcore_amd._lib import rng_state_words

    sx, sy = lr.LEE_PAIR
    n = lr.LEE_SIZES[-1]
    coords, X = lr.lee_input(n)
    ip, ix, w = lee_graph_on_device(ctx, kind, coords, n)
    ctx.set_expression(X, np.arange(X.shape[1]))
    words = rng_state_words(np.random.default_rng(lr.LEE_SEEDED_SEED))
    got = ctx.lee_local_seeded(words, n, sx, sy, Pg, Pl)
    rows, end_words = oracle.perm_table(lr.LEE_SEEDED_SEED, n, Pg + Pl)
    np.testing.assert_array_equal(words, end_words)
    zx, zy = lr.zscores64(X[:, sx]), lr.zscores64(X[:, sy])
    L = zx * lr.row_sequential(ip, ix, w, zy)
    np.testing.assert_allclose(got["L_local"], L, rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(got["count"], lr.lee_local_counts(ip, ix, w, zx, zy, L, rows[Pg:]))
    if Pg > 0:
        u = np.array([(zx * lr.row_sequential(ip, ix, w, zy[r])).sum() for r in rows[:Pg]])
        assert got["L"] == pytest.approx(L.sum(), rel=1e-9)
        assert got["count_abs_ge"] == int((np.abs(u) >= abs(L.sum())).sum())


# ---- the public functions --------------------------------------------------------------------------------------------

API_FIELDS = ("z", "lag", "I", "p", "p_adj", "quadrant")


def test_local_morans_i_default_batches(oracle):
    """130 genes at the default batch_size of 100: batches of 100 and 30, seven tiles with a ragged last one in the
    first, dense and CSR input; then a gene list that is unsorted and repeats a gene across the batch edge."""
    from spatialcore_amd.spatial import local_morans_i

    n, G, P = 1500, 130, 33
    coords, X = synth(n, 140, 31, dtype=np.float32)
    want = oracle.local_morans_i(coords, X, np.arange(G), K, P, 3, fdr="fdr_bh", alpha=0.4)
    names = [f"g{i}" for i in range(G)]
    for Xin in (X.toarray(), X):
        ad = make_adata(coords, Xin)
        local_morans_i(ad, genes=names, n_neighbors=K, n_permutations=P, seed=3, alpha=0.4)
        for f in API_FIELDS:
            np.testing.assert_array_equal(ad.obsm[f"local_morans_{f}"], want[f], err_msg=f"{f} sparse={sparse.issparse(Xin)}")
    cols = np.random.default_rng(4).permutation(140)[:G]
    cols[100] = cols[99]                           # the same gene on both sides of the batch edge
    assert len(set(cols.tolist())) == G - 1 and (np.diff(cols) < 0).any()
    want = oracle.local_morans_i(coords, X, cols, K, P, 5, fdr="fdr_bh", alpha=0.4)
    ad = make_adata(coords, X)
    local_morans_i(ad, genes=[f"g{i}" for i in cols], n_neighbors=K, n_permutations=P, seed=5, alpha=0.4)
    for f in API_FIELDS:
        np.testing.assert_array_equal(ad.obsm[f"local_morans_{f}"], want[f], err_msg=f"gene list {f}")


def test_lees_l_local_against_the_restated_flow(oracle):
    """compute_cell_pvalues with 40 permutations: numpy's z-scores, one generator across the pairs (40 rows for the
    global statistic, then 40 for the cells, per pair); p-values and quadrants equal (no near tie on this input)."""
    from spatialcore_amd.spatial import lees_l_local

    api = lr.LEE_API
    n, P, k, alpha = api["n"], api["P"], api["k"], api["alpha"]
    coords, X = lr.lee_input(n)
    ad = make_adata(coords, X)
    pairs = [(f"g{a}", f"g{b}") for a, b in api["pairs"]]
    lees_l_local(ad, gene_pairs=pairs, n_neighbors=k, n_permutations=P, compute_cell_pvalues=True,
                 significance_filter=True, alpha=alpha, seed=api["seed"])
    ip, ix, w = lr.knn_csr(oracle.knn_bruteforce(coords, k), lr.knn_weight(k))
    rows = table(oracle, n, 2 * P * len(pairs), api["seed"])
    labels = np.array(["NS", "HH", "LL", "HL", "LH"])
    for gi, (a, b) in enumerate(api["pairs"]):
        key = f"g{a}_g{b}"
        zx, zy = lr.zscores64(X[:, a]), lr.zscores64(X[:, b])
        lag = lr.row_sequential(ip, ix, w, zy)
        L = zx * lag
        p = lr.pvalue32(lr.lee_local_counts(ip, ix, w, zx, zy, L, rows[2 * P * gi + P:2 * P * (gi + 1)]), P)
        np.testing.assert_array_equal(ad.obs[f"{key}_pvalue"].values, p, err_msg=key)
        quad = lr.classify(zx, lag, p, alpha, False)
        np.testing.assert_array_equal(ad.obs[f"{key}_quadrant"].astype(str).values, labels[quad], err_msg=key)
        np.testing.assert_allclose(ad.obs[f"{key}_lees_l"].values, L.astype(np.float32), rtol=1e-6, atol=1e-7)
        u = np.array([(zx * lr.row_sequential(ip, ix, w, zy[r])).sum() for r in rows[2 * P * gi:2 * P * gi + P]])
        prm = ad.uns[f"{key}_lees_l_params"]
        assert prm["global_pvalue"] == float(((np.abs(u) >= abs(L.sum())).sum() + 1) / (P + 1))
