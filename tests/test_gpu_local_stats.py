"""GPU: Getis-Ord Gi / Gi* and local Geary's C against their plain restatement (tests/local_stats_restated.py, pinned to
the textbook formulas by tests/test_cpu_local_stats.py).

Every comparison is ``==``: z, lag, the statistic, both tails of the counts and the zero-variance flags.  The
permutation tables are the tests' own (rows of numpy's stream plus hand-made rows, uploaded with ``set_permutations``).
The edges are those of tests/test_gpu_local.py, whose structure this file follows: 16-gene tiles and 128-gene code-row
groups; quads of 4 (Geary: pairs) and launches of 32 permutations of the code-row kernels, batches of 8 of the float-row
kernels; 32 / 64 cells per workgroup; unequal weights, unequal degrees, empty rows, negative values; the self edge of Gi*;
both tails at 65535, the packed word full.
"""
import numpy as np
import pytest

import local_restated as lr
import local_stats_restated as ls
from conftest import make_adata, synth

pytestmark = pytest.mark.gpu

K = 6
FIELDS = ("z", "lag", "stat", "ge", "le")
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


def knn_graph(ctx, stat, coords, k=K):
    """The statistic's row-normalised kNN graph on the device (Gi*: k + 1 neighbours, self included); returns its CSR
    arrays, built here from the neighbour lists."""
    kk = k + 1 if stat == "getis_star" else k
    idx = ctx.knn(coords, kk, include_self=stat == "getis_star")
    ctx.graph_from_knn(lr.knn_weight(kk))
    return lr.knn_csr(idx, lr.knn_weight(kk))


def thinned_graph(ctx, stat, coords, n, **kw):
    idx = ctx.knn(coords, K)
    graph = lr.thinned_csr(ls.star_lists(idx) if stat == "getis_star" else idx, **kw)
    ctx.set_graph_csr(*graph, n)
    return graph


def native(ctx, stat, X, perms, n_perm=None, row0=0):
    n, G = X.shape
    ctx.set_expression(X, np.arange(G))
    ctx.set_permutations(perms)
    return ctx.local_stat("geary" if stat == "geary" else "getis", n, len(perms) - row0 if n_perm is None else n_perm, row0,
                          star=stat == "getis_star")


def assert_same(got, want, note=""):
    np.testing.assert_array_equal(got["zero_var"], want["zero_var"], err_msg=f"zero_var {note}")
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype, f
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{f} {note}")


def both_forms(monkeypatch):
    """Yields "code" then "float": under the second, count data takes the float-row kernels too."""
    yield "code"
    monkeypatch.setenv("SC_LM_FLOAT_ROWS", "1")
    yield "float"
    monkeypatch.delenv("SC_LM_FLOAT_ROWS")


def level_hist(want, P):
    return lr.count_hist(np.minimum(want["ge"], want["le"]), P)


# ---- native local_stat against the restatement -----------------------------------------------------------------------

@pytest.mark.parametrize("stat", ls.STATS)
@pytest.mark.parametrize("G", [1, 16, 17, 128, 129])
def test_gene_edges(ctx, oracle, monkeypatch, G, stat):
    """One tile, a ragged second tile, one code-row group, a ragged second one; a zero-variance column and an all-zero
    column in the last tile.  Both forms, and the histogram of m = min(ge, le).  The self edge of Gi* sits inside its row."""
    n, P = 1500, 6
    X = lr.count_matrix(n, G, 100 + G, zero_var=1 if G > 1 else None, all_zero=G - 1 if G > 1 else None)
    graph = knn_graph(ctx, stat, lr.uniform_coords(n, 1))
    if stat == "getis_star":
        rows = graph[1].reshape(n, K + 1)
        assert ((rows == np.arange(n)[:, None]).sum(axis=1) == 1).all()
        assert ((rows[:, 0] < np.arange(n)) & (rows[:, -1] > np.arange(n))).any()   # a smaller and a larger neighbour
    perms = table(oracle, n, P)
    want = ls.restated(stat, X, graph, perms)
    if G > 1:
        assert want["zero_var"][1] and want["zero_var"][G - 1] and want["zero_var"].sum() == 2
    for form in both_forms(monkeypatch):
        assert_same(native(ctx, stat, X, perms), want, form)
        hist = ctx.local_stat_hist(P)
        np.testing.assert_array_equal(hist, level_hist(want, P), err_msg=form)
        assert (hist.sum(axis=1) == n).all()


@pytest.mark.parametrize("stat", ls.STATS)
@pytest.mark.parametrize("P", [1, 3, 4, 5, 32, 33])
def test_permutation_edges_code_rows(ctx, oracle, P, stat):
    """Quads of 4 permutations (Geary: pairs), at most 32 per launch: ragged quads, one full launch, a second launch."""
    n, G = 1500, 17
    X = lr.count_matrix(n, G, 7)
    graph = knn_graph(ctx, stat, lr.uniform_coords(n, 1))
    perms = table(oracle, n, 33)[:P]
    assert_same(native(ctx, stat, X, perms), ls.restated(stat, X, graph, perms))


@pytest.mark.parametrize("stat", ls.STATS)
@pytest.mark.parametrize("data", ["lognorm", "counts"])
@pytest.mark.parametrize("P", [1, 7, 8, 9, 17])
def test_permutation_edges_float_rows(ctx, oracle, monkeypatch, P, data, stat):
    """Batches of 8 permutations; on the count matrix the exact ties reach the float-row kernels too."""
    n, G = 1500, 17
    if data == "counts":
        monkeypatch.setenv("SC_LM_FLOAT_ROWS", "1")
        X = lr.count_matrix(n, G, 7)
    else:
        X = lr.lognorm_matrix(n, G, 8)
    graph = knn_graph(ctx, stat, lr.uniform_coords(n, 1))
    perms = table(oracle, n, 33)[:P]
    assert_same(native(ctx, stat, X, perms), ls.restated(stat, X, graph, perms))


@pytest.mark.parametrize("stat", ls.STATS)
@pytest.mark.parametrize("n", [33, 63, 64, 65, 513])
def test_cell_edges(ctx, oracle, monkeypatch, n, stat):
    """32 cells per workgroup of the code-row kernels, 64 of the float-row kernels, 512 per block of the compaction."""
    G, P = 17, 9
    X = lr.count_matrix(n, G, n, zero_var=2)
    graph = knn_graph(ctx, stat, lr.uniform_coords(n, n))
    perms = table(oracle, n, P)
    want = ls.restated(stat, X, graph, perms)
    for form in both_forms(monkeypatch):
        assert_same(native(ctx, stat, X, perms), want, form)
    Xf = lr.lognorm_matrix(n, G, n + 1)
    assert_same(native(ctx, stat, Xf, perms), ls.restated(stat, Xf, graph, perms), "lognorm")


GRAPHS = {"unequal": dict(), "equal-weights-unequal-degrees": dict(equal_weights=True),
          "empty-rows-equal-weights": dict(equal_weights=True, empty_every=9), "empty-rows-unequal": dict(empty_every=9)}


@pytest.mark.parametrize("stat", ls.STATS)
@pytest.mark.parametrize("kind", sorted(GRAPHS))
def test_weights_and_rows(ctx, oracle, kind, stat):
    """Graphs through set_graph_csr: unequal weights, one weight with unequal degrees, rows without edges; count data
    and a matrix with negative non-integer values.  On an empty row the sum, C and G are 0 and every permutation ties."""
    n, G, P = 700, 17, 9
    graph = thinned_graph(ctx, stat, lr.uniform_coords(n, 3), n, seed=6, **GRAPHS[kind])
    deg = np.diff(graph[0])
    assert deg.min() < deg.max()
    perms = table(oracle, n, P)
    rng = np.random.default_rng(9)
    for name, X in (("counts", lr.count_matrix(n, G, 12)),
                    ("negative", (rng.normal(0.0, 2.0, (n, G)) * (rng.uniform(size=(n, G)) < 0.6)).astype(np.float32))):
        want = ls.restated(stat, X, graph, perms)
        got = native(ctx, stat, X, perms)
        assert_same(got, want, name)
        if "empty" in kind:
            empty = deg == 0
            assert empty.any()
            assert (got["lag"][empty] == 0).all() and (got["stat"][empty] == 0).all()
            assert (got["ge"][empty] == P).all() and (got["le"][empty] == P).all()
    assert (X < 0).any() and (X != np.round(X)).any()


@pytest.mark.parametrize("stat", ls.STATS)
@pytest.mark.parametrize("data", ["counts", "lognorm"])
def test_hand_made_rows(ctx, oracle, monkeypatch, data, stat):
    """The identity, a reversal and one random row five times among rows of numpy's stream.  Under the identity the
    permuted value is the observed one: every identity row adds exactly 1 to ge and to le, whatever the data."""
    n, G = 700, 17
    X = lr.count_matrix(n, G, 14) if data == "counts" else lr.lognorm_matrix(n, G, 15)
    graph = knn_graph(ctx, stat, lr.uniform_coords(n, 3))
    one = np.random.default_rng(2).permutation(n).astype(np.int32)
    ident = np.arange(n, dtype=np.int32)
    base = np.concatenate([table(oracle, n, 3), ident[None, ::-1], np.tile(one, (5, 1))])
    with_ident = np.concatenate([ident[None], base[:4], ident[None], base[4:]])
    want, want2 = ls.restated(stat, X, graph, base), ls.restated(stat, X, graph, with_ident)
    for form in (both_forms(monkeypatch) if data == "counts" else ["float"]):
        got, got2 = native(ctx, stat, X, base), native(ctx, stat, X, with_ident)
        assert_same(got, want, form)
        assert_same(got2, want2, form)
        np.testing.assert_array_equal(got2["ge"], got["ge"] + 2)
        np.testing.assert_array_equal(got2["le"], got["le"] + 2)


@pytest.mark.parametrize("stat", ls.STATS)
@pytest.mark.parametrize("data", ["counts", "lognorm"])
def test_seeded_equals_generate_then_count(ctx, stat, data):
    """local_stat_seeded draws its permutations inside the call, beside the counts: every output and the generator
    words it leaves are those of generate_permutations followed by local_stat."""
    from spatialcore_amd._lib import rng_state_words

    n, G, P = 3000, 21, 40
    X = lr.count_matrix(n, G, 21) if data == "counts" else lr.lognorm_matrix(n, G, 22)
    knn_graph(ctx, stat, lr.uniform_coords(n, 8))
    ctx.set_expression(X, np.arange(G))
    code, star = ("geary" if stat == "geary" else "getis"), stat == "getis_star"
    w1 = rng_state_words(np.random.default_rng(77))
    ctx.generate_permutations(w1, n, P)
    want = ctx.local_stat(code, n, P, star=star)
    w2 = rng_state_words(np.random.default_rng(77))
    got = ctx.local_stat_seeded(code, w2, n, P, star=star)
    np.testing.assert_array_equal(w1, w2)
    assert_same(got, want)
    assert want["ge"].max() <= P and ((want["ge"] + want["le"]) >= P).all()


@pytest.mark.parametrize("stat", ["getis", "geary"])
def test_both_tails_full(ctx, oracle, monkeypatch, stat):
    """The largest P the two tails accept: 15 rows of numpy's stream tiled 4369 times are 65535 permutations.  Counts are
    additive over rows, so the expected tails are the restatement's of the 15 rows times 4369.  On a row without edges the
    statistic and every permuted value are the empty sum 0: ge = le = 65535, all 32 bits of the packed word set.  The
    histogram of m = min(ge, le) and the p of the classification read the folded words."""
    n, G, rows, reps = 40, 2, 15, 4369
    P = rows * reps
    assert P == 65535
    X = lr.count_matrix(n, G, 23)
    graph = thinned_graph(ctx, stat, lr.uniform_coords(n, 5), n, seed=6, empty_every=17)
    empty = np.diff(graph[0]) == 0
    assert empty[8] and empty[25]
    base = table(oracle, n, rows)
    want = ls.restated(stat, X, graph, base)
    want["ge"], want["le"] = want["ge"] * reps, want["le"] * reps
    assert want["ge"].dtype == np.int32 and not want["zero_var"].any()
    assert (want["ge"][empty] == P).all() and (want["le"][empty] == P).all()
    perms = np.tile(base, (reps, 1))
    levels = np.tile(lr.pvalue32(np.arange(P + 1), P), (G, 1))
    m = np.minimum(want["ge"], want["le"])
    for form in both_forms(monkeypatch):
        assert_same(native(ctx, stat, X, perms), want, form)
        np.testing.assert_array_equal(ctx.local_stat_hist(P), level_hist(want, P), err_msg=form)
        p, _, _ = ctx.local_stat_classify(n, levels, levels, np.zeros(G, dtype=bool), 0.05)
        np.testing.assert_array_equal(p, levels[np.arange(G)[None, :], m], err_msg=form)


def test_state_hygiene(ctx, oracle):
    """A local-stat result does not satisfy local Moran's finalisation, nor the reverse."""
    n, G, P = 300, 5, 4
    X = lr.count_matrix(n, G, 16)
    knn_graph(ctx, "getis", lr.uniform_coords(n, 4))
    perms = table(oracle, n, P)
    flags = np.zeros(G, dtype=bool)
    tab = np.zeros((G, P + 1), dtype=np.float32)
    for stat in ls.STATS:
        native(ctx, stat, X, perms)
        with pytest.raises(RuntimeError, match="no sc_local_moran result"):
            ctx.local_moran_hist(P)
        with pytest.raises(RuntimeError, match="no sc_local_moran result"):
            ctx.local_moran_classify(n, tab, tab, flags, 0.05)
        assert ctx.local_stat_hist(P).sum() == n * G
    ctx.local_moran(n, P)
    with pytest.raises(RuntimeError, match="no sc_local_stat result"):
        ctx.local_stat_hist(P)
    with pytest.raises(RuntimeError, match="no sc_local_stat result"):
        ctx.local_stat_classify(n, tab, tab, flags, 0.05)
    assert ctx.local_moran_hist(P).sum() == n * G
    with pytest.raises(ValueError, match="above 65535"):
        ctx.local_stat("getis", n, 65536)


# ---- the public functions --------------------------------------------------------------------------------------------

def bh_sorted(p):
    """Benjamini-Hochberg over one gene's cells by sorting them: float32 p times n, float64 quotient by the rank, the
    running minimum from the largest down, clipped, stored as float32."""
    n = p.size
    order = np.argsort(p, kind="stable")
    adj = (p[order] * np.float32(n)).astype(np.float64) / np.arange(1, n + 1)
    adj = np.minimum.accumulate(adj[::-1])[::-1]
    out = np.empty(n)
    out[order] = adj
    return np.clip(out, 0, 1).astype(np.float32)


API = dict(n=1500, G=24, P=19, k=6, seed=5, alpha=0.3, batch=7)
_API = {}


def api_input():
    """20 requested genes of a 24-gene count matrix (half of the genes smooth in space), out of order, one named three
    times (twice in one batch, once in the next), one constant."""
    if not _API:
        n = API["n"]
        cols = np.random.default_rng(4).permutation(API["G"])[:20]
        cols[5] = cols[12] = cols[3]
        coords, X = synth(n, API["G"], 31, dtype=np.float32, sparse_x=False)
        X[:, cols[9]] = 2
        assert X.max() < 32 and (X == np.round(X)).all()           # the code-row form
        _API.update(coords=coords, X=X, cols=cols)
    return _API["coords"], _API["X"], _API["cols"]


def api_restated(oracle, stat, P):
    """The flow of the public functions on the restatement: batches of 7 genes on one default_rng(seed) stream, p from
    m = min(ge, le), sort-based BH per gene, classes; flagged genes z = lag = statistic = 0, p = p_adj = 1, class 0."""
    coords, X, cols = api_input()
    n, alpha = API["n"], API["alpha"]
    graph = ls.stat_graph(stat, oracle.knn_bruteforce(coords, API["k"]), API["k"])
    rng = np.random.default_rng(API["seed"])
    out = {f: np.zeros((n, cols.size), dtype=np.float32) for f in ("z", "lag", "stat")}
    p = np.ones((n, cols.size), dtype=np.float32)
    zero = np.zeros(cols.size, dtype=bool)
    for b0 in range(0, cols.size, API["batch"]):
        b1 = min(b0 + API["batch"], cols.size)
        perms = np.stack([rng.permutation(n) for _ in range(P)]) if P else np.zeros((0, n), dtype=np.int64)
        r = ls.restated(stat, X[:, cols[b0:b1]], graph, perms)
        for f in out:
            out[f][:, b0:b1] = r[f]
        if P:
            p[:, b0:b1] = lr.pvalue32(np.minimum(r["ge"], r["le"]), P)
        zero[b0:b1] = r["zero_var"]
    C = out["stat"].copy()
    for f in out:
        out[f][:, zero] = 0
    p[:, zero] = 1
    padj = np.stack([bh_sorted(p[:, g]) for g in range(cols.size)], axis=1) if P else p
    padj[:, zero] = 1
    if stat == "geary":
        ip, ix, w = graph
        # (classes of flagged genes are 0 whatever the arrays hold)
        cls = ls.geary_classes(C, ls.geary_expectation(ip, ix, w), out["z"], out["lag"], padj if P else None, alpha, zero)
    else:
        cls = ls.spot_classes(out["stat"], padj if P else None, alpha, zero)
    return dict(out, p=p, p_adj=padj, cls=cls, zero=zero)


@pytest.mark.parametrize("P", [19, 0])
@pytest.mark.parametrize("stat", ls.STATS)
def test_public_functions(oracle, stat, P):
    """Three batches on one stream, a duplicate and a zero-variance gene: every obsm array equals the restated flow."""
    from spatialcore_amd.spatial import local_gearys_c, local_getis_ord

    coords, X, cols = api_input()
    want = api_restated(oracle, stat, P)
    assert want["zero"].sum() == 1 and len(set(cols.tolist())) == cols.size - 2
    ad = make_adata(coords, X)
    kw = dict(genes=[f"g{i}" for i in cols], n_neighbors=API["k"], n_permutations=P, seed=API["seed"], alpha=API["alpha"],
              batch_size=API["batch"])
    if stat == "geary":
        local_gearys_c(ad, **kw)
        key, val, cls = "local_geary", "C", "cluster"
    else:
        local_getis_ord(ad, star=stat == "getis_star", **kw)
        key, val, cls = "local_getis", "G", "spot"
    for f, name in (("z", "z"), ("lag", "lag"), ("stat", val), ("p", "p"), ("p_adj", "p_adj"), ("cls", cls)):
        got = ad.obsm[f"{key}_{name}"]
        assert got.dtype == want[f].dtype and got.shape == want[f].shape, name
        np.testing.assert_array_equal(got, want[f], err_msg=name)
    prm = ad.uns[f"{key}_params"]
    assert prm["zero_variance_genes"] == [f"g{cols[9]}"] and prm["n_permutations"] == P and "class_codes" in prm
    assert ("star" in prm) == (stat != "geary")
    if P:
        assert len(np.unique(want["cls"])) == (3 if stat != "geary" else 5)     # every class occurs
        assert (want["p_adj"] < API["alpha"]).any() and (want["p_adj"] >= API["alpha"]).any()
    assert ad.uns["spatialcore_metadata"]["operations"][-1]["function"] == ("local_gearys_c" if stat == "geary" else "local_getis_ord")


def test_gi_shares_z_and_lag_with_local_morans_i():
    """local_getis_ord(star=False) runs on the graph and the preparation of local_morans_i: _z and _lag bit for bit, in
    three batches with a repeated gene and in one batch of distinct genes in column order (whose arrays become the
    outputs as they are); G does not depend on the batches."""
    from spatialcore_amd.spatial import local_getis_ord, local_morans_i

    coords, X, cols = api_input()
    for genes, batch in ([f"g{i}" for i in cols], 7), ([f"g{i}" for i in sorted(set(cols.tolist()))], 100):
        a, b, c = make_adata(coords, X), make_adata(coords, X), make_adata(coords, X)
        local_getis_ord(a, genes=genes, star=False, n_permutations=5, batch_size=batch)
        local_morans_i(b, genes=genes, n_permutations=5, batch_size=batch)
        local_getis_ord(c, genes=genes, star=False, n_permutations=5, batch_size=3)
        for f in ("z", "lag"):
            np.testing.assert_array_equal(a.obsm[f"local_getis_{f}"], b.obsm[f"local_morans_{f}"], err_msg=f)
        np.testing.assert_array_equal(a.obsm["local_getis_G"], c.obsm["local_getis_G"])
        assert a.obsm["local_getis_p"].shape == (API["n"], len(genes)) and a.obsm["local_getis_spot"].dtype == np.int8
