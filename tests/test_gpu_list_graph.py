"""The resident weighted graph (sc_list_graph.h) across its users: what a new search, a graph from the lists, an uploaded
graph and the ends of a Lanczos run leave valid, walked through Context methods on 64 points; and the symmetric union at
its lower bound n = k + 1, where every list entry is mutual.  The arithmetic of the graphs is pinned elsewhere
(test_gpu_diffusion.py, test_gpu_umap.py, test_gpu_louvain.py); here it is which call may follow which."""
import numpy as np
import pytest

import diffusion_restated as R

pytestmark = pytest.mark.gpu

N, D, K = 64, 8, 5
LAYOUT = dict(a=1.5, b=0.9, gamma=1.0, alpha0=1.0, neg=5, n_epochs=4, seed=3)


@pytest.fixture(scope="module")
def points():
    return np.random.default_rng(64).standard_normal((N, D))


@pytest.fixture
def ctx():
    from spatialcore_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def _y0():
    return np.random.default_rng(2).standard_normal((N, 2))


def _start():
    return np.random.default_rng(1).standard_normal(N)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_new_search_drops_the_graph_and_the_run(ctx, points):
    ctx.knn_dense(points, K)
    ctx.diffmap_graph()
    ctx.lanczos_begin(_start(), 8)
    ctx.knn_dense(points, K)
    with pytest.raises(RuntimeError, match="no Lanczos run"):
        ctx.lanczos_run(2)
    with pytest.raises(RuntimeError, match="no graph is resident"):
        ctx.diffmap_graph_get()
    with pytest.raises(RuntimeError, match="no graph is resident"):
        ctx.umap_layout(None, _y0(), **LAYOUT)
    with pytest.raises(RuntimeError, match="no graph is resident"):
        ctx.louvain_begin_resident(None, 1 << 16, 10)
    with pytest.raises(RuntimeError, match="no transition matrix"):
        ctx.lanczos_begin(_start(), 8)


def test_a_graph_from_the_lists_drops_the_run_and_replaces_the_graph(ctx, points):
    from spatialcore_amd import _lib

    ctx.knn_dense(points, K)
    ctx.diffmap_graph()
    kernel = ctx.diffmap_graph_get()
    ctx.lanczos_begin(_start(), 8)
    info = ctx.fuzzy_graph()
    with pytest.raises(RuntimeError, match="no Lanczos run"):
        ctx.lanczos_run(2)
    Y = ctx.umap_layout(None, _y0(), **LAYOUT)
    assert Y.shape == (N, 2) and np.all(np.isfinite(Y)) and not np.array_equal(Y, _y0())
    fuzzy = ctx.diffmap_graph_get(transition=True)
    # the fuzzy graph: the same union, memberships in place of the kernel weights -- bit for bit what a context that never
    # held another graph computes
    assert fuzzy[1].size == info["n_edges"]
    assert np.array_equal(fuzzy[0], kernel[0]) and np.array_equal(fuzzy[1], kernel[1])
    assert np.all(fuzzy[2] > 0.0) and not np.array_equal(fuzzy[2], kernel[2])
    fresh = _lib.Context(0)
    fresh.knn_dense(points, K)
    fresh.fuzzy_graph()
    assert _same(fuzzy, fresh.diffmap_graph_get(transition=True))
    fresh.close()


def test_an_uploaded_graph_drops_the_lists(ctx, points):
    ctx.knn_dense(points, K)
    ctx.diffmap_graph()
    g = ctx.diffmap_graph_get()
    other = np.random.default_rng(5).standard_normal((N, D))
    ctx.knn_dense(other, K)            # lists of other points are resident when g arrives
    assert ctx.diffmap_graph_csr(*g) == R.n_components(g[0], g[1])
    with pytest.raises(RuntimeError, match="no neighbour lists are resident"):
        ctx.fuzzy_graph()
    with pytest.raises(RuntimeError, match="no neighbour lists are resident"):
        ctx.diffmap_graph()
    ctx.lanczos_begin(_start(), 8)
    alpha, beta = ctx.lanczos_run(2)
    assert alpha.size == 2 and beta.size == 3
    assert np.array_equal(ctx.louvain_resident_weights(), g[2])
    assert _same(ctx.diffmap_graph_get(), g)


def test_the_end_of_a_run_keeps_the_graph(ctx, points):
    ctx.knn_dense(points, K)
    ctx.diffmap_graph()
    g = ctx.diffmap_graph_get(transition=True)
    ctx.lanczos_begin(_start(), 8)
    ctx.lanczos_run(2)
    ctx.lanczos_end()
    with pytest.raises(RuntimeError, match="no Lanczos run"):
        ctx.lanczos_run(2)
    assert _same(ctx.diffmap_graph_get(transition=True), g)
    ctx.lanczos_begin(_start(), 8)     # and a new run may begin on it
    assert ctx.lanczos_run(1)[0].size == 1


def test_a_refused_upload_touches_nothing(ctx, points):
    ctx.knn_dense(points, K)
    ctx.diffmap_graph()
    g = ctx.diffmap_graph_get(transition=True)
    ctx.lanczos_begin(_start(), 8)
    ctx.lanczos_run(2)
    bad = g[2].copy()
    bad[7] = 0.0
    with pytest.raises(ValueError, match="stored value 7 must be finite and > 0"):
        ctx.diffmap_graph_csr(g[0], g[1], bad)
    assert _same(ctx.diffmap_graph_get(transition=True), g)
    assert ctx.lanczos_run(1)[0].size == 3                 # the open run goes on
    assert np.array_equal(ctx.louvain_resident_weights(), g[2])
    assert ctx.fuzzy_graph()["n_edges"] == g[1].size       # and the lists are still there


@pytest.mark.parametrize("n,d,k", [(6, 3, 5), (3, 2, 2)])
def test_union_where_every_entry_is_mutual(ctx, n, d, k):
    """n = k + 1: every cell lists every other, every sorted key run has length exactly 2, and the union stores
    nnz = n k entries -- the lower edge of the range check and of the first-of-run flags with the compaction."""
    X = np.random.default_rng(n).standard_normal((n, d))
    ctx.knn_dense(X, k)
    info = ctx.diffmap_graph()
    indptr, indices, w = ctx.diffmap_graph_get()
    g = R.graph(X, k)
    assert g["indices"].size == n * k and np.all(np.diff(g["indptr"]) == k)
    assert np.array_equal(indptr, g["indptr"]) and np.array_equal(indices, g["indices"])
    assert info["n_edges"] == n * k and info["n_components"] == 1
