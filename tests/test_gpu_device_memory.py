"""GPU tests that device memory comes back: every assertion is an exact equality on Context.device_mem(), the library's
own count of the bytes its DBufs hold.

Call-scoped entry points (k-means, the threshold calls, NMF, HVG, annotation's predict / transform) allocate their
buffers inside the call and must leave the counter where it was.  The baseline is read after a first warm-up call, so
that the context's own grow-only buffers (the sort scratch, th_sorted after ks_prepare) are at size.

Resident problems (PCA, annotation training, Harmony; Louvain's case lives in test_gpu_louvain.py) hold memory between
_begin and _end: during > before, a second _begin with the same inputs stays at during, _end returns to before, a second
_end is SC_OK and changes nothing.

Refusals after allocation.  Read entry point by entry point, every SC_ERR_INVALID return of sc_kmeans_fit,
sc_metagene_score, sc_ks_prepare, sc_ks_argmax, sc_ks_classify, sc_gmm_fit, sc_gmm_posterior, sc_nmf_fit, sc_hvg_pearson,
sc_annot_predict, sc_annot_transform, sc_pca_begin, sc_annot_train_begin, sc_harmony_begin and sc_louvain_begin comes
before the call's first allocation: their values are checked on the host, and what can fail afterwards is a HIP error,
which no test provokes.  So none of those has a refusal case here.  The one entry point that refuses after its buffers
exist is sc_louvain_begin_resident, whose symmetry check runs on the device; it has the refusal case."""
import numpy as np
import pytest

import harmony_restated as H
import kmeans_restated as kr
import pca_restated
from test_cpu_niches import blobs
from test_gpu_niches_edges import _random_draws, _zero_draws

pytestmark = pytest.mark.gpu

T = 3   # classes of the annotation cases
K = 3   # components of the NMF cases


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


def _counts():
    """300 cells x 9 genes of counts with an all-zero gene and an all-zero cell (float64 CSR, canonical)."""
    return pca_restated.counts(300, 9, pca_restated.SEED)


def _scores(dtype=np.float64):
    """500 scores in two groups around 0 and 4."""
    rng = np.random.default_rng(3)
    return np.concatenate([rng.normal(0.0, 1.0, 300), rng.normal(4.0, 1.0, 200)]).astype(dtype)


def _returns(ctx, call):
    """Runs call() once to warm the context's own buffers up, then once more between two readings of the counter."""
    call()
    before = ctx.device_mem()
    out = call()
    assert ctx.device_mem() == before
    return out


# ---- 1. call-scoped entry points -------------------------------------------------------------------------------------------------------
def _kmeans(ctx, X, n_clusters, max_iter, draws):
    tol = float(np.mean(np.var(X, axis=0)) * 1e-4)
    return ctx.kmeans(X, n_clusters, draws.shape[0], max_iter, tol, X.mean(axis=0), draws)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kmeans(dtype):
    X = blobs(700, 5, 6, 24, dtype)
    fit = _returns(_ctx(), lambda: _kmeans(_ctx(), X, 6, 300, _random_draws(24, 2, 6)))
    assert fit["distinct"] == 6


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kmeans_with_relocation_scratch(dtype):
    """Run 0 seeds every cluster on point 0, so five clusters start empty and the relocation's distance buffer is used;
    two runs, so the best-run comparison's buffer is used as well."""
    n, n_clusters = 700, 6
    X = blobs(n, 5, n_clusters, 24, dtype)
    draws = _zero_draws(n, n_clusters, [0], 24)
    ref = kr.fit(X, n_clusters, draws.shape[0], 300, draws, kernel_order=True)
    assert ref["relocations"][0][0]["empties"] == [1, 2, 3, 4, 5]
    fit = _returns(_ctx(), lambda: _kmeans(_ctx(), X, n_clusters, 300, draws))
    np.testing.assert_array_equal(fit["seeds"][0], [0] * n_clusters)
    np.testing.assert_array_equal(fit["labels"], ref["labels"])


def test_metagene_score():
    F = np.random.default_rng(5).gamma(2.0, 1.0, (500, 3))
    out = _returns(_ctx(), lambda: _ctx().metagene_score(F, "shifted_geometric_mean"))
    assert out["n_valid"] == 500


def test_ks_prepare_and_argmax():
    """th_sorted stays with the context after ks_prepare (ks_argmax reads it): it is part of the baseline."""
    ctx, x = _ctx(), _scores()
    prep = _returns(ctx, lambda: ctx.ks_prepare(x, 0.5, ranks=(0, 499)))
    assert prep["order"][0] == x.min() and prep["order"][1] == x.max()
    i, score, d = _returns(ctx, lambda: ctx.ks_argmax(prep["bg_mean"], prep["bg_std"]))
    assert 0 <= i < x.size and d > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ks_classify(dtype):
    x = _scores(dtype)
    dev, lab, n_high = _returns(_ctx(), lambda: _ctx().ks_classify(x, 2.0, float(x.max())))
    assert n_high == int((x >= 2.0).sum())


def test_gmm_fit_and_posterior():
    ctx, x = _ctx(), _scores()
    draws = _random_draws(7, 2, 2)
    fit = _returns(ctx, lambda: ctx.gmm_fit(x, 2, 2, 300, 1e-4 * float(x.var()), x.mean(), draws))
    b = fit["best"]
    assert fit["converged"][b]
    high = [int(np.argmax(fit["means"][b]))]
    prob, lab, n_high = _returns(ctx, lambda: ctx.gmm_posterior(x, fit["weights"][b], fit["means"][b], fit["variances"][b], high, 0.5))
    assert 0 < n_high < x.size


@pytest.mark.parametrize("loss", ["frobenius", "kullback-leibler"])
def test_nmf_fit(loss):
    X = _counts()
    rng = np.random.default_rng(9)
    W0, H0 = rng.uniform(0.1, 1.0, (X.shape[0], K)), rng.uniform(0.1, 1.0, (K, X.shape[1]))
    out = _returns(_ctx(), lambda: _ctx().nmf_fit(X.indptr, X.indices, X.data, X.shape[1], W0, H0, loss, max_iter=20))
    assert out["n_iter"] >= 1 and out["error_trace"][-1] <= out["error_trace"][0]


def test_hvg_pearson():
    X = _counts()
    s, ss, rm, rv = _returns(_ctx(), lambda: _ctx().hvg_pearson(X.indptr, X.indices, X.data, X.shape[1], 100.0, float(np.sqrt(X.shape[0]))))
    np.testing.assert_array_equal(s, np.asarray(X.sum(axis=0)).ravel())


def _model(G):
    rng = np.random.default_rng(13)
    return rng.normal(0, 0.7, (T, G)), rng.normal(0, 1.0, T), np.full(G, 0.5), np.ones(G)


@pytest.mark.parametrize("scores", [True, False])
def test_annot_predict(scores):
    X = _counts()
    coef, b, mean, scale = _model(X.shape[1])
    out = _returns(_ctx(), lambda: _ctx().annot_predict(X.indptr, X.indices, X.data, "counts", coef, b, mean, scale, scores=scores))
    assert out["labels"].min() >= 0 and out["labels"].max() < T


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_annot_transform(dtype):
    S = np.random.default_rng(15).normal(0, 2.0, (500, T)).astype(dtype)
    out = _returns(_ctx(), lambda: _ctx().annot_transform(S))
    assert np.isfinite(out["softmax"]).all()


# ---- 2. resident problems --------------------------------------------------------------------------------------------------------------
def _resident(ctx, begin, end):
    """The life of a resident problem on the counter."""
    before = ctx.device_mem()
    try:
        begin()
        during = ctx.device_mem()
        assert during > before
        begin()                                   # a second begin replaces the problem
        assert ctx.device_mem() == during
    finally:
        end()
    assert ctx.device_mem() == before
    end()                                         # a second end is SC_OK (the wrapper raises on anything else) ...
    assert ctx.device_mem() == before             # ... and changes nothing


def test_pca_begin_and_end():
    ctx, X = _ctx(), _counts()
    for normalize in (False, True):
        _resident(ctx, lambda: ctx.pca_begin(X.indptr, X.indices, X.data, X.shape[1], normalize), ctx.pca_end)


def test_pca_scratch_of_gram_and_project_goes_with_the_problem():
    ctx, X = _ctx(), _counts()
    G = X.shape[1]
    before = ctx.device_mem()
    ctx.pca_begin(X.indptr, X.indices, X.data, G)
    try:
        begun = ctx.device_mem()
        ctx.pca_gram()
        ctx.pca_project(np.eye(2, G), np.zeros(2))
        assert ctx.device_mem() > begun
    finally:
        ctx.pca_end()
    assert ctx.device_mem() == before


def test_annot_train_begin_and_end():
    ctx, X = _ctx(), _counts()
    n, G = X.shape
    labels, weights = (np.arange(n) % T).astype(np.int32), np.ones(n)
    _resident(ctx, lambda: ctx.annot_train_begin(X.indptr, X.indices, X.data, G, "counts", T, labels, weights), ctx.annot_train_end)


def test_harmony_begin_and_end():
    ctx = _ctx()
    Z, batch, B, Y, nb, sigma, theta, lamb = H.case_inputs({c[0]: c for c in H.CASES}["pair"])
    _resident(ctx, lambda: ctx.harmony_begin(Z, batch, B, Y, nb, sigma, theta, lamb), ctx.harmony_end)


def test_louvain_begin_refused_on_the_device_returns_its_memory():
    """sc_louvain_begin_resident allocates level 0, uploads the weights and checks their symmetry on the device: weights
    that differ between an entry and its mirror are refused (SC_ERR_INVALID) once the state exists."""
    ctx = _ctx()
    ctx.knn_dense(blobs(400, 5, 4, 31, np.float64), 10, fetch=False)
    nnz = int(ctx.diffmap_graph()["n_edges"])
    g, max_rounds = 1 << 16, 500
    try:
        ctx.louvain_begin_resident(None, g, max_rounds)     # warm-up: the same allocations, accepted
    finally:
        ctx.louvain_end()
    before = ctx.device_mem()
    q = np.ones(nnz, dtype=np.uint16)
    q[0] = 2
    with pytest.raises(ValueError, match="not symmetric in structure and weight"):
        ctx.louvain_begin_resident(q, g, max_rounds)
    assert ctx.device_mem() == before
    ctx.louvain_end()
    assert ctx.device_mem() == before


# ---- 3. two contexts on one device -----------------------------------------------------------------------------------------------------
def test_closing_a_context_with_a_resident_problem_leaves_the_other_alone():
    from spatialcore_amd import _lib

    X, C = blobs(700, 5, 6, 24, np.float64), _counts()
    draws = _random_draws(24, 2, 6)
    a, b = _lib.Context(0), _lib.Context(0)
    try:
        first = _kmeans(b, X, 6, 300, draws)
        mem_b = b.device_mem()
        a.pca_begin(C.indptr, C.indices, C.data, C.shape[1])
        assert a.device_mem() > 0
        a.close()
        assert b.device_mem() == mem_b
        again = _kmeans(b, X, 6, 300, draws)
        np.testing.assert_array_equal(again["labels"], first["labels"])
        assert b.device_mem() == mem_b
    finally:
        a.close()
        b.close()
