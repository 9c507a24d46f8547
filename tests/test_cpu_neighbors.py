"""sc_knn_dense_gram's arithmetic on the host (tests/neighbors_restated.py): the filter's error bound
against the direct form and against exact rational arithmetic, the certification rule against the exact search, the
margins the GPU tests' certification counts rest on, and the argument checks of ``neighbors``."""
import functools
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import diffusion_restated as R
import neighbors_restated as N
from spatialcore_amd import SimpleAnnData, _lib
from spatialcore_amd.neighbors import neighbors

ORDERS = ("matmul", "reversed", "pairwise")
NAMES = ("pca_like", "offset_1e3", "offset_1e6", "float32", "traj", "lattice", "tiny", "huge")


@functools.lru_cache(maxsize=None)
def _recipe(name):
    n = 2000 if name in ("traj", "lattice") else 1000
    X = N.recipes(n)[name]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _truth(name, k):
    return R.knn(_recipe(name), k)


# ---- the bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bound_holds_for_every_pair_in_three_orders(name):
    X = _recipe(name)
    n = X.shape[0]
    worst = 0.0
    for b in range(0, n, 500):
        rows = np.arange(b, min(b + 500, n))
        d2 = N.direct(X, rows)
        for order in ORDERS:
            s, E, lo = N.bounds(X, rows, order)
            assert np.all(np.isfinite(s)) and np.all(E > 0)
            ratio = np.abs(s - d2) / E
            worst = max(worst, float(ratio.max()))
            assert np.all(np.abs(s - d2) <= E), (name, order, float(ratio.max()))
            assert np.all(lo <= d2)
    print(f"{name}: worst |s - d2_dev| / E over {n * n} pairs and {len(ORDERS)} orders = {worst:.3g}")


@pytest.mark.parametrize("name", NAMES)
def test_bound_against_exact_rational_arithmetic(name):
    """Both error terms of the derivation, measured against the exact d2 of the float64 inputs: |s - d2| + |d2_dev - d2| <= E."""
    X = np.asarray(_recipe(name), dtype=np.float64)
    n = X.shape[0]
    rng = np.random.default_rng(5)
    rows = rng.integers(0, n, 40)
    cols = rng.integers(0, n, 40)
    cols[:4] = rows[:4]                       # the diagonal too: d2 = 0 exactly
    d2_dev = N.direct(X, rows)
    per_order = [N.bounds(X, rows, order) for order in ORDERS]
    worst = Fraction(0)
    for p, (i, j) in enumerate(zip(rows, cols)):
        exact = sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(X[i], X[j]))
        for s, E, _ in per_order:
            err = abs(Fraction(float(s[p, j])) - exact) + abs(Fraction(float(d2_dev[p, j])) - exact)
            assert err <= Fraction(float(E[p, j])), (name, int(i), int(j))
            worst = max(worst, err / Fraction(float(E[p, j])))
    print(f"{name}: worst (|s - d2| + |d2_dev - d2|) / E over {3 * rows.size} exact pairs = {float(worst):.3g}")


# ---- the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slack", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_filter_rerank_and_fallback_equal_the_exact_search(name, slack):
    X, k = _recipe(name), 15
    ti, td = _truth(name, k)
    idx, d2, certified, _ = N.filtered_knn(X, k, slack)
    wrong = certified & (np.any(idx != ti, axis=1) | np.any(d2 != td, axis=1))
    print(f"{name}, slack {slack}: {int((~certified).sum())} of {X.shape[0]} rows uncertified, {int(wrong.sum())} certified rows differ")
    assert not wrong.any()
    fi, fd = N.with_fallback(X, k, idx, d2, certified)
    assert np.array_equal(fi, ti) and np.array_equal(fd, td)


# ---- the conditions the GPU tests' counts rest on -----------------------------------------------------------------------
@pytest.mark.parametrize("slack", [1, 0])
@pytest.mark.parametrize("k", [15, 32])
def test_pca_like_rows_are_certified_with_a_wide_margin(k, slack):
    """The sample on which tests/test_gpu_neighbors.py asserts rows_fallback == 0, at both k, with one slack entry and
    with the default: every margin is at least 1e6 of the row's largest E, so no count there can hinge on a rounding."""
    X = N.pca_like(3000, 50, N.CERT_SEED)
    nrm = N.norms(X)
    e_max = (N.c_e(50) * 2.0 ** -52) * (nrm + nrm.max()) + N.TINY     # max_j E_ij of row i
    idx, d2, certified, margin = N.filtered_knn(X, k, slack)
    value = (margin / e_max).min()
    print(f"pca_like n=3000, k={k}, slack={slack}: min_i (lo_(L) - D) / max E = {value:.3g}")
    assert certified.all()
    assert value >= 1e6


def test_forty_fold_duplicates_certify_no_row():
    X, k = N.duplicates(100, 40, 50, 0), 15
    for slack in (1, 0):
        assert k + (slack or N.SLACK_DEFAULT) < 39
        _, _, certified, _ = N.filtered_knn(X, k, slack)
        assert not certified.any()


@pytest.mark.parametrize("d, dtype, k, slack, m", N.LISTED_EDGE, ids=N.LISTED_EDGE_IDS)
def test_far_copies_leave_exactly_the_copies_uncertified(d, dtype, k, slack, m):
    """The samples on which tests/test_gpu_neighbors.py asserts rows_fallback == m: the m copies miss the certificate
    (D = 0 and lo_(L) <= 0, whatever the rounding), every other row's margin is at least 1e6 of its largest E.

    A row's largest E is taken in two parts, since E_ij grows with |x_j|^2 and a copy's norm is 1e6.  Among the first 1000
    cells, which decide the row's kept list and its L-th key: margin >= 1e6 max_j E_ij.  The copies: their lo lies beyond
    the row's L-th key by at least 1e6 of their own (larger) E, so no rounding brings one of them into the kept list."""
    X = N.far_copies(d, m, dtype)
    nrm = N.norms(X)
    ce = N.c_e(d) * 2.0 ** -52
    e_near = ce * (nrm[:1000] + nrm[:1000].max()) + N.TINY
    e_far = ce * (nrm[:1000] + nrm[1000]) + N.TINY
    _, d2, certified, margin = N.filtered_knn(X, k, slack)
    lo_L = margin[:1000] + d2[:1000, k - 1]
    lo_far = R.pair_d2(X, np.arange(1000), np.full(1000, 1000)) - e_far
    near, far = (margin[:1000] / e_near).min(), ((lo_far - lo_L) / e_far).min()
    print(f"far_copies d={d}, k={k}, slack={slack}, m={m}: over the first 1000 rows min (lo_(L) - D) / max E = {near:.3g}, "
          f"min (lo_copy - lo_(L)) / E_copy = {far:.3g}")
    assert certified[:1000].all() and not certified[1000:].any()
    assert near >= 1e6 and far >= 1e6
    assert np.all(d2[1000:] == 0.0) and np.all(margin[1000:] <= 0.0)


@pytest.mark.parametrize("k, slack, m", [(15, 0, 23), (2, 1, 3)])
def test_far_copies_no_more_than_the_list_holds_are_certified(k, slack, m):
    """The control: m = L copies have L - 1 twins each, so the L-th kept candidate is a distant cell and every row is certified."""
    _, _, certified, _ = N.filtered_knn(N.far_copies(50, m), k, slack)
    assert certified.all()


def test_lattice_certifies_some_rows_and_not_others():
    X = _recipe("lattice")
    _, _, certified, margin = N.filtered_knn(X, 15, 0)
    missed = int((~certified).sum())
    print(f"lattice: {missed} of {X.shape[0]} rows uncertified at the default slack")
    assert 0 < missed < X.shape[0]
    # integer squared distances: a margin is an integer up to E, never a rounding away from zero
    assert np.all(np.abs(margin - np.rint(margin)) < 1e-6)


def test_wide_lattice_sends_rows_through_the_fallback_without_a_zero_scale():
    """The second input of the drivers' tests in tests/test_gpu_neighbors.py, at the size where path 0 takes the filter: a
    row whose k-th and L-th kept distances tie (margin <= 0 at integer distances, whatever the rounding) misses the
    certificate, and no cell has the 8 twins that would make the median of its 15 neighbour distances zero."""
    X, k = N.lattice_wide(10000, 2), 15
    assert X.shape == (10000, 40)
    _, _, certified, margin = N.filtered_knn(X, k, 0)
    tied = int(np.count_nonzero(margin < 0.5))
    print(f"wide lattice: {int((~certified).sum())} of 10000 rows uncertified, {tied} of them by a tie")
    assert tied > 0 and not certified[margin < 0.5].any()
    assert np.unique(X, axis=0, return_counts=True)[1].max() <= k // 2


# ---- the public function on the host ------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")

    monkeypatch.setattr(_lib, "default_context", refuse)


def _adata(n=40, **obsm):
    X = R.traj(n, 3, 0)[0]
    obs = pd.DataFrame(index=[f"cell{i}" for i in range(n)])
    return SimpleAnnData(np.zeros((n, 2)), obs=obs, obsm={"X_pca": X, **obsm})


@pytest.mark.parametrize("kwargs, message", [
    (dict(n_neighbors=1), "n_neighbors must be an integer in 2..32"),
    (dict(n_neighbors=33), "n_neighbors must be an integer in 2..32"),
    (dict(n_neighbors=40), "below the 40 cells"),
    (dict(n_neighbors=15.0), "n_neighbors must be an integer"),
    (dict(n_neighbors=True), "n_neighbors must be an integer"),
    (dict(use_rep="missing"), "is not an entry of adata.obsm"),
    (dict(use_rep="wide"), "has 65 columns"),
    (dict(use_rep="flat"), "must be a real 2-D array"),
    (dict(use_rep="nan"), "contains NaN or infinite values"),
    (dict(use_rep="huge"), "magnitude 2^500 or more"),
    (dict(key_added=""), "key_added must be a non-empty string"),
    (dict(key_added=3), "key_added must be a non-empty string"),
])
def test_argument_errors_come_before_a_context_exists(no_device, kwargs, message):
    base = R.traj(40, 3, 0)[0]
    bad = base.copy()
    bad[39, 2] = np.nan
    big = base.copy()
    big[0, 0] = 2.0 ** 500
    ad = _adata(wide=np.zeros((40, 65)), flat=np.zeros(40), nan=bad, huge=big)
    with pytest.raises(ValueError) as err:
        neighbors(ad, **kwargs)
    assert message in str(err.value)
    assert not ad.obsp and "neighbors" not in ad.uns


def test_neighbors_is_exported():
    import spatialcore_amd

    assert "neighbors" in spatialcore_amd.__all__
    assert spatialcore_amd.neighbors.neighbors is neighbors
