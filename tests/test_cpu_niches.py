"""CPU tests of identify_niches: the numpy restatement of sc_kmeans_fit against the reference's own results
(tests/golden/ref_niches.npz, scripts/make_niche_golden.py) and the request validation, which runs before any device
call."""
import numpy as np
import pandas as pd
import pytest

import kmeans_restated as kr
from conftest import load_golden

G = load_golden("ref_niches.npz")
CASES = [str(c) for c in G["cases"]]
# cases whose Lloyd passes meet ties that float32 and fp64 break differently (see the test)
LATTICE_TIES = {"knn_k8", "raw_k12", "knn_k8_iter2"}


def _case(name):
    P = G[f"profile_{G[f'{name}_kind']}"]
    K, n_init, rs, max_iter = (int(G[f"{name}_{k}"]) for k in ("n_niches", "n_init", "random_state", "max_iter"))
    return P, K, n_init, rs, max_iter


def ari(a, b):
    """Adjusted Rand index (Hubert and Arabie)."""
    ct = pd.crosstab(np.asarray(a), np.asarray(b)).to_numpy().astype(np.float64)
    comb = lambda x: x * (x - 1) / 2.0  # noqa: E731
    s_ij = comb(ct).sum()
    s_a, s_b = comb(ct.sum(axis=1)).sum(), comb(ct.sum(axis=0)).sum()
    expected = s_a * s_b / comb(ct.sum())
    top = 0.5 * (s_a + s_b)
    return 1.0 if top == expected else (s_ij - expected) / (top - expected)


@pytest.mark.parametrize("name", CASES)
def test_restated_kmeans_matches_reference(name):
    from spatialcore_amd.spatial.neighborhoods import kmeans_draws

    P, K, n_init, rs, max_iter = _case(name)
    fit = kr.fit(P, K, n_init, max_iter, kmeans_draws(rs, n_init, K))
    stable = G[f"{name}_seed_stable"]
    ref_seeds = G[f"{name}_seeds"]
    np.testing.assert_array_equal(fit["seeds"][stable], ref_seeds[stable])
    if name.startswith("dup"):
        assert ari(fit["labels"], G[f"{name}_labels"]) == 1.0
        assert fit["distinct"] < K
        return
    if name in LATTICE_TIES:
        # profiles on the lattice k / 15: sklearn's float32 assignment breaks exact-arithmetic ties between centres by
        # its own rounding, the fp64 one by another, and the runs then part; same seeds, close optima
        assert abs(fit["inertia"] / float(G[f"{name}_inertia"]) - 1.0) < 2e-2
        return
    assert np.array_equal(fit["seeds"], ref_seeds) and float(G[f"{name}_label_margin"]) > 1e-5
    assert ari(fit["labels"], G[f"{name}_labels"]) == 1.0
    # the stop on tolerance may come one Lloyd pass apart (a near-tie cell moved by float32 rounding): ~1e-4
    np.testing.assert_allclose(fit["centers"], G[f"{name}_centroids"], rtol=0, atol=1e-3)
    np.testing.assert_allclose(fit["inertia"], float(G[f"{name}_inertia"]), rtol=1e-5)


def test_first_centre_rule_is_numpy_choice():
    for n, dtype, seed in ((7, np.float32, 0), (6000, np.float32, 3), (1001, np.float64, 5)):
        rs = np.random.RandomState(seed)
        w = np.ones(n, dtype=dtype)
        state = rs.get_state()
        ref = rs.choice(n, p=w / w.sum())
        rs.set_state(state)
        assert kr.first_index(rs.random_sample(), n, dtype) == ref


def test_draws_are_the_kmeanspp_stream():
    """kmeans_draws replays the RandomState calls of k-means++: one random_sample, then uniform(size=L) per centre."""
    from spatialcore_amd.spatial.neighborhoods import kmeans_draws

    d = kmeans_draws(4, 3, 8)
    L = 2 + int(np.log(8))
    assert d.shape == (3, 1 + 7 * L)
    rs = np.random.RandomState(4)
    flat = rs.random_sample(3 * (1 + 7 * L))
    np.testing.assert_array_equal(d.ravel(), flat)


def _adata(n=40, C=4, key="neighborhood_profile", zero_rows=0):
    from spatialcore_amd import SimpleAnnData

    P = np.random.default_rng(0).random((n, C)).astype(np.float32) + 0.1
    P[:zero_rows] = 0
    return SimpleAnnData(np.zeros((n, 1)), var_names=["g0"], obsm={key: P})


@pytest.mark.parametrize("kwargs,adata_kw,message", [
    (dict(n_niches=3), dict(key="other"),
     "adata.obsm['neighborhood_profile'] not found. Run compute_neighborhood_profile() first."),
    (dict(n_niches=3, method="dbscan"), {}, "Invalid method: 'dbscan'. Must be 'kmeans' or 'minibatch_kmeans'."),
    (dict(n_niches=1), {}, "n_niches must be >= 2, got 1"),
    (dict(n_niches=41), {}, "n_niches (41) cannot exceed number of cells (40)"),
    (dict(n_niches=3), dict(zero_rows=2),
     "2 cells have empty neighborhood profiles. Increase radius, switch to knn, or pre-filter isolated cells "
     "before profiling."),
    # the reference's order: the key before the method, the method before n_niches
    (dict(n_niches=1, method="dbscan"), dict(key="other"),
     "adata.obsm['neighborhood_profile'] not found. Run compute_neighborhood_profile() first."),
    (dict(n_niches=1, method="dbscan"), {}, "Invalid method: 'dbscan'. Must be 'kmeans' or 'minibatch_kmeans'."),
])
def test_identify_niches_validation_messages(kwargs, adata_kw, message, monkeypatch):
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import identify_niches

    def no_device(*a, **k):
        raise AssertionError("validation must happen before any device call")

    monkeypatch.setattr(_lib, "default_context", no_device)
    with pytest.raises(ValueError) as e:
        identify_niches(_adata(**adata_kw), **kwargs)
    assert str(e.value) == message
