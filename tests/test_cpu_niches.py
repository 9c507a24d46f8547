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


def blobs(n, C, K, seed, dtype, spread=1.0, noise=0.6):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, spread, (K, C))
    X = centres[rng.integers(0, K, n)] + rng.normal(0, noise, (n, C))
    return X.astype(dtype)


# n, C, K, n_init, max_iter, dtype, seed: the shapes the kernels are compared with the restatement on
BLOB_SHAPES = [
    (3000, 6, 5, 10, 300, np.float32, 1),
    (3000, 6, 5, 10, 300, np.float64, 2),       # float64 input: no float32 rounding of D^2 or the potential
    (2500, 3, 9, 4, 300, np.float32, 3),        # K > C
    (2000, 100, 40, 2, 300, np.float32, 4),     # the general path (C > 64)
    (5000, 8, 6, 1, 300, np.float32, 5),        # n_init = 1
    (3000, 6, 5, 10, 1, np.float32, 6),         # max_iter = 1: no convergence, the final E-step
    (9000, 5, 70, 2, 300, np.float64, 7),       # K > 64: the general path, several seeding groups
]


@pytest.mark.parametrize("name", CASES)
def test_restated_kmeans_matches_reference(name):
    _check_against_reference(name, kernel_order=False)


@pytest.mark.parametrize("name", CASES)
def test_kernel_order_restatement_matches_reference(name):
    _check_against_reference(name, kernel_order=True)


def _check_against_reference(name, kernel_order):
    from spatialcore_amd.spatial.neighborhoods import kmeans_draws

    P, K, n_init, rs, max_iter = _case(name)
    fit = kr.fit(P, K, n_init, max_iter, kmeans_draws(rs, n_init, K), kernel_order=kernel_order)
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


@pytest.mark.parametrize("n,C,K,n_init,max_iter,dtype,seed", BLOB_SHAPES)
def test_kernel_order_and_point_order_agree(n, C, K, n_init, max_iter, dtype, seed):
    """The two modes differ in summation order alone: the same seeds, labels and stopping, and centres that agree to
    1 ulp of float32 (float64 centres are compared after rounding to float32)."""
    from spatialcore_amd.spatial.neighborhoods import kmeans_draws

    X = blobs(n, C, K, seed, dtype)
    draws = kmeans_draws(seed, n_init, K)
    a = kr.fit(X, K, n_init, max_iter, draws)
    b = kr.fit(X, K, n_init, max_iter, draws, kernel_order=True)
    np.testing.assert_array_equal(a["seeds"], b["seeds"])
    np.testing.assert_array_equal(a["labels"], b["labels"])
    assert (a["n_iter"], a["strict"], a["best_run"]) == (b["n_iter"], b["strict"], b["best_run"])
    ca, cb = a["centers"].astype(np.float32), b["centers"].astype(np.float32)
    assert np.all(np.abs(ca - cb) <= np.spacing(np.maximum(np.abs(ca), np.abs(cb))))


def test_kernel_order_sums_are_the_stated_loops():
    """_wg_sums, _wg_inertia and _thread_shift against plain Python loops in the orders the module docstring states, on
    sizes with several tiles per workgroup, a ragged last tile and more than 256 (cluster, feature) pairs."""
    rng = np.random.default_rng(0)
    n, C, K, nb = 1100, 3, 4, 2             # 5 tiles: workgroup 0 has tiles 0, 2, 4 (76 points), workgroup 1 has 1, 3
    X = rng.normal(0, 1, (n, C)) * 10.0 ** rng.integers(-6, 6, (n, C))
    labels = rng.integers(0, K, n)
    sums = np.zeros((K, C))
    for b in range(nb):
        part = np.zeros((K, C))
        for tile in range(b, -(-n // 256), nb):
            for p in range(tile * 256, min(n, tile * 256 + 256)):
                for c in range(C):
                    part[labels[p], c] = part[labels[p], c] + X[p, c]
        sums = sums + part
    got = kr._wg_sums(X, labels, K, nb)
    np.testing.assert_array_equal(got, sums)
    flat = np.zeros((K, C))
    np.add.at(flat, labels, X)
    assert not np.array_equal(got, flat)    # the order matters on this input

    d = np.abs(X[:, 0])
    total = 0.0
    for b in range(nb):
        threads = [0.0] * 256
        for tile in range(b, -(-n // 256), nb):
            for tid in range(256):
                if tile * 256 + tid < n:
                    threads[tid] = threads[tid] + d[tile * 256 + tid]
        wg = 0.0
        for t in threads:
            wg = wg + t
        total = total + wg
    assert kr._wg_inertia(d, nb) == total
    assert total != float(np.add.accumulate(d)[-1])

    new, old = rng.normal(0, 1, (5, 130)), rng.normal(0, 1, (5, 130))
    dd = (new - old).ravel()
    threads = [0.0] * 256
    for i in range(dd.size):
        threads[i % 256] = threads[i % 256] + dd[i] * dd[i]
    s = 0.0
    for t in threads:
        s = s + t
    assert kr._thread_shift(new, old) == s


def test_workgroups_per_run():
    assert kr.workgroups(3000, 6, 5, 1) == kr.workgroups(3000, 6, 5, 3) == 12      # one tile each
    assert kr.workgroups(65536, 4, 3, 2) == 256 and kr.workgroups(65537, 4, 3, 2) == 256
    assert kr.workgroups(4, 3, 4, 3) == 1
    assert kr.workgroups(10 ** 6, 200, 200, 10) == (1 << 25) // (4 * 10 ** 5) == 83  # the partial sums' bound


def test_draws_for_seeds_and_tie_draws():
    X = blobs(4200, 3, 4, 8, np.float32)
    Xc = X - X.mean(axis=0)
    seeds = [4199, 0, 63, 4096]
    d = kr.draws_for_seeds(Xc, seeds)
    assert d.shape == (1 + 3 * 3,) and np.all((0 <= d) & (d < 1))
    np.testing.assert_array_equal(kr.seeding(Xc, 4, d), seeds)
    with pytest.raises(ValueError):
        kr.draws_for_seeds(Xc, [5, 7, 5, 9])         # a centre cannot be drawn twice: its D^2 is 0
    # integer D^2: every order gives the same prefix, and numpy's flat searchsorted is the oracle of a tie draw
    D = np.random.default_rng(1).integers(0, 50, 9000).astype(np.float32)
    D[200:230] = 0
    pre = np.cumsum(D.astype(np.float64))
    np.testing.assert_array_equal(kr.flat_prefix(D), pre)
    pot = float(np.float32(pre[-1]))
    assert pot == pre[-1]
    i, u = kr.tie_draws(D, pot)
    assert i.size > 100 and np.all(u * pot == pre[i])
    for ii, uu in zip(i[::7], u[::7]):
        assert kr.search(D, uu * pot) == np.searchsorted(pre, uu * pot, side="left") <= ii


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
