"""The inputs of tests/test_gpu_moran_limits.py are what those tests say they are -- against the oracle alone, no GPU."""
import numpy as np
import pytest

import moran_limits_inputs as mi

N, G = mi.N_CELLS, mi.N_GENES


@pytest.fixture(scope="module")
def X():
    return mi.saturating_counts(N, G, 1)


def test_ring_graph_is_regular_uniform_and_sorted():
    for n, d in ((7, 0), (7, 1), (7, 6), (N, 257)):
        indptr, indices, data = mi.ring_graph(n, d, 0.25)
        assert (np.diff(indptr) == d).all() and indices.size == n * d and (data == 0.25).all()
        rows = indices.reshape(n, d) if d else indices.reshape(n, 0)
        assert (np.diff(rows, axis=1) > 0).all()                         # strictly ascending: no duplicate, no self-loop
        want = (np.arange(n)[:, None] + np.arange(1, d + 1)[None, :]) % n
        np.testing.assert_array_equal(rows, np.sort(want, axis=1))
        assert not (rows == np.arange(n)[:, None]).any()


def test_saturating_counts_recipe(X):
    assert X.dtype == np.float32 and X.shape == (N, G)
    assert (X == np.floor(X)).all() and X.min() >= 0
    assert (X[300:, ::2] == 255).all() and (X[:300, ::2].max(axis=0) <= 255).all()
    assert (X[:300, ::2].std(axis=0) > 50).all()                         # the even genes do have a variance
    assert X[:, 1::2].max() <= 15 and (X[:, 1::2].max(axis=0) >= 4).all()
    assert int((X.max(axis=0) >= 16).sum()) == 65                        # 130 + 65 nibble slots: ONE 256-slot row group
    assert -(-(G + 65) // 256) == 1 and -(-G // 128) == 2


@pytest.mark.parametrize("d,top", [(255, 65025), (256, 65280), (257, 65535), (258, 65790)])
def test_neighbour_sums_reach_the_16_bit_limit(X, d, top):
    S = np.asarray(mi.adjacency(mi.ring_graph(N, d, 1.0 / d), N) @ X.astype(np.float64))
    assert S.max() == top == 255 * d
    assert ((S[:, ::2] == top).sum(axis=0) > 1000).all()                 # most cells of every even gene sit at the top
    assert S[:, 1::2].max() < 15 * d                                     # their packed neighbours stay small
    assert (top <= 65535) == mi.u8_prelude_allowed(d)


def test_nibble_guard_flips_between_255_and_256():
    for n in (1, N, 4096, 70001, (1 << 20) - 1):
        assert mi.score_cells_per_split(n) == 2048
        for d in (1, 15, 16, 17, 32, 33, 254, 255):
            assert mi.nibble_guard(255, d, n), (n, d)
        for d in (256, 257, 258, 1000):
            assert not mi.nibble_guard(255, d, n), (n, d)
    assert mi.score_cells_per_split(1 << 21) == 4096 and mi.score_cells_per_split((1 << 20) + 1) == 2056


def test_worst_nibble_accumulator_is_near_its_top(X):
    worst = mi.worst_nibble_sum(mi.ring_graph(N, 255, 1.0 / 255), X, N)
    print(f"worst per-split sum of 15 S at d = 255: {worst:.4e}")
    assert 0.85 * 2.0 ** 31 < worst < 2.0 ** 31
    assert worst < mi.NIBBLE_LIMIT                                       # ... and the host's bound does cover it


def test_straddling_genes_lie_on_either_side_of_the_lattice_bound():
    x = mi.straddling_genes(4096, 257)
    assert (x == np.floor(x)).all() and x.min() >= 0 and (x.max(axis=0) == 65535).all()
    assert tuple(int(s) for s in x.sum(axis=0)) == mi.STRADDLE_TOTALS
    below, above = mi.lattice_product(257, x[:, 0]), mi.lattice_product(257, x[:, 1])
    assert below == 257.0 * 65535.0 * 237_400_000 and above == 257.0 * 65535.0 * 237_600_000
    assert below < mi.LATTICE_LIMIT < above
    np.testing.assert_allclose([below, above], [3.9984e15, 4.0018e15], rtol=1e-4)
    assert abs(below / mi.LATTICE_LIMIT - 1) > 3e-4 and abs(above / mi.LATTICE_LIMIT - 1) > 3e-4
    assert above < 2.0 ** 53                                             # (the bound itself is conservative)


def _families():
    Xs = mi.saturating_counts(N, G, 1).astype(np.float64)
    for d in (1, 17, 255, 257, 258):
        yield f"ring d={d}", N, mi.ring_graph(N, d, 1.0 / d), Xs[:, [0, 1, 2, 127, 128, 129]]
    indptr, indices, data = mi.ring_graph(N, 16, 1.0 / 16)
    data = data.copy(); data[-1] = np.nextafter(data[-1], 1.0)
    yield "ring d=16, one weight an ulp off", N, (indptr, indices, data), Xs[:, [0, 1, 128]]
    indptr = indptr.copy(); indptr[-1] -= 1
    yield "ring d=16, last row short", N, (indptr, indices[:-1], mi.ring_graph(N, 16, 1.0 / 16)[2][:-1]), Xs[:, [0, 1, 128]]
    yield "straddling genes", 4096, mi.ring_graph(4096, 257, 1.0 / 257), mi.straddling_genes(4096, 257)


@pytest.mark.parametrize("case", range(8))
def test_oracle_sweep_and_gather_form_agree(oracle, case):
    """The oracle's literal row-permuted sweep (scanpy's loop on g[perm, :]) and its gather form, which the GPU tests
    compare with, agree at the GPU tests' tolerance on every input family; an identity row counts as a tie."""
    name, n, parts, X = list(_families())[case]
    g = mi.as_csr(parts, n)
    vals = oracle.dense_genes(X)
    perms = mi.identity_first(oracle.perm_table(5, n, 4)[0])
    I = oracle.morans_i_scores(g, vals)
    sims = oracle.morans_i_sims_gather(g, vals, perms)
    lit = np.stack([oracle.morans_i_scores(g, vals, perms[p]) for p in range(perms.shape[0])])
    np.testing.assert_allclose(sims, lit, rtol=1e-9, atol=1e-13, err_msg=name)
    np.testing.assert_allclose(sims[0], I, rtol=1e-9, atol=1e-14, err_msg=name)
    count, lat = oracle.morans_count_ge(g, vals, perms, sims, I)
    uniform_regular = "ulp" not in name and "short" not in name
    assert lat.all() == uniform_regular and lat.any() == uniform_regular, name
    assert (count[lat] >= 1).all(), name                                 # the identity row: T_p == T_obs, counted
    if name == "straddling genes":
        assert (np.abs(I) > 0.9).all()                                   # (what keeps the near-tie rule meaningful)
        near = (np.abs(sims - I) <= 1e-11 * np.abs(I)).sum(axis=0)
        assert (near >= 1).all()                                         # the identity row is within the near-tie rule
