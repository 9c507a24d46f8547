"""The byte-plane scoring kernel against the fp64-row kernel and the oracle (run with -m gpu on an MI355X).

An all-lattice uint8 batch on 16-bit neighbour sums is scored by k_moran_score_wg<8, 4, false, true> in 8-bit integer dot
products over blocks of four cells, as two byte planes S = lo + 256 hi (sc_moran.hip; the arithmetic is restated in
tests/test_cpu_moran_byte_planes.py).  Every output must be the fp64-row kernel's bit for bit and the oracle's on the very
graph, at the shapes where the kernel takes another path:

  ring degree 1 / 255 / 256 / 257   counts of 255; hi plane empty, S crossing 255 -> 256, S = 65535
  P = 24 / 40 / 128 / 152           workgroup form: 3 and 5 live wavefronts beside idle ones, a full task, a full and a short one
  P = 9                             the per-wavefront fallback kernel (fp64 products): equal to the workgroup form's rows
  n = 2310 / 2049 / 2064            second split of 16 super-blocks + a tail of 6 / of one cell (tail only) / of one super-block
  G = 130                           a second gene group with two genes

Tolerances are those of test_gpu_moran_limits.py: lattice counts ==, I at rtol 1e-9 / atol 1e-14, sims at rtol 1e-9 /
atol 1e-13."""
import numpy as np
import pytest

import moran_limits_inputs as mi
from test_gpu_moran_limits import assert_identical, assert_is_oracle, run

pytestmark = pytest.mark.gpu

G = mi.N_GENES
P_MAX = 152
DEGREES = (1, 255, 256, 257)


@pytest.fixture(scope="module")
def ctx():
    from spatialcore_amd import _lib

    c = _lib.default_context(0)
    yield c
    c.set_moran_source_bits(8)


def pattern_counts(n, genes):
    """cell c, gene g holds (37 c + 11 g) mod 251: the four bytes of every transposed word differ, and so do a row's genes"""
    return ((37 * np.arange(n)[:, None] + 11 * np.arange(genes)[None, :]) % 251).astype(np.float32)


@pytest.fixture(scope="module")
def inputs(oracle):
    """counts and permutation table (identity first) per (kind, n), made once"""
    cache = {}

    def get(kind, n):
        if (kind, n) not in cache:
            X = mi.saturating_counts(n, G, 1) if kind == "saturating" else pattern_counts(n, G)
            cache[kind, n] = (X, mi.identity_first(oracle.perm_table(11, n, P_MAX)[0]))
        return cache[kind, n]

    return get


@pytest.fixture(scope="module")
def reference(oracle, inputs):
    """Oracle results per (kind, n, degree), computed once for all P_MAX rows (a shorter table is their prefix)."""
    cache = {}

    def get(kind, n, d, P):
        X, perms = inputs(kind, n)
        if (kind, n, d) not in cache:
            g = mi.as_csr(mi.ring_graph(n, d, 1.0 / d), n)
            vals = oracle.dense_genes(X)
            cache[kind, n, d] = (g, vals, oracle.morans_i_scores(g, vals), oracle.morans_i_sims_gather(g, vals, perms))
        g, vals, I, sims = cache[kind, n, d]
        count, lat = oracle.morans_count_ge(g, vals, perms[:P], sims[:P], I)
        return {"I": I, "sims": sims[:P], "count_ge": count, "lattice": lat}

    return get


def check(ctx, inputs, reference, kind, n, d, P):
    X, perms = inputs(kind, n)
    parts = mi.ring_graph(n, d, 1.0 / d)
    tab = reference(kind, n, d, P)
    try:
        out8, path8 = run(ctx, 8, parts, X, perms[:P], n)
        out64, path64 = run(ctx, 64, parts, X, perms[:P], n)
    finally:
        ctx.set_moran_source_bits(8)
    what = f"{kind} counts, n={n} d={d} P={P}"
    assert path8[:2] == (8, 16) and path8[2] == 2, (what, path8)
    assert path64[:2] == (64, 64), (what, path64)
    assert_is_oracle(out8, tab, what)
    assert_identical(out8, out64, "byte planes vs fp64 rows: " + what)
    return out8


@pytest.mark.parametrize("P", [24, 40, 128, 152])
@pytest.mark.parametrize("d", DEGREES)
def test_workgroup_form_at_degree_and_chunk_edges(ctx, inputs, reference, d, P):
    check(ctx, inputs, reference, "saturating", mi.N_CELLS, d, P)


@pytest.mark.parametrize("d", DEGREES)
def test_fallback_kernel_equals_the_workgroup_form(ctx, inputs, reference, d):
    """P = 9 takes k_moran_score (fp64 products of the same integers); its rows are the first nine of the P = 24 run."""
    short = check(ctx, inputs, reference, "saturating", mi.N_CELLS, d, 9)
    full = check(ctx, inputs, reference, "saturating", mi.N_CELLS, d, 24)
    np.testing.assert_array_equal(short["sims"], full["sims"][:9])
    np.testing.assert_array_equal(short["I"], full["I"])


@pytest.mark.parametrize("P", [40, 152])
@pytest.mark.parametrize("d", DEGREES)
@pytest.mark.parametrize("n", [2049, 2064])
def test_second_split_of_one_cell_and_of_one_super_block(ctx, inputs, reference, n, d, P):
    assert mi.score_cells_per_split(n) == 2048
    check(ctx, inputs, reference, "saturating", n, d, P)


@pytest.mark.parametrize("d", DEGREES)
def test_counts_that_differ_in_every_transposed_byte(ctx, inputs, reference, d):
    X, _ = inputs("pattern", mi.N_CELLS)
    blocks = X[:mi.N_CELLS // 4 * 4].reshape(-1, 4, G)
    assert all((blocks[:, i] != blocks[:, j]).all() for i in range(4) for j in range(i))   # a word's four cells
    assert all((X[:, 2 * k] != X[:, 2 * k + 1]).all() for k in range(G // 2))               # a lag word's two genes
    check(ctx, inputs, reference, "pattern", mi.N_CELLS, d, 152)
