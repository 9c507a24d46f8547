"""The global Moran prelude at the limits its host-side guards protect (run with -m gpu on an MI355X).

moran_prepare (sc_moran.hip) chooses the prelude and scoring kernels from the degree of the graph, the range of the counts
and the sums a task can reach; every choice keeps an integer from overflowing.  Each guard gets a case on either side, the
case asserts which path ran (moran_source_bits / moran_lag_bits / moran_row_groups), and the numbers are the oracle's on
the very graph (oracle/oracle.py: morans_i_scores, morans_i_sims_gather, morans_count_ge, graph_moments):

  guard                                           last shape inside            first shape outside
  degree <= 257 (packed 16-bit neighbour sums)    ring d = 257, counts 255     d = 258 (fp64 lag rows)
  15 xmax d cells_per_split < 2e9 (nibble sums)   d = 255, counts 255          d = 256 (uint8 source, 16-bit lag)
  d xmax[g] xsum[g] < 4.0e15 (exact lattice)      total 237 400 000            total 237 600 000 (centred arithmetic)
  one weight and one degree (the lattice itself)  ring d = 16                  one weight an ulp off / one row short

The inputs are proven to be what is said of them in tests/test_cpu_moran_limits.py.  Tolerances are those of
test_gpu_kernels.py: lattice counts ==, I at rtol 1e-9 / atol 1e-14, sims at rtol 1e-9 / atol 1e-13, other counts by
assert_counts_match."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import moran_limits_inputs as mi
from conftest import synth
from test_gpu_kernels import assert_counts_match

pytestmark = pytest.mark.gpu

N, G = mi.N_CELLS, mi.N_GENES
P_MAX = 40
KEYS = ("I", "sims", "count_ge", "sim_sum", "sim_sumsq")


@pytest.fixture(scope="module")
def ctx():
    from spatialcore_amd import _lib

    c = _lib.default_context(0)
    yield c
    c.set_moran_source_bits(8)


@pytest.fixture(scope="module")
def X():
    return mi.saturating_counts(N, G, 1)


@pytest.fixture(scope="module")
def perms(oracle):
    return mi.identity_first(oracle.perm_table(11, N, P_MAX)[0])


@pytest.fixture(scope="module")
def reference(oracle, X, perms):
    """Oracle results per graph, computed once per ring degree for all P_MAX rows (a shorter table is their prefix)."""
    cache = {}

    def get(key, parts, P):
        if key not in cache:
            g = mi.as_csr(parts, N)
            vals = oracle.dense_genes(X)
            cache[key] = (g, vals, oracle.morans_i_scores(g, vals), oracle.morans_i_sims_gather(g, vals, perms))
        g, vals, I, sims = cache[key]
        count, lat = oracle.morans_count_ge(g, vals, perms[:P], sims[:P], I)
        return {"I": I, "sims": sims[:P], "count_ge": count, "lattice": lat}

    return get


def run(ctx, bits, parts, X, table, n=N):
    """One sc_moran on a CSR graph; returns the outputs and (source bits, lag bits, row groups) of the path that ran."""
    ctx.set_moran_source_bits(bits)
    ctx.set_graph_csr(*parts, n)
    ctx.set_expression(X, np.arange(X.shape[1]))
    ctx.set_permutations(table)
    out = ctx.moran(table.shape[0])
    return out, (ctx.moran_source_bits(), ctx.moran_lag_bits(), ctx.moran_row_groups())


def assert_identical(a, b, what):
    for key in KEYS:
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{key}: {what}")


def assert_is_oracle(out, tab, what, exact_counts=True):
    np.testing.assert_allclose(out["I"], tab["I"], rtol=1e-9, atol=1e-14, err_msg=what)
    np.testing.assert_allclose(out["sims"], tab["sims"], rtol=1e-9, atol=1e-13, err_msg=what)
    if exact_counts:
        assert tab["lattice"].all(), what
        np.testing.assert_array_equal(out["count_ge"], tab["count_ge"], err_msg=what)
        assert (out["count_ge"] >= 1).all(), what                # the identity row is an exact tie, and a tie counts
    else:
        assert_counts_match(out["count_ge"], tab)


@pytest.mark.parametrize("P", [9, 40])      # the per-wavefront form and the workgroup form of the scoring kernel
@pytest.mark.parametrize("d", [1, 16, 17, 255, 256, 257, 258])
def test_uint8_prelude_at_degree_edges(ctx, reference, X, perms, d, P):
    """Neighbour sums of uint8 counts as packed 16-bit halves (k_lag_u8) up to 255 x 257 = 65535, the fp64 lag rows from
    degree 258: statistics and counts are the oracle's and bit-identical to the fp64-row kernel's."""
    parts = mi.ring_graph(N, d, 1.0 / d)
    tab = reference(d, parts, P)
    try:
        out8, path8 = run(ctx, 8, parts, X, perms[:P])
        out64, path64 = run(ctx, 64, parts, X, perms[:P])
    finally:
        ctx.set_moran_source_bits(8)
    assert path8[0] == 8 and path8[1] == (16 if d <= 257 else 64) and path8[2] == 2, path8
    assert path64[0] == 64 and path64[1] == 64, path64
    assert_is_oracle(out8, tab, f"d={d} P={P}")
    assert_identical(out8, out64, f"uint8 source vs fp64 rows, d={d} P={P}")


def test_uint8_prelude_degree_257_seeded_pipeline(ctx, oracle, X):
    """The same limit through sc_moran_seeded (numpy stream, no identity row) against sc_moran on the fetched table."""
    from spatialcore_amd._lib import rng_state_words

    P = 40
    parts = mi.ring_graph(N, 257, 1.0 / 257)
    ctx.set_moran_source_bits(8)
    ctx.set_graph_csr(*parts, N)
    ctx.set_expression(X, np.arange(G))
    w1 = rng_state_words(np.random.default_rng(7))
    table = ctx.generate_permutations(w1, N, P, fetch=True)
    two = ctx.moran(P)
    assert (ctx.moran_source_bits(), ctx.moran_lag_bits()) == (8, 16)
    w2 = rng_state_words(np.random.default_rng(7))
    one = ctx.moran_seeded(w2, P)
    assert (ctx.moran_source_bits(), ctx.moran_lag_bits()) == (8, 16)
    np.testing.assert_array_equal(w1, w2)
    np.testing.assert_array_equal(table, oracle.perm_table(7, N, P)[0])
    assert_identical(one, two, "sc_moran_seeded vs sc_moran")
    g, vals = mi.as_csr(parts, N), oracle.dense_genes(X)
    I, sims = oracle.morans_i_scores(g, vals), oracle.morans_i_sims_gather(g, vals, table)
    count, lat = oracle.morans_count_ge(g, vals, table, sims, I)
    assert lat.all()
    np.testing.assert_allclose(one["I"], I, rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(one["sims"], sims, rtol=1e-9, atol=1e-13)
    np.testing.assert_array_equal(one["count_ge"], count)


@pytest.mark.parametrize("P", [9, 40])
@pytest.mark.parametrize("d", [15, 16, 17, 32, 33, 255, 256])
def test_nibble_source_at_flush_and_accumulator_edges(ctx, reference, X, perms, d, P):
    """The 4-bit source: byte sums of nibbles flushed every 16 neighbours (k_lag_nib: d = 15 / 16 / 17 / 32 / 33 are one
    flush, a full one, one more neighbour, two, two and one), S = S_lo + 16 S_hi up to 65025 in a uint16 (k_nib_fixup), and
    uint32 sums of nibble x S per task that reach 1.92e9 at d = 255 (test_cpu_moran_limits).  At d = 256 the host's bound
    says no: the uint8 source with 16-bit lag runs instead.  Bit-identical to the uint8 and fp64 runs in every case."""
    parts = mi.ring_graph(N, d, 1.0 / d)
    tab = reference(d, parts, P)
    assert mi.nibble_guard(255, d, N) == (d <= 255)
    try:
        out4, path4 = run(ctx, 4, parts, X, perms[:P])
        out8, path8 = run(ctx, 8, parts, X, perms[:P])
        out64, path64 = run(ctx, 64, parts, X, perms[:P])
    finally:
        ctx.set_moran_source_bits(8)
    assert path4 == ((4, 16, 1) if d <= 255 else (8, 16, 2)), path4
    assert path8 == (8, 16, 2) and path64[:2] == (64, 64), (path8, path64)
    assert_is_oracle(out4, tab, f"nibble source d={d} P={P}")
    assert_identical(out4, out8, f"nibble vs uint8 source, d={d} P={P}")
    assert_identical(out4, out64, f"nibble source vs fp64 rows, d={d} P={P}")


def test_lattice_bound_straddled(ctx, oracle):
    """Two uint16-class genes with degree x largest count x total = 3.9984e15 and 4.0018e15, co-loaded with a dozen small
    ones.  The gene below 4.0e15 is a lattice gene: its count includes the identity row's tie and equals the oracle's.  The
    gene above takes the ordinary centred arithmetic: sims and I at the float tolerance, its count under the near-tie rule.
    (The oracle's lattice_genes knows no such bound -- it decides every integer gene on exact int64 sums -- so the table's
    `lattice` flag of that gene is forced False here; the kernel's own count of it is the float comparison.)  Neither
    gene's results depend on whether the other is loaded."""
    n, d, P = 4096, 257, 12
    parts = mi.ring_graph(n, d, 1.0 / d)
    pair = mi.straddling_genes(n, d)
    assert mi.lattice_product(d, pair[:, 0]) < mi.LATTICE_LIMIT < mi.lattice_product(d, pair[:, 1])
    small = np.asarray(synth(n, 12, 3, dtype=np.float64, sparse_x=False)[1]) * 257.0      # integers, some beyond 255
    assert small.max() > 255 and small.max() < 65536
    Xb = np.column_stack([small[:, :6], pair[:, 0], small[:, 6:], pair[:, 1]])              # genes 6 and 13
    lo, hi = 6, 13
    table = mi.identity_first(oracle.perm_table(3, n, P)[0])
    g, vals = mi.as_csr(parts, n), oracle.dense_genes(Xb)
    I, sims = oracle.morans_i_scores(g, vals), oracle.morans_i_sims_gather(g, vals, table)
    count, lat = oracle.morans_count_ge(g, vals, table, sims, I)
    assert lat.all()
    lat = lat.copy(); lat[hi] = False
    count = count.copy(); count[hi] = (sims[:, hi] >= I[hi]).sum()
    try:
        both, path = run(ctx, 8, parts, Xb, table, n)
        assert path[0] == 16 and path[1] == 64, path
        keep_lo, keep_hi = [c for c in range(14) if c != hi], [c for c in range(14) if c != lo]
        only_lo, path_lo = run(ctx, 8, parts, Xb[:, keep_lo], table, n)
        only_hi, path_hi = run(ctx, 8, parts, Xb[:, keep_hi], table, n)
        assert path_lo[0] == 16 and path_hi[0] == 16
    finally:
        ctx.set_moran_source_bits(8)
    np.testing.assert_allclose(both["I"], I, rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(both["sims"], sims, rtol=1e-9, atol=1e-13)
    assert both["count_ge"][lo] == count[lo] and count[lo] >= 1                              # exact, tie included
    assert_counts_match(both["count_ge"], {"lattice": lat, "count_ge": count, "sims": sims, "I": I})
    for alone, cols in ((only_lo, keep_lo), (only_hi, keep_hi)):
        for key in KEYS:
            np.testing.assert_array_equal(alone[key], both[key][..., cols], err_msg=key)


@pytest.mark.parametrize("flaw", ["one weight an ulp off", "last row one edge short"])
def test_graph_classification_of_a_flawed_ring(ctx, oracle, X, perms, flaw):
    """sc_graph_set_csr: a degree-16 ring whose last weight differs by one ulp is not uniform, one whose last row has 15
    edges is not regular -- no lattice, the centred uint16 kernel, against the oracle on that very graph."""
    P = 9
    indptr, indices, data = mi.ring_graph(N, 16, 1.0 / 16)
    if flaw == "one weight an ulp off":
        data = data.copy(); data[-1] = np.nextafter(data[-1], 1.0)
    else:
        indptr = indptr.copy(); indptr[-1] -= 1
        indices, data = indices[:-1], data[:-1]
    parts = (indptr, indices, data)
    g, vals = mi.as_csr(parts, N), oracle.dense_genes(X)
    assert not oracle.lattice_genes(g, vals).any()
    I, sims = oracle.morans_i_scores(g, vals), oracle.morans_i_sims_gather(g, vals, perms[:P])
    count, lat = oracle.morans_count_ge(g, vals, perms[:P], sims, I)
    assert not lat.any()
    try:
        out, path = run(ctx, 8, parts, X, perms[:P])
        sound, path_sound = run(ctx, 8, mi.ring_graph(N, 16, 1.0 / 16), X, perms[:P])
    finally:
        ctx.set_moran_source_bits(8)
    assert path[0] == 16 and path[1] == 64, path
    assert path_sound[:2] == (8, 16), path_sound                     # the ring itself IS a lattice graph
    assert_is_oracle(out, {"I": I, "sims": sims, "count_ge": count, "lattice": lat}, flaw, exact_counts=False)


def test_processing_order_does_not_change_any_output(ctx, X, perms):
    """sc_graph_capture_order keeps the last neighbour search's bin order when its point count equals the graph's rows --
    here a search over UNRELATED points.  The prelude kernels that walk that order (k_lag_nib, k_lag_u8, k_lag_f32rows,
    sc_lag_tiles) must give what they give in the identity order, bit for bit, in every source width."""
    P = 9
    parts = mi.ring_graph(N, 17, 1.0 / 17)
    rng = np.random.default_rng(2)
    lognorm = np.asarray(synth(N, 37, 4, sparse_x=False, normalize=True)[1])
    batches = [("counts, nibble source", 4, X, 4), ("counts, uint8 source", 8, X, 8),
               ("counts, fp64 rows", 64, X, 64), ("log-normalised float32", 8, lognorm, 32),
               ("fp64-only values", 8, X.astype(np.float64) + 1e-9, 64)]
    try:
        for name, bits, Xb, want_bits in batches:
            runs = []
            for order in ("identity", "foreign"):
                if order == "identity":
                    ctx.knn(rng.uniform(0, 100, (N + 1, 2)), 6)
                else:
                    ctx.knn(rng.uniform(0, 100, (N, 2)), 6, fetch=False)
                out, path = run(ctx, bits, parts, Xb, perms[:P])
                assert path[0] == want_bits, (name, order, path)
                runs.append(out)
            assert_identical(runs[0], runs[1], f"{name}: identity order vs a foreign bin order")
    finally:
        ctx.set_moran_source_bits(8)


def _moments_graph(n, seed, integer_weights=True):
    """Random sparse rows: self-loops, empty rows, one-way edges and mutual edges with different weights."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        if i % 5 == 3 and n > 1:
            continue                                               # an empty row
        k = int(rng.integers(1, min(n, 9) + 1))
        c = rng.choice(n, size=k, replace=False)
        if i % 7 == 0:
            c = np.union1d(c, [i])                                 # a self-loop
        rows.append(np.full(c.size, i)); cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    if n > 2:                                                      # mutual edges: i -> i + 1 and back, unequal weights
        ii = np.arange(0, n - 1, 3)
        rows, cols = np.concatenate([rows, ii, ii + 1]), np.concatenate([cols, ii + 1, ii])
    keep = np.unique(rows * n + cols)
    rows, cols = keep // n, keep % n
    w = rng.integers(1, 8, rows.size).astype(np.float64) if integer_weights else rng.uniform(0.1, 2.0, rows.size)
    A = csr_matrix((w, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_graph_moments_at_row_block_edges(ctx, oracle, n):
    """k_moments / k_weight_sum take 1024 rows per block.  Small-integer weights: s0, s1, s2 are exact in any order."""
    A = _moments_graph(n, n)
    if n > 1:
        coo = A.tocoo()
        back = np.asarray(A[coo.col, coo.row]).ravel()            # weight of the reverse edge, 0 where there is none
        off = coo.row != coo.col
        assert (np.diff(A.indptr) == 0).any() and (~off).any()                       # empty rows, self-loops
        assert (off & (back == 0)).any() and (off & (back != 0) & (back != coo.data)).any()   # one-way; mutual, unequal
    ctx.set_graph_csr(A.indptr, A.indices, A.data, n)
    assert ctx.graph_moments() == oracle.graph_moments(A)
    if n > 1:       # s0 alone first (k_weight_sum, the scoring's own sum), the three moments pending beside it, then asked for
        ctx.set_graph_csr(A.indptr, A.indices, A.data, n)
        ctx.set_expression(np.arange(2.0 * n).reshape(n, 2) % 5, np.arange(2))
        ctx.moran(0)
        assert ctx.graph_moments() == oracle.graph_moments(A)


def test_graph_moments_float_weights(ctx, oracle):
    A = _moments_graph(2049, 5, integer_weights=False)
    ctx.set_graph_csr(A.indptr, A.indices, A.data, 2049)
    np.testing.assert_allclose(ctx.graph_moments(), oracle.graph_moments(A), rtol=1e-12)


def test_graph_moments_belong_to_the_active_graph(ctx, oracle):
    """A scoring set-up starts the moments of graph A on the side stream and nobody collects them; a job begun with
    sc_moran_seeded_begin is dropped; then graph B is loaded: sc_graph_moments must answer for B."""
    from spatialcore_amd._lib import rng_state_words

    n = 1025
    A, B = _moments_graph(n, 21), _moments_graph(n, 22)
    assert oracle.graph_moments(A) != oracle.graph_moments(B)
    Xs = np.asarray(synth(n, 5, 6, sparse_x=False)[1])
    ctx.set_graph_csr(A.indptr, A.indices, A.data, n)
    ctx.set_expression(Xs, np.arange(5))
    w = rng_state_words(np.random.default_rng(1))
    ctx.moran_seeded(w, 3)                                         # (its set-up launched A's moments; they are still pending)
    ctx.moran_seeded_begin(w, n, 5)
    ctx.moran_seeded_abort()
    ctx.set_graph_csr(B.indptr, B.indices, B.data, n)
    assert ctx.graph_moments() == oracle.graph_moments(B)
    # ... and with the job begun BEFORE graph A arrives and finished on it, then B
    ctx.moran_seeded_begin(w, n, 5)
    ctx.set_graph_csr(A.indptr, A.indices, A.data, n)
    ctx.moran_seeded_finish(w)
    ctx.set_graph_csr(B.indptr, B.indices, B.data, n)
    assert ctx.graph_moments() == oracle.graph_moments(B)
    ctx.set_graph_csr(A.indptr, A.indices, A.data, n)
    assert ctx.graph_moments() == oracle.graph_moments(A)
