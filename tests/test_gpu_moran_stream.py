"""Moran's finalise beside the scoring (a ring of partial-sum slices, the finalise launches on a side stream) and the
consumer's set-up in two callbacks around the generator's top-up (pipe_consume): the smallest shapes at which a ring or
an ordering mistake shows.  n = 5000 cells are 3 splits of the scoring kernels with a ragged last one; G = 130 / 17
are two / one uint8 row groups with a padded last group; P = 1000 is the 11-chunk schedule 32, 40, 128 x 6, 96, 48, 24
(more than three times the ring), P = 400 the 6 chunks 32, 72, 128, 96, 48, 24.

Every pipeline result is compared bit for bit with the two-step path -- the host generator's table uploaded, then
sc_moran -- and the statistics with the oracle's gather form to rtol 1e-9 (the only difference: summation order)."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

from conftest import load_golden

pytestmark = pytest.mark.gpu

N, K = 5000, 6
KEYS = ("sims", "I", "count_ge", "sim_sum", "sim_sumsq")


@pytest.fixture(scope="module")
def ctx():
    from spatialcore_amd import _lib

    c = _lib.default_context(0)
    yield c
    c.set_moran_source_bits(8)
    c.set_permgen_mode(0)


def words(seed):
    from spatialcore_amd._lib import rng_state_words

    return rng_state_words(np.random.default_rng(seed))


def counts_matrix(n, G, seed, wide=()):
    """Integer counts < 16 (lattice genes on a kNN graph: the uint8 source), `wide` genes with values of 16 and more."""
    rng = np.random.default_rng(seed)
    X = np.minimum(rng.poisson(rng.uniform(0.2, 4.0, G), (n, G)), 15).astype(np.float64)
    for g in wide:
        X[:, g] = rng.poisson(14.0, n)
        assert 16 <= X[:, g].max() < 256
    return X


@pytest.fixture(scope="module")
def case(oracle):
    """Coordinates, the kNN graph as CSR (rows of K entries of weight 1 / K), 130 count genes, the host generator's 1000
    permutations from seed 7 and the oracle's statistics of all of them -- computed once, never written to."""
    from spatialcore_amd._lib import perm_numpy_host

    rng = np.random.default_rng(1)
    coords = rng.uniform(0, np.sqrt(N) * 10, (N, 2))
    nbr = np.sort(oracle.knn_tree(coords, K), axis=1)
    g = csr_matrix((np.full(N * K, 1.0 / K), nbr.reshape(-1), np.arange(0, N * K + 1, K)), shape=(N, N))
    X = counts_matrix(N, 130, 2)
    w = words(7)
    table = perm_numpy_host(w, N, 1000)
    vals = oracle.dense_genes(X)
    out = {"coords": coords, "g": g, "X": X, "table": table, "words_after": w, "vals": vals,
           "sims": oracle.morans_i_sims_gather(g, vals, table), "I": oracle.morans_i_scores(g, vals)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def load(c, case, G):
    g = case["g"]
    c.set_graph_csr(g.indptr, g.indices, g.data, N)
    c.set_expression(case["X"][:, :G], np.arange(G))


def two_step(c, case, P):
    c.set_permutations(case["table"][:P])
    return c.moran(P)


def assert_same(got, want, what=""):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what} {key}")


def assert_oracle(out, case, P, G):
    np.testing.assert_allclose(out["I"], case["I"][:G], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(out["sims"], case["sims"][:P, :G], rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("G", [130, 17])
@pytest.mark.parametrize("bits", [8, 16, 32, 64])
def test_ring_wraps_and_reuses_slices_p1000(ctx, case, bits, G):
    """11 scoring launches on 3 slices: every slice is reused at least three times, the tapering last chunks included."""
    P = 1000
    ctx.set_moran_source_bits(bits)
    load(ctx, case, G)
    w = words(7)
    pipe = ctx.moran_seeded(w, P)
    assert ctx.moran_source_bits() == bits
    np.testing.assert_array_equal(w, case["words_after"])
    want = two_step(ctx, case, P)
    assert ctx.moran_source_bits() == bits
    assert_same(pipe, want, f"source {bits}")
    assert_oracle(pipe, case, P, G)


def test_ring_nibble_source_p400(ctx, case, oracle):
    """The 4-bit source (one 256-slot row group for 130 genes, five of them with a high nibble) and its own finalise
    kernel over the 6-chunk schedule."""
    from spatialcore_amd._lib import perm_numpy_host

    P, G = 400, 130
    wide = (3, 40, 77, 128, 129)
    X = counts_matrix(N, G, 5, wide=wide)
    g = case["g"]
    ctx.set_moran_source_bits(4)
    ctx.set_graph_csr(g.indptr, g.indices, g.data, N)
    ctx.set_expression(X, np.arange(G))
    w = words(9)
    pipe = ctx.moran_seeded(w, P)
    assert ctx.moran_source_bits() == 4
    table = perm_numpy_host(words(9), N, P)
    ctx.set_permutations(table)
    want = ctx.moran(P)
    assert ctx.moran_source_bits() == 4
    assert_same(pipe, want, "source 4")
    vals = oracle.dense_genes(X)
    np.testing.assert_allclose(pipe["I"], oracle.morans_i_scores(g, vals), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(pipe["sims"], oracle.morans_i_sims_gather(g, vals, table), rtol=1e-9, atol=1e-13)


def test_resident_table_path(ctx, case, oracle):
    """sc_moran on an uploaded table: P = 300 is the chunks 128, 128, 44 (one turn of the ring), P = 600 five launches on
    the same context; then index rows that are no permutations (k_moran_perm / k_moran_finalize: one launch pair per
    16-gene tile and chunk, 6 for 17 genes at P = 300)."""
    G = 130
    ctx.set_moran_source_bits(8)
    load(ctx, case, G)
    ctx.set_permutations(case["table"][:600])
    a = ctx.moran(300)
    b = ctx.moran(600)
    assert ctx.moran_source_bits() == 8
    assert_oracle(a, case, 300, G)
    assert_oracle(b, case, 600, G)
    np.testing.assert_array_equal(a["sims"], b["sims"][:300])
    np.testing.assert_array_equal(a["I"], b["I"])
    pipe = ctx.moran_seeded(words(7), 600)
    np.testing.assert_array_equal(b["sims"], pipe["sims"])      # (chunked 32, 56, 128 x 2, 96, 48, 24 there)
    np.testing.assert_array_equal(b["count_ge"], pipe["count_ge"])
    G = 17
    idx = np.random.default_rng(3).integers(0, N, (300, N)).astype(np.int32)
    load(ctx, case, G)
    ctx.set_permutations(idx)
    free = ctx.moran(300)
    assert ctx.moran_source_bits() == 64
    want = oracle.morans_i_sims_gather(case["g"], case["vals"][:G], idx)
    np.testing.assert_allclose(free["I"], case["I"][:G], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(free["sims"], want, rtol=1e-9, atol=1e-13)
    np.testing.assert_array_equal(free["count_ge"], (free["sims"] >= free["I"]).sum(axis=0))


def test_state_across_jobs_on_one_context(ctx, case):
    """The ring's counter, events and slice size belong to one job: a shrinking slice (G 130 -> 17), a single-chunk job
    and a job begun and aborted leave nothing behind -- each result is that of a context that ran nothing before."""
    from spatialcore_amd._lib import Context

    ctx.set_moran_source_bits(8)

    def job(c, G, P, seed):
        load(c, case, G)
        return c.moran_seeded(words(seed), P)

    def fresh(G, P, seed):
        with Context(0) as f:
            return job(f, G, P, seed)

    got = [job(ctx, 130, 1000, 7), job(ctx, 17, 1000, 7), job(ctx, 17, 40, 8)]
    load(ctx, case, 130)
    w = words(11)
    ctx.moran_seeded_begin(w, N, 1000, ahead_chunks=2)
    ctx.moran_seeded_abort()
    np.testing.assert_array_equal(w, words(11))
    got.append(job(ctx, 130, 400, 12))
    want = [fresh(130, 1000, 7), fresh(17, 1000, 7), fresh(17, 40, 8), fresh(130, 400, 12)]
    for i, (a, b) in enumerate(zip(got, want)):
        assert_same(a, b, f"job {i}")
    assert_oracle(got[0], case, 1000, 130)
    assert_oracle(got[1], case, 1000, 17)


@pytest.fixture(scope="module")
def big(ctx):
    """n = 131072 + 37 cells (the block-parallel generator), 130 count genes, P = 400 through the one-call form."""
    n, G, P = 131072 + 37, 130, 400
    rng = np.random.default_rng(4)
    coords = rng.uniform(0, np.sqrt(n) * 10, (n, 2))
    X = counts_matrix(n, G, 6).astype(np.float32)
    ctx.set_moran_source_bits(8)
    ctx.knn(coords, K, fetch=False)
    ctx.graph_from_knn(1.0 / K)
    ctx.set_expression(X, np.arange(G))
    w = words(21)
    one = ctx.moran_seeded(w, P)
    assert ctx.permgen_form(n) == "block-parallel"
    return {"n": n, "P": P, "one": one, "words_after": w}


@pytest.mark.parametrize("ahead", [2, 3, 0])
def test_two_phase_setup_beside_block_parallel_generator(ctx, big, ahead):
    """begin / finish with every lookahead begin can leave (2, 3, all chunks): the first half of the set-up is enqueued,
    the generator topped up, the rest of the set-up waits -- results and generator state of the one-call form, and the
    block-parallel scan passed its verification."""
    n, P = big["n"], big["P"]
    stats = ctx.permgen_stats()
    w = words(21)
    ctx.moran_seeded_begin(w, n, P, ahead_chunks=ahead)
    two = ctx.moran_seeded_finish(w)
    np.testing.assert_array_equal(w, big["words_after"])
    assert_same(two, big["one"], f"ahead_chunks {ahead}")
    after = ctx.permgen_stats()
    assert after[0] == stats[0] + 1       # one more block-parallel job
    assert after[1] == stats[1] and after[2] == stats[2]       # no sequential job, no fallback


def test_consumers_without_a_split_setup(ctx):
    """sc_lee_seeded (no set-up in the pipeline) and sc_local_moran_seeded (its whole set-up as the second callback)
    against their two-step paths, at the shapes of their own tests."""
    g = load_golden("ref_lees_l.npz")
    coords, X = g["c0_coords"], g["c0_X"]
    k, P, seed = int(g["c0_k"]), int(g["c0_P"]), int(g["c0_seed"])
    pairs = g["c0_pairs"]
    n = X.shape[0]
    ctx.knn(coords, k, fetch=False)
    ctx.graph_from_knn(float(np.float32(1.0) / np.float32(k)))
    ctx.set_expression(X, np.arange(X.shape[1]))
    _, var = ctx.expr_stats()
    live = np.array([var[a] > 0 and var[b] > 0 for a, b in pairs])
    assert P > 0 and live.any()
    w = words(seed)
    out = ctx.lee_seeded(w, pairs[:, 0], pairs[:, 1], P, return_perms=True)
    w2 = words(seed)
    off = np.where(live, np.cumsum(live) - 1, -1) * P
    off[~live] = -1
    ctx.generate_permutations(w2, n, int(live.sum()) * P)
    np.testing.assert_array_equal(w, w2)
    ref = ctx.lee(pairs[:, 0], pairs[:, 1], off, P, return_perms=True)
    np.testing.assert_allclose(out["L"], ref["L"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out["L_perm"], ref["L_perm"], rtol=1e-9, atol=1e-10)     # (summation order differs)
    np.testing.assert_array_equal(out["count_abs_ge"][live], ref["count_abs_ge"][live])

    n, P, G = 3000, 41, 21
    rng = np.random.default_rng(n + P)
    coords = rng.uniform(0, np.sqrt(n) * 10, (n, 2))
    X = rng.poisson(rng.uniform(0.1, 3.0, G), (n, G)).astype(np.float32)
    ctx.knn(coords, K, fetch=False)
    ctx.graph_from_knn(1.0 / K)
    ctx.set_expression(X, np.arange(G))
    w1 = words(77)
    ctx.generate_permutations(w1, n, P)
    want = ctx.local_moran(n, P)
    w2 = words(77)
    got = ctx.local_moran_seeded(w2, n, P)
    np.testing.assert_array_equal(w1, w2)
    for f in ("z", "lag", "I", "count"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
