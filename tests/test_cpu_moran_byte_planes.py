"""The arithmetic of the byte-plane scoring kernel, restated in numpy (no GPU).

k_moran_score_wg<8, 4, false, true> (sc_moran.hip) scores an all-lattice uint8 batch on 16-bit neighbour sums in
integers: S = lo + 256 hi, and per task (gene group, cell split, 128 permutations) it keeps one uint32 sum per gene and
plane, fed by 8-bit dot products over blocks of four cells (v_dot4_u32_u8) for the split's whole 16-cell super-blocks and
by single products for its ragged tail; the task's result is (double)lo_sum + 256.0 * (double)hi_sum.  Restated here with
numpy's wrapping uint32 arithmetic and compared with the int64 sum of S x per split and permutation; the bound that keeps
a plane sum below 2^32 is asserted for the largest n the kernel serves."""
import numpy as np
import pytest

import moran_limits_inputs as mi

N, G = mi.N_CELLS, mi.N_GENES
SUPER_BLOCK = 16        # SCORE_SB
BLOCK = 4               # CB: cells of one dot product


def udot4(a, b, acc):
    """v_dot4_u32_u8 without clamp: acc + sum of the four byte products, in wrapping uint32.  a, b: (..., 4) uint8."""
    prod = a.astype(np.uint32) * b.astype(np.uint32)
    with np.errstate(over="ignore"):
        return (acc + prod.sum(axis=-1, dtype=np.uint32)).astype(np.uint32)


def byte_plane_partials(S, X, inv):
    """partial[split][perm][gene] as the kernel leaves it: S (n, G) integer neighbour sums <= 65535, X (n, G) counts <= 255,
    inv (P, n) inverse permutation rows (cell j of permutation p multiplies S[j] with X[inv[p, j]])."""
    n, genes = S.shape
    assert S.max() <= 65535 and X.max() <= 255
    lo, hi = (S & 0xff).astype(np.uint8), (S >> 8).astype(np.uint8)
    x8 = X.astype(np.uint8)
    cps = mi.score_cells_per_split(n)
    out = []
    for c0 in range(0, n, cps):
        c1 = min(c0 + cps, n)
        whole = (c1 - c0) // SUPER_BLOCK * SUPER_BLOCK
        rows = []
        for p in range(inv.shape[0]):
            slo = np.zeros(genes, dtype=np.uint32)
            shi = np.zeros(genes, dtype=np.uint32)
            for b0 in range(c0, c0 + whole, BLOCK):              # one pipeline block: four cells, a word per gene and operand
                xs = x8[inv[p, b0:b0 + BLOCK]].T                 # (genes, 4): the transposed gathered bytes
                slo = udot4(xs, lo[b0:b0 + BLOCK].T, slo)
                shi = udot4(xs, hi[b0:b0 + BLOCK].T, shi)
            with np.errstate(over="ignore"):
                for j in range(c0 + whole, c1):                  # the ragged tail: plain uint32 products
                    xj = x8[inv[p, j]].astype(np.uint32)
                    slo = (slo + xj * lo[j].astype(np.uint32)).astype(np.uint32)
                    shi = (shi + xj * hi[j].astype(np.uint32)).astype(np.uint32)
            rows.append(slo.astype(np.float64) + 256.0 * shi.astype(np.float64))
        out.append(rows)
    return np.array(out)


def int64_partials(S, X, inv):
    n = S.shape[0]
    cps = mi.score_cells_per_split(n)
    return np.array([[(S[c0:c0 + cps].astype(np.int64) * X[inv[p, c0:c0 + cps]].astype(np.int64)).sum(axis=0)
                      for p in range(inv.shape[0])] for c0 in range(0, n, cps)])


@pytest.fixture(scope="module")
def counts():
    return mi.saturating_counts(N, G, 1).astype(np.int64)


@pytest.fixture(scope="module")
def inverse_rows():
    rng = np.random.default_rng(5)
    return np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(3)])


@pytest.mark.parametrize("d", [1, 16, 255, 256, 257])
def test_plane_sums_recombine_to_the_int64_sums(counts, inverse_rows, d):
    """Rings of degree 1 .. 257 under saturating counts: hi is 0 throughout (d = 1), S crosses 255 -> 256, and reaches
    65535 with both planes 255 (d = 257).  Two splits, 2048 cells and 262 = 16 super-blocks + a tail of 6."""
    S = np.asarray(mi.adjacency(mi.ring_graph(N, d, 1.0 / d), N) @ counts).astype(np.int64)
    assert S.max() == 255 * d and ((S >> 8).max() > 0) == (d > 1)
    got, want = byte_plane_partials(S, counts, inverse_rows), int64_partials(S, counts, inverse_rows)
    assert got.shape == want.shape == (2, inverse_rows.shape[0], G)
    assert want.max() < 2 ** 53
    np.testing.assert_array_equal(got, want.astype(np.float64))
    assert (got.astype(np.int64) == want).all()


def test_tail_only_and_single_super_block_splits():
    """n = 2049: the second split is one cell, all tail; n = 2064: exactly one super-block, no tail."""
    for n in (2049, 2064):
        X = mi.saturating_counts(n, 6, 2).astype(np.int64)
        S = np.asarray(mi.adjacency(mi.ring_graph(n, 257, 1.0), n) @ X).astype(np.int64)
        inv = np.stack([np.arange(n), np.random.default_rng(n).permutation(n)])
        np.testing.assert_array_equal(byte_plane_partials(S, X, inv), int64_partials(S, X, inv).astype(np.float64))


def test_a_plane_sum_cannot_overflow_uint32():
    """The non-BIG form serves n < 2^25: a task has at most 65536 cells, a plane sum at most 65536 x 255 x 255 < 2^32, and
    the recombined task sum stays an exact double."""
    n_max = (1 << 25) - 1
    assert mi.score_cells_per_split(n_max) == 65536
    for n in (1, 2310, 1 << 20, (1 << 20) + 1, 1 << 24, n_max - 1, n_max):
        cps = mi.score_cells_per_split(n)
        assert cps <= 65536 and cps * 255 * 255 < 2 ** 32
        assert cps * 65535 * 255 < 2 ** 53
    assert 65536 * 255 * 255 == 4_261_478_400
    assert mi.score_cells_per_split(1 << 25) == 65536 and mi.score_cells_per_split((1 << 25) + 4096) > 65536   # from there: BIG
