"""The expansion of the rejection scan's accept masks into J (k_expand, sc_permgen.hip) at its edges.

One workgroup expands one scan block of 16384 draws: every scan thread puts its accepted, masked draws into an LDS staging
buffer at the count the scan left for it, and the workgroup writes the block's run of J as 16-byte stores with the head and
the tail peeled to alignment.  A wrong staging offset, a wrong peel or a run cut at the wrong place shows in the permutation
table and nowhere else, so every case compares the whole table and the generator state left behind with the oracle's scalar
model of numpy's stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from spatialcore_amd import _lib

    with _lib.Context(0) as c:
        yield c


def _check(ctx, oracle, seed_or_words, n, P):
    from spatialcore_amd._lib import rng_state_words

    if isinstance(seed_or_words, int):
        words = rng_state_words(np.random.default_rng(seed_or_words))
    else:
        words = np.array(seed_or_words, dtype=np.uint64)
    want, wwords = oracle.perm_table(words, n, P)
    got = ctx.generate_permutations(words, n, P, fetch=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(words, wwords)
    return words


@pytest.mark.parametrize("seed,n,P", [
    (3, 2, 40), (4, 3, 40),             # many permutations inside one scan block: i wraps and the mask resets inside a thread's 16 draws
    (7, 1000, 64),                      # permutations end inside blocks: staging offsets cross permutation boundaries
    (5, 4098, 5), (6, 65538, 5),        # just above a power of two: about half the draws rejected, threads with no accepts
    (8, 16385, 3), (9, 16386, 3),       # a permutation of about one block: head and tail alignment of the contiguous run
])
def test_expansion_runs_against_numpy(ctx, oracle, seed, n, P):
    _check(ctx, oracle, seed, n, P)


def test_expansion_over_several_pipeline_chunks(ctx, oracle):
    """P = 300 is three chunks of permutations: one {first block, end block} pair each, and a chunk's last block runs into
    the next chunk's first permutations."""
    _check(ctx, oracle, 10, 4099, 300)


@pytest.mark.parametrize("mode", [0, 1])
def test_both_scan_forms_feed_the_same_expansion(ctx, oracle, mode):
    """n >= 131072: mode 0 is the block-parallel chain, mode 1 the sequential scan; n = 131077 is just above a power of two."""
    try:
        ctx.set_permgen_mode(mode)
        before = ctx.permgen_stats()
        _check(ctx, oracle, 12, 131077, 5)
        par, seq, fallbacks = (a - b for a, b in zip(ctx.permgen_stats()[:3], before[:3]))
        assert (par, seq, fallbacks) == ((1, 0, 0) if mode == 0 else (0, 1, 0)), ctx.permgen_note()
    finally:
        ctx.set_permgen_mode(0)


@pytest.mark.parametrize("seed,n,P,accepted", [(0, 1000, 7, True), (5, 16385, 2, True), (1, 16385, 2, False)])
def test_second_call_starts_with_a_buffered_half_word(ctx, oracle, seed, n, P, accepted):
    """The first call consumes an odd number of 32-bit draws, so the second starts with the buffered high half of a 64-bit
    output.  The host takes that draw: when the first Fisher-Yates step accepts it, it is J[0], written from the host, and
    block 0's run starts at J[1] (every 16-byte group of the run is shifted by one word); when it is rejected, nothing is."""
    words = _check(ctx, oracle, seed, n, P)
    M = n - 1
    mask = (1 << M.bit_length()) - 1
    assert int(words[4]) == 1 and ((int(words[5]) & mask) <= M) == accepted      # (of the case, not of the code under test)
    _check(ctx, oracle, words, n, 5)
