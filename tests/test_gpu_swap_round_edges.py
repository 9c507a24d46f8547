"""The workgroup form of the Fisher-Yates swaps (k_apply_swaps_wg, sc_swaps.hip) at the edges of its round schedule.

A round is the longest prefix of 512 consecutive steps that touch pairwise distinct slots, decided from the partners in the
kernel's LDS ring.  What can go wrong in any change to that loop is a round's length applied to the wrong steps, a partner
read from a ring slot that is not filled yet (or already overwritten), and the last rounds of a permutation, which are
shorter than a workgroup; with two permutations per workgroup, a half that has no permutation or has finished.  All of it
shows in the table: the forward table (the shuffle itself) comes through generate_permutations, the inverse table (the same
transpositions in ascending order) through moran_seeded, which gathers through nothing else from 65536 cells on."""
import numpy as np
import pytest

from conftest import synth

pytestmark = pytest.mark.gpu

G, K = 16, 6


@pytest.fixture(scope="module")
def ctx():
    from spatialcore_amd import _lib

    with _lib.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def tables(oracle):
    """The oracle's table and final generator state per (n, P): computed once, shared, never written."""
    cache = {}

    def get(n, P):
        if (n, P) not in cache:
            t, w = oracle.perm_table(17, n, P)
            t.setflags(write=False)
            w.setflags(write=False)
            cache[(n, P)] = (t, w)
        return cache[(n, P)]

    return get


def _words():
    from spatialcore_amd._lib import rng_state_words

    return rng_state_words(np.random.default_rng(17))


CASES = [(65536, 3), (65537, 3), (70001, 1), (70001, 2), (70001, 3), (70001, 4)]   # 65536: the first length of the workgroup form


@pytest.mark.parametrize("pw", [1, 2])
@pytest.mark.parametrize("n,P", CASES)
def test_forward_table(ctx, tables, monkeypatch, n, P, pw):
    monkeypatch.setenv("SC_SWAP_PW", str(pw))
    want, wwords = tables(n, P)
    words = _words()
    got = ctx.generate_permutations(words, n, P, fetch=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(words, wwords)


@pytest.mark.parametrize("n", [65536, 65537, 70001])
def test_inverse_table_through_the_scoring(ctx, tables, monkeypatch, n):
    """moran_seeded on the inverse rows the kernel builds == moran on the oracle's uploaded table, bit for bit."""
    coords, X = synth(n, G, 23, dtype=np.float32, sparse_x=False)
    ctx.knn(coords, K, fetch=False)
    ctx.graph_from_knn(1.0 / K)
    ctx.set_expression(X, np.arange(G))
    for P in sorted({p for m, p in CASES if m == n}):
        want, wwords = tables(n, P)
        ctx.set_permutations(want)
        two_step = ctx.moran(P)
        for pw in (1, 2):
            monkeypatch.setenv("SC_SWAP_PW", str(pw))
            words = _words()
            one = ctx.moran_seeded(words, P)
            np.testing.assert_array_equal(words, wwords, err_msg=f"P {P} pw {pw}")
            for key in ("I", "sims", "count_ge", "sim_sum", "sim_sumsq"):
                np.testing.assert_array_equal(one[key], two_step[key], err_msg=f"{key} P {P} pw {pw}")
