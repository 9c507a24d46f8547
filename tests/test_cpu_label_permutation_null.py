"""CPU: the one driver of the label-permutation nulls (neighborhood_enrichment, ripley_k, ligrec), on fakes."""
import numpy as np
import pytest

from spatialcore_amd.spatial.neighborhoods import _label_permutation_null


class _Ctx:
    def __init__(self):
        self.generated = []

    def generate_permutations(self, words, n, rows):
        assert words.dtype == np.uint64 and words.shape == (6,)
        self.generated.append((n, rows))


class _Comm:
    def __init__(self, world, rank):
        self.world, self.rank, self.reduced = world, rank, []

    def sum_over_ranks_i64(self, sums):
        self.reduced.append(np.array(sums))
        return sums * self.world


def _drive(P, perm_batch, comm=None, rng="numpy"):
    ctx, passes, ranges = _Ctx(), [], []

    def resident(rows):
        passes.append((rows, len(ctx.generated)))       # (rows asked for, batches generated before this pass)
        return f"observed after {len(passes)}", np.array([rows, 1], dtype=np.int64)

    def counter(lo, n):
        ranges.append((lo, n))
        return "observed", np.array([n, 1], dtype=np.int64)

    observed, sums = _label_permutation_null(ctx, 11, P, 5, perm_batch, rng, comm, resident, counter)
    return ctx, passes, ranges, observed, sums


@pytest.mark.parametrize("P,perm_batch,want", [(37, 16, [16, 16, 5]), (32, 16, [16, 16]), (5, 16, [5]), (16, 1, [1] * 16)])
def test_numpy_path_asks_for_min_of_batch_and_rest(P, perm_batch, want):
    ctx, passes, ranges, observed, sums = _drive(P, perm_batch)
    assert ctx.generated == [(11, rows) for rows in want] and not ranges
    assert passes == [(rows, b + 1) for b, rows in enumerate(want)]       # every batch is generated, then counted
    np.testing.assert_array_equal(sums, [P, len(want)])
    assert observed == f"observed after {len(want)}"


def test_no_permutations_is_one_pass_without_generation():
    ctx, passes, ranges, observed, sums = _drive(0, 16)
    assert ctx.generated == [] and passes == [(0, 0)] and observed == "observed after 1"
    np.testing.assert_array_equal(sums, [0, 1])


def test_a_shard_is_counted_from_its_lower_bound_and_reduced_once():
    # ranks 0, 1, 2 of 3 take 13, 12, 12 of 37; the numpy path's batches are min(perm_batch, hi - done) within the shard
    for rank, lo, want in [(0, 0, [5, 5, 3]), (1, 13, [5, 5, 2]), (2, 25, [5, 5, 2])]:
        comm = _Comm(3, rank)
        ctx, passes, _, _, sums = _drive(37, 5, comm)
        assert [rows for _, rows in ctx.generated] == want == [rows for rows, _ in passes]
        assert len(comm.reduced) == 1
        np.testing.assert_array_equal(comm.reduced[0], [sum(want), 3])
        np.testing.assert_array_equal(sums, [3 * sum(want), 9])
        comm = _Comm(3, rank)
        ctx, passes, ranges, observed, sums = _drive(37, 5, comm, rng="philox")
        assert ranges == [(lo, sum(want))] and not passes and not ctx.generated and len(comm.reduced) == 1
    # an empty shard (more ranks than permutations) still runs its one pass and still joins the collective
    comm = _Comm(4, 3)
    ctx, passes, _, _, _ = _drive(2, 5, comm)
    assert ctx.generated == [] and passes == [(0, 0)] and len(comm.reduced) == 1
    # one rank: no collective
    comm = _Comm(1, 0)
    _drive(7, 5, comm)
    assert comm.reduced == []
