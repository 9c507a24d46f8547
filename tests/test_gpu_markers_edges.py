"""GPU tests of sc_ranksum at the edges of its kernels: several table rounds of k_rs_runs in one chunk (up to the 4096
groups of the envelope, with empty genes inside a chunk and genes across chunk seams), pieces of exactly 255 / 256 / 257 /
512 / 513 cells and empty groups between occupied ones, one sort batch whose genes differ in value class, and the ends
of the ordered-bits keys (neighbouring representable values, denormals, signed zeros, the largest finite values).  The
second sort batch (more than 2^27 pairs) is in tests/test_gpu_fullsize.py.

The reference is tests/wilcoxon_restated.py (integer_tables, or integer_tables_bincount where there are thousands of
groups; tests/test_cpu_markers.py holds them equal).  Integer outputs are compared with ==, the value sums by the policy
of tests/test_gpu_markers.py.  The inputs come from tests/test_cpu_markers.py, which asserts without a device that each
of them reaches the edge it is about."""
import math

import numpy as np
import pytest
from scipy import sparse
from scipy.stats import rankdata

from test_cpu_markers import (PIECE_SIZES, ROUNDS_CASES, mixed_class_input, piece_input, rounds_input, rounds_codes)
from test_gpu_markers import INT_KEYS, _assert_tables, _ranksum
from wilcoxon_restated import integer_tables, integer_tables_bincount

pytestmark = pytest.mark.gpu

BYTE_KEYS = ("rank2", "nnz", "n_neg", "sums")


def _assert_gene_bytes(got, g, alone, label=""):
    """Gene g of a call == gene 0 of the call that loaded it alone, byte for byte."""
    for k in BYTE_KEYS:
        assert got[k][g].tobytes() == alone[k][0].tobytes(), (label, g, k)
    assert int(got["tie_nonzero"][g]) == int(alone["tie_nonzero"][0]), (label, g)


# ---- 1. table rounds of k_rs_runs ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_groups, also_zero", ROUNDS_CASES,
                         ids=[f"{k}" + "".join(f"-gene{g}-empty" for g in z) for k, z in ROUNDS_CASES])
def test_table_rounds(n_groups, also_zero):
    """A chunk of 2048 pairs that spans more genes than the LDS table holds (4096 // n_groups) is added in several
    rounds: 2 / 2 / 1 rounds in the three chunks at 300 groups, 18 / 18 / 7 at 4096 (tests/test_cpu_markers.py restates
    the walk).  float32: the one-pass sort; the same matrix * 0.1 as float64: the two-pass sort.  At 4096 groups about
    half of the groups are empty: gpiece[g] == gpiece[g + 1] in k_rs_final."""
    X, code = rounds_input(also_zero), rounds_codes(n_groups)
    if n_groups == 4096:
        assert (np.bincount(code, minlength=n_groups) == 0).sum() > 1000
    _assert_tables(_ranksum(X, code, n_groups), integer_tables_bincount(X, code, n_groups), "float32", sums="exact")
    X64 = X.astype(np.float64) * 0.1
    assert (X64.astype(np.float32).astype(np.float64) != X64).any()
    _assert_tables(_ranksum(X64, code, n_groups), integer_tables_bincount(X64, code, n_groups), "fp64", sums="rtol")


@pytest.mark.parametrize("form", ["float32", "fp64"])
def test_a_gene_of_many_rounds_equals_the_gene_loaded_alone(form):
    """4096 groups: one gene per round, 18 / 18 / 7 rounds in the three chunks.  Loaded alone a gene has a chunk span of
    one gene and a single round."""
    X, code = rounds_input(), rounds_codes(4096)
    if form == "fp64":
        X = X.astype(np.float64) * 0.1
    got = _ranksum(X, code, 4096)
    for g in range(X.shape[1]):
        _assert_gene_bytes(got, g, _ranksum(X[:, [g]], code, 4096), form)


# ---- 2. pieces ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "csr"])
def test_piece_edges_and_empty_groups(form):
    """Groups of 0, 1, 255, 256, 257, 0, 512, 513 and 2 cells (pieces of 256 cells: full ones, a last piece of one cell,
    gpiece[g] == gpiece[g + 1] for the empty groups) and 300 excluded cells, shuffled and with contiguous groups."""
    got = []
    for X, code in piece_input():
        want = integer_tables(X, code, 9)
        out = _ranksum(sparse.csr_matrix(X) if form == "csr" else X, code, 9)
        _assert_tables(out, want, form, sums="exact")                 # raw counts: exact in any order
        assert out["group_n"].tolist() == PIECE_SIZES
        for k in ("rank2", "nnz", "sums"):
            assert not out[k][:, [0, 5]].any(), k
            assert out[k][:, [1, 2, 3, 4, 6, 7, 8]].any(axis=0).all(), k
        got.append(out)
    for k in INT_KEYS + ("sums",):                                    # integer-valued data: the sums are == as well
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)
    assert got[0]["tie_nonzero"].tolist() == got[1]["tie_nonzero"].tolist()


# ---- 3. value classes mixed inside one batch -------------------------------------------------------------------------------

def test_one_batch_of_mixed_value_classes():
    """33 genes in one batch; genes 20 and 32 are not float32-exact, so all 33 take the two-pass fp64 sort (payload
    gene << 12 | group).  Loaded alone, the 31 count genes take the one-pass float32 sort: the same bytes either way."""
    X = mixed_class_input()
    assert X.dtype == np.float64
    code = np.random.default_rng(52).choice(5, X.shape[0], p=[0.4, 0.3, 0.15, 0.1, 0.05]).astype(np.int32)
    got, want = _ranksum(X, code, 5), integer_tables(X, code, 5)
    counts = [g for g in range(33) if g not in (20, 32)]
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert [int(t) for t in got["tie_nonzero"]] == [int(t) for t in want["tie_nonzero"]]
    np.testing.assert_array_equal(got["sums"][counts], want["sums"][counts])          # integer-valued
    eps = np.finfo(np.float64).eps
    for g in (20, 32):                                                                # both signs: n_k eps sum |x|
        for k in range(5):
            x = X[code == k, g]
            assert abs(got["sums"][g, k] - math.fsum(x)) <= x.size * eps * math.fsum(np.abs(x)), (g, k)
    for g in range(33):
        _assert_gene_bytes(got, g, _ranksum(X[:, [g]], code, 5))


# ---- 4. key edges -----------------------------------------------------------------------------------------------------------

N_EDGE = 1500


def _edge_code():
    return np.random.default_rng(61).choice(3, N_EDGE, p=[0.5, 0.3, 0.2]).astype(np.int32)


def _ordinary(seed, dtype, signed):
    """One column of ordinary values with ties (counts 1, 2, 3 ..., negated at random if ``signed``) and ~55 % zeros."""
    rng = np.random.default_rng(seed)
    x = np.where(rng.uniform(size=N_EDGE) < 0.45, rng.poisson(1.0, N_EDGE) + 1.0, 0.0)
    if signed:
        x *= rng.choice([-1.0, 1.0], N_EDGE)
    return x.astype(dtype)


def _plant(x, values, seed, copies=7):
    """``copies`` cells of every value, at random places (a tie run of each, spread over the groups)."""
    at = np.random.default_rng(seed).choice(x.size, copies * len(values), replace=False)
    x = x.copy()
    for j, v in enumerate(values):
        x[at[j * copies:(j + 1) * copies]] = v
    return x


def _check_edges(X, code, no_sums=()):
    """One call against integer_tables; sums by the n_k * eps * sum |x| bound against math.fsum (both signs in a gene)."""
    with np.errstate(over="ignore", invalid="ignore"):
        want = integer_tables(X, code, 3)
    got = _ranksum(X, code, 3)
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert [int(t) for t in got["tie_nonzero"]] == [int(t) for t in want["tie_nonzero"]]
    D = (np.asarray(X.todense()) if sparse.issparse(X) else X).astype(np.float64)
    eps = np.finfo(np.float64).eps
    for g in range(D.shape[1]):
        for k in range(3):
            x = D[code == k, g]
            if g not in no_sums:
                assert abs(got["sums"][g, k] - math.fsum(x)) <= x.size * eps * math.fsum(np.abs(x)), (g, k)
    return got, want


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_neighbouring_float32_values(dtype):
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    assert up > one and np.float32(up - one) == np.float32(2.0 ** -23)
    X = np.stack([_plant(_ordinary(1, np.float32, False), [one, up], 2),
                  _plant(_ordinary(3, np.float32, True), [-one, -up], 4),
                  _plant(_ordinary(5, np.float32, True), [one, up, -one, -up], 6)], axis=1).astype(dtype)
    got, want = _check_edges(X, _edge_code())
    # the planted neighbour of 1.0 is a tie run of its own (7 cells) next to the many 1.0 of the ordinary values
    for g in range(3):
        vals, counts = np.unique(X[:, g], return_counts=True)
        assert (counts[np.isin(vals, [up, -up])] == 7).all() and np.isin(vals, [up, -up]).sum() == (1, 1, 2)[g]
        assert (counts[np.isin(vals, [one, -one])] > 7).all()


def test_float64_values_closer_than_float32_precision():
    """1.0, 1.0 + 2^-40 and nextafter(1.0, 2): one float32, three float64 values -> three ranks, and the gene must be
    classed as not float32-exact (as float32 the three would be one tie run)."""
    vals = [1.0, 1.0 + 2.0 ** -40, np.nextafter(1.0, 2.0)]
    assert len({np.float32(v) for v in vals}) == 1 and len(set(vals)) == 3
    X = np.stack([_plant(_ordinary(7, np.float64, False), vals, 8),
                  _plant(_ordinary(9, np.float64, True), [-v for v in vals], 10),
                  _ordinary(11, np.float64, False)], axis=1)                          # a float32-exact gene beside them
    code = _edge_code()
    got, want = _check_edges(X, code)
    as32 = integer_tables(X.astype(np.float32), code, 3)
    for g in (0, 1):                                                                  # the float32 image ties them
        assert int(want["tie_nonzero"][g]) != int(as32["tie_nonzero"][g]) and (want["rank2"][g] != as32["rank2"][g]).any()
        r2 = 2.0 * rankdata(X[:, g])
        sign = 1.0 if g == 0 else -1.0
        assert len({r2[X[:, g] == sign * v][0] for v in vals}) == 3


@pytest.mark.parametrize("kind", ["float32", "float32 as float64", "float64"])
def test_denormals(kind):
    """Denormals are non-zero, distinct, and ranked on their side of the zero block."""
    if kind == "float64":
        small = [5e-324, 1e-310]
        assert all(0.0 < v < np.finfo(np.float64).tiny for v in small)
        dtype = np.float64
    else:
        small = [np.float32(1e-40), np.float32(2e-40)]
        assert all(np.float32(0.0) < v < np.finfo(np.float32).tiny for v in small) and small[0] != small[1]
        dtype = np.float32
    X = np.stack([_plant(_ordinary(12, dtype, False), small, 13),
                  _plant(_ordinary(14, dtype, True), [-v for v in small], 15),
                  _plant(_ordinary(16, dtype, True), small + [-v for v in small], 17)], axis=1)
    assert X.dtype == dtype
    if kind == "float32 as float64":
        X = X.astype(np.float64)
    code = _edge_code()
    plain = np.stack([_ordinary(12, dtype, False), _ordinary(14, dtype, True), _ordinary(16, dtype, True)], axis=1)
    got, want = _check_edges(X, code)
    # 14 / 14 / 28 planted cells count as non-zero (some replace an ordinary non-zero: compare with the exact count)
    np.testing.assert_array_equal(got["nnz"].sum(axis=1), (X != 0).sum(axis=0))
    assert ((X != 0).sum(axis=0) > (plain != 0).sum(axis=0)).all()
    np.testing.assert_array_equal(got["n_neg"], (X < 0).sum(axis=0))
    assert got["n_neg"][0] == 0 and got["n_neg"][1] >= 14


@pytest.mark.parametrize("form", ["dense float32", "dense float64", "csr float32", "csr float64"])
def test_signed_zeros(form):
    """-0.0 and 0.0 both belong to the zero block, dense and as explicitly stored CSR entries."""
    dtype = np.float32 if form.endswith("32") else np.float64
    X = np.stack([_plant(_ordinary(18, dtype, False), [-0.0, 0.0], 19, copies=40),
                  _plant(_ordinary(20, dtype, True), [-0.0, 0.0], 21, copies=40)], axis=1)
    assert X.dtype == dtype and (np.signbit(X) & (X == 0)).sum(axis=0).min() >= 40
    code = _edge_code()
    if form.startswith("csr"):
        stored = (X != 0) | (np.random.default_rng(22).uniform(size=X.shape) < 0.2) | np.signbit(X)
        rows, cols = np.nonzero(stored)
        indptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))])
        A = sparse.csr_matrix((X[rows, cols], cols, indptr), shape=X.shape)
        assert A.has_canonical_format and A.nnz > (X != 0).sum() + 80 and np.signbit(A.data[A.data == 0]).any()
        assert not np.signbit(A.data[A.data == 0]).all()
        got, want = _check_edges(A, code)
    else:
        got, want = _check_edges(X, code)
    np.testing.assert_array_equal(got["nnz"].sum(axis=1), (X != 0).sum(axis=0))
    np.testing.assert_array_equal(got["n_neg"], (X < 0).sum(axis=0))


@pytest.mark.parametrize("kind", ["float32", "float32 as float64", "float64"])
def test_largest_finite_values(kind):
    """+-max are accepted (k_rs_count refuses only what is not finite) and ranked first and last.  ``sums`` is not compared
    for the columns that hold +-DBL_MAX: two of them overflow in one order of addition and cancel in another."""
    dtype = np.float64 if kind == "float64" else np.float32
    big = np.finfo(dtype).max
    X = np.stack([_plant(_ordinary(23, dtype, True), [big, -big], 24, copies=1),
                  _plant(_ordinary(25, dtype, True), [big, -big], 26, copies=5),
                  _plant(_ordinary(27, dtype, False), [big], 28, copies=2)], axis=1)
    assert X.dtype == dtype and np.isfinite(X).all()
    if kind == "float32 as float64":
        X = X.astype(np.float64)
    code = _edge_code()
    got, want = _check_edges(X, code, no_sums=(0, 1, 2) if kind == "float64" else ())
    # column 0: one cell each.  The smallest has rank 1; the largest has rank N: read off its group's rank sum
    N = N_EDGE
    r2 = np.rint(2.0 * rankdata(X[:, 0].astype(np.float64))).astype(np.int64)
    lo, hi = int(np.argmin(X[:, 0])), int(np.argmax(X[:, 0]))
    assert r2[lo] == 2 and r2[hi] == 2 * N
    for cell in (lo, hi):                                  # the group's rank sum without that cell = the other cells' ranks
        k = code[cell]
        others = (code == k) & (np.arange(N) != cell)
        assert got["rank2"][0, k] - r2[cell] == r2[others].sum()
