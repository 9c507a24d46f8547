"""Inputs that drive the global Moran prelude to the edge of its integer formats (plain numpy, no GPU).

The host chooses the prelude and scoring kernels from three facts of the batch and the graph (moran_prepare in
sc_moran.hip), each of which keeps an integer from overflowing:

  degree <= 257                     255 x 257 = 65535: the last neighbour sum of uint8 counts that fits the packed 16-bit
                                    halves of k_lag_u8 without a carry into the neighbouring gene's half
  15 xmax d cells_per_split < 2e9   the uint32 sums of nibble x S per task of the 4-bit source
  d xmax[g] xsum[g] < 4.0e15        every partial sum of a lattice gene's T_p stays an exact integer in fp64

The graphs are circulant rings: regular, one weight, any degree, no neighbour search needed.  The guard expressions are
restated here so that the CPU tests can say on which side an input lies; tests/test_cpu_moran_limits.py proves each
input is what tests/test_gpu_moran_limits.py says it is."""
import numpy as np
from scipy.sparse import csr_matrix

N_CELLS = 2310          # two score splits: 2048 cells, then 262 = 16 super-blocks of 16 + a tail of 6
N_GENES = 130           # a second 128-gene group with 2 genes
LATTICE_LIMIT = 4.0e15  # moran_prepare: degree x largest count x sum of counts below this -> lattice gene
NIBBLE_LIMIT = 2.0e9    # moran_prepare: 15 x largest count x degree x cells of a split below this -> nibble source allowed
STRADDLE_TOTALS = (237_400_000, 237_600_000)


def ring_graph(n, d, w):
    """Directed circulant CSR (indptr, indices, data): row i holds columns i + 1 .. i + d (mod n), ascending; every
    weight w.  Regular and uniform for any degree 0 <= d <= n - 1."""
    assert 0 <= d <= n - 1
    cols = (np.arange(n, dtype=np.int64)[:, None] + np.arange(1, d + 1, dtype=np.int64)[None, :]) % n
    cols.sort(axis=1)
    indptr = np.arange(0, n * d + 1, d, dtype=np.int64) if d else np.zeros(n + 1, dtype=np.int64)
    return indptr, cols.reshape(-1).astype(np.int32), np.full(n * d, float(w), dtype=np.float64)


def as_csr(parts, n):
    indptr, indices, data = parts
    return csr_matrix((data, indices, indptr), shape=(n, n))


def adjacency(parts, n):
    indptr, indices, data = parts
    return csr_matrix((np.ones(indices.size), indices, indptr), shape=(n, n))


def saturating_counts(n, G, seed):
    """(n, G) float32 counts.  Even genes: 255 everywhere except cells [0, 300), which are uniform in 0 .. 255 (so the
    gene has a variance); on a ring of degree 257 most cells then have the neighbour sum 65535 exactly, and the gene in
    the other half of each packed word would show any carry.  Odd genes: min(Poisson(1.2), 15), one nibble."""
    rng = np.random.default_rng(seed)
    X = np.minimum(rng.poisson(1.2, (n, G)), 15).astype(np.float32)
    n_even = X[:, ::2].shape[1]
    X[:, ::2] = 255.0
    m = min(300, n)
    X[:m, ::2] = rng.integers(0, 256, (m, n_even))
    return X


def straddling_genes(n=4096, d=257):
    """(n, 2) float64: two uint16-class genes whose lattice products d x 65535 x total lie on either side of 4.0e15,
    4e-4 away from it (3.9984e15 and 4.0018e15 at d = 257): rounding cannot decide the side.  The sine makes the genes
    strongly autocorrelated on the ring (I ~ 0.97), so that the near-tie rule of the float comparison is not smaller than
    the oracle's own rounding noise on the identity row."""
    out = np.empty((n, 2), dtype=np.float64)
    i = np.arange(n)
    for k, total in enumerate(STRADDLE_TOTALS):
        rng = np.random.default_rng(100 + k)
        x = np.rint(total / n + 7000.0 * np.sin(2 * np.pi * i / n) + rng.integers(-200, 201, n)).astype(np.int64)
        x[0] = 65535
        q, r = divmod(int(total - x.sum()), n - 1)      # level cells 1 .. n - 1 to the exact total
        x[1:] += q
        x[1:1 + r] += 1
        assert x.sum() == total and x.min() >= 0 and x.max() == 65535
        out[:, k] = x
    return out


def identity_first(perms):
    """The table with row 0 replaced by the identity: every lattice gene has one exact tie to count."""
    perms = np.array(perms, dtype=np.int32, copy=True)
    perms[0] = np.arange(perms.shape[1], dtype=np.int32)
    return perms


# ---- the host's guards, restated ----

def score_cells_per_split(n):
    """Cells of one scoring task (score_cells_per_split in sc_moran.hip): a function of n alone."""
    cps = -(-(-(-n // 512)) // 8) * 8
    return max(cps, 2048)


def u8_prelude_allowed(d):
    return d <= 257


def nibble_guard(xmax_all, d, n):
    return 15.0 * float(xmax_all) * float(d) * float(score_cells_per_split(n)) < NIBBLE_LIMIT


def lattice_product(d, x):
    """What moran_prepare compares with LATTICE_LIMIT for one gene's counts x."""
    return float(d) * float(x.max()) * float(x.sum())


def worst_nibble_sum(parts, X, n):
    """Largest sum over one split's cells of 15 x S (S = neighbour sums of the full counts): the bound of the per-task
    uint32 accumulators of the 4-bit source, over all genes and splits."""
    S = np.asarray(adjacency(parts, n) @ np.asarray(X, dtype=np.float64))
    cps = score_cells_per_split(n)
    return max(float((15.0 * S[c0:c0 + cps]).sum(axis=0).max()) for c0 in range(0, n, cps))
