"""Inputs that take sc_nmf_fit_graph (sc_nmf.hip) to the edges its first tests stop short of (plain numpy,
no GPU).

  chunk      NMF_CELL_CHUNK = 1024 cells per partial of the sums over cells: n = 1024, 1025, 1300, 1500, 2049 with
             edge_graph relabelled by c -> (c + 1010) mod n, so that the chain crosses 1023 | 1024 and the planted degrees
             sit on the cells 1010 .. 1033 (the isolated cell on 1010): graph rows whose neighbours lie in the other chunk
  hub        the chain 0 .. n - 1 and cell 1100 joined to every other cell: a graph row of n - 1 entries, hundreds of
             fetches of lane_group_walk, its neighbours in both chunks
  zeros      W rows, a W column and an H row of exact zeros in the start: den == 0 -> EPS in the graph W pass
  float32    values handed over as float32 (k_nmf_values<float>, nmf_xconst<float>)
  stop       two (lambda, tol) at which the stop rule on the objective and on the error end at different iterations
  extremes   lambda = 1e-12 and 1e8; weights over twelve decades
  counts     max_iter = 1, 10, 11

Every input comes from a fixed seed.  tests/test_cpu_spatial_nmf_edges.py proves, with the restatement alone, that each
input is what tests/test_gpu_spatial_nmf_edges.py says it is; the restated fits are computed once per process
(functools.lru_cache) and handed out read-only."""
import functools

import numpy as np
from scipy import sparse

import nmf_restated as R
import spatial_nmf_restated as S

LAMBDA = 2.5
SHIFT = 1010                                  # the relabelling of the chunk cases
HUB = 1100                                    # the hub cell: in the second cell chunk
CHUNK_TRIPLES = [(1024, 19, 3), (1025, 17, 1), (1500, 19, 3), (1500, 17, 1), (2049, 23, 33), (1300, 21, 64)]   # n, G, K
# 13 iterations: a check at iteration 10, three more passes, the tail evaluation; K = 64 gets 3 (the restatement's time)
CHUNK_RUNS = [(n, G, K, it) for n, G, K in CHUNK_TRIPLES for it in ((3, 13) if K <= 33 else (3,))]
# a second chunk of one cell (or none) adds the chunk sums exactly as one running sum does: bounds cases only
CHUNK_ORDER_SHOWS = [(1500, 19, 3), (1500, 17, 1), (2049, 23, 33), (1300, 21, 64)]
HUB_RUNS = [(1500, 17, 1, 13), (1500, 19, 3, 13), (1300, 21, 64, 3)]                                           # n, G, K, iterations
HUB_WEIGHT_SEED = 41
ZERO_TRIPLE = (259, 37, 20)
SMALL_TRIPLE = (130, 21, 3)
F32_TRIPLES = [(130, 21, 3), (150, 23, 64)]
STOP_RULES = [(1000.0, 1e-2, 50, 90), (1.0, 1e-3, 60, 50)]     # lambda, tol, the stop on the objective, on the error
EXTREME_LAMBDAS = (1e-12, 1e8)
WEIGHT_DECADES = 6.0                                            # weights x 10^u, u uniform in [-6, 6]
COUNT_ITERS = (1, 10, 11)
KEYS = ("W", "H", "objective_trace", "error_trace")


def kp_of(K):
    return 256 // R.w_rows_per_workgroup(K)


def relabel(A, shift):
    """The graph with cell c renamed (c + shift) mod n."""
    n = A.shape[0]
    to = (np.arange(n) + shift) % n
    coo = sparse.coo_matrix(A)
    return S._symmetric_csr(to[coo.row], to[coo.col], coo.data, n)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _start(X, K):
    return _frozen(*R.start(X, K, 7))


# ---- builders: each returns (X, A, W0, H0, facts) --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_case(n, G, K):
    """The "edge" case of tests/test_gpu_spatial_nmf.py, unchanged."""
    X = R.counts(n, G, 3, 200 + K)
    A, special = S.edge_graph(n, kp_of(K), 300 + K)
    W0, H0 = _start(X, K)
    return X, A, W0, H0, {"special": special}


@functools.lru_cache(maxsize=None)
def chunk_case(n, G, K):
    X = R.counts(n, G, 3, 200 + K)
    A0, special = S.edge_graph(n, kp_of(K), 300 + K)
    A = relabel(A0, SHIFT)
    W0, H0 = _start(X, K)
    return X, A, W0, H0, {"special": {d: (c + SHIFT) % n for d, c in special.items()}, "unshifted": A0}


def hub_graph(n, hub, seed):
    """The chain 0 -- 1 -- ... -- n - 1 and ``hub`` joined to every other cell; weights symmetric, uniform in [0.1, 3]."""
    edges = {(i, i + 1) for i in range(n - 1)} | {(min(hub, j), max(hub, j)) for j in range(n) if j != hub}
    e = np.asarray(sorted(edges), dtype=np.int64)
    w = np.random.default_rng(seed).uniform(0.1, 3.0, size=e.shape[0])
    return S._symmetric_csr(np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), np.concatenate([w, w]), n)


@functools.lru_cache(maxsize=None)
def hub_case(n, G, K):
    X = R.counts(n, G, 3, 200 + K)
    A = hub_graph(n, HUB, HUB_WEIGHT_SEED)
    W0, H0 = _start(X, K)
    return X, A, W0, H0, {"hub": HUB}


@functools.lru_cache(maxsize=None)
def zero_case():
    """edge_case(259, 37, 20) with W0[isolated cell] = W0[the cell of degree Kp] = 0, W0[:, K - 1] = 0, H0[2] = 0."""
    n, G, K = ZERO_TRIPLE
    X, A, W0, H0, facts = edge_case(n, G, K)
    rows = (0, facts["special"][kp_of(K)])
    W0, H0 = W0.copy(), H0.copy()
    W0[list(rows)] = 0.0
    W0[:, K - 1] = 0.0
    H0[2] = 0.0
    _frozen(W0, H0)
    return X, A, W0, H0, {"zero_rows": rows, "zero_column": K - 1, "zero_component": 2}


@functools.lru_cache(maxsize=None)
def f32_case(n, G, K):
    """log1p of the counts rounded to float32 and kept as float32; facts["X64"] holds the unrounded float64 values."""
    C, A, _, _, _ = edge_case(n, G, K)
    X64 = C.copy()
    X64.data = np.log1p(C.data)
    X = X64.astype(np.float32)
    assert X.dtype == np.float32 and X.data.dtype == np.float32 and X.has_canonical_format
    W0, H0 = _start(X, K)
    return X, A, W0, H0, {"X64": X64}


@functools.lru_cache(maxsize=None)
def stop_case():
    X, xy, _ = S.planted(600, 30, 4, 1)
    W0, H0 = _frozen(*R.start(X, 4, 0))
    return X, S.knn_union(xy, 6), W0, H0, {}


@functools.lru_cache(maxsize=None)
def decades_case():
    """edge_case(130, 21, 3) with every edge's weight multiplied by 10^u, u uniform in [-WEIGHT_DECADES, WEIGHT_DECADES],
    the same factor on both stored entries of the edge."""
    X, A, W0, H0, _ = edge_case(*SMALL_TRIPLE)
    up = sparse.triu(A, k=1).tocoo()
    u = np.random.default_rng(61).uniform(-WEIGHT_DECADES, WEIGHT_DECADES, size=up.nnz)
    w = up.data * 10.0 ** u
    B = S._symmetric_csr(np.concatenate([up.row, up.col]), np.concatenate([up.col, up.row]), np.concatenate([w, w]), A.shape[0])
    return X, B, W0, H0, {"factors": 10.0 ** u}


BUILDERS = {"edge": edge_case, "chunk": chunk_case, "hub": hub_case, "zeros": zero_case, "f32": f32_case, "stop": stop_case,
            "decades": decades_case}


def case(kind, *args):
    """(X, A, W0, H0) of a case."""
    return BUILDERS[kind](*args)[:4]


@functools.lru_cache(maxsize=None)
def restated(kind, args, lam, max_iter, tol):
    """spatial_nmf_restated.ordered on a case, computed once and read-only."""
    X, A, W0, H0 = case(kind, *args)
    out = S.ordered(X, A, lam, W0, H0, max_iter=max_iter, tol=tol)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- what the CPU test measures ----------------------------------------------------------------------------------------------
def cross_chunk_entries(A):
    """Stored graph entries whose row and column lie in different cell chunks."""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return int(np.sum(rows // R.CELL_CHUNK != A.indices // R.CELL_CHUNK))


def penalty_sums(X, A, W):
    """R added in chunks of 1024 cells (the device's order) and as one running sum over all cells."""
    o = S._OrderedGraph(X, W.shape[1], A, LAMBDA)
    r = o.row_penalties(np.asarray(W))
    return float(R._seq(R._seg_sum(r, o.cell_ptr), 0)), float(R._seq(r, 0))


def hub_sums(A, W, hub):
    """g_hub,k = sum_e a_e W[j_e][k] in index order from 0 (the device's) and as an adjacent-pair tree of the same products."""
    lo, hi = A.indptr[hub], A.indptr[hub + 1]
    prod = A.data[lo:hi, None] * np.asarray(W)[A.indices[lo:hi]]
    return R._seq(prod, 0), R._tree(prod.T)


def first_w_pass_terms(X, A, lam, W0, H0):
    """(num, den) of the first W pass, before the den == 0 guard."""
    o = S._OrderedGraph(X, W0.shape[1], A, lam)
    HHt, _ = o.hprep(np.asarray(H0))
    return o.w_terms(np.asarray(W0), np.asarray(H0), HHt)


def first_stop(trace, tol):
    """The iteration at which sklearn's rule stops on ``trace`` (checks every tenth iteration), None if it never does."""
    t = np.asarray(trace, dtype=np.float64)
    for c in range(1, t.size):
        if (t[c - 1] - t[c]) / t[0] < tol:
            return 10 * c
    return None
