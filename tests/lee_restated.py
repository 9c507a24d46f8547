"""Inputs of the Lee's L edge tests (tests/test_gpu_kernels.py) and the reference's core loop restated on them in float64
numpy: z-scores with the population sd (0 for a constant gene), L = z_x . (W z_y), L_perm = (W^T z_x) . z_y[perm] and
#{|L_perm| >= |L|}.  tests/test_cpu_lee_restated.py checks without a device that no comparison of these inputs is a near
tie, so the device's counts may be compared with ==."""
import functools

import numpy as np

from conftest import synth

K = 6
NEAR_TIE = 1e-6          # relative distance of |L_perm| from |L| below which a count could depend on summation order

# the per-pair rows (sc_lee_seeded, sc_lee): one cell into the second wavefront's quarter of an observed block, into the
# second 8192-cell row block, into the second 16384-cell observed block -- each leaves a ragged quad of cells for the MFMA
ROW_SIZES = (4097, 8193, 16385)
ROW_GENES, ROW_CONSTANT, ROW_P, ROW_SEED = 20, 5, 3, 61     # two 16-gene tiles
ROW_PAIRS = np.array([[0, 1], [2, 17], [ROW_CONSTANT, 3], [18, 1]])    # same tile, across tiles, dead, across again

# the shared grid (sc_lee_shared): nine x tiles = one full pass of eight and a pass of one ragged tile (2 genes)
GRID_N, GRID_X, GRID_Y, GRID_P, GRID_SEED = 4099, 130, 17, 2, 62


def _operands(oracle, n, genes, seed, constant=None):
    coords, X = synth(n, genes, seed, dtype=np.float64, sparse_x=False)
    if constant is not None:
        X[:, constant] = 3.0
    W = oracle.reference_weights(coords, K).astype(np.float64)
    sd = X.std(axis=0)
    Z = np.where(sd > 0, (X - X.mean(axis=0)) / np.where(sd > 0, sd, 1), 0.0)
    return coords, X, W, Z


@functools.lru_cache(maxsize=None)
def rows_case(oracle, n):
    """A fresh block of ROW_P permutations per live pair, in pair order, from one stream (AC:1129-1140)."""
    coords, X, W, Z = _operands(oracle, n, ROW_GENES, ROW_SEED + n % 7, ROW_CONSTANT)
    live = np.array([a != ROW_CONSTANT and b != ROW_CONSTANT for a, b in ROW_PAIRS])
    perms, words = oracle.perm_table(ROW_SEED, n, int(live.sum()) * ROW_P)
    offset = np.where(live, (np.cumsum(live) - 1) * ROW_P, -1)
    L, Lp = np.zeros(len(ROW_PAIRS)), np.zeros((len(ROW_PAIRS), ROW_P))
    for q, (a, b) in enumerate(ROW_PAIRS):
        if live[q]:
            L[q] = Z[:, a] @ (W @ Z[:, b])
            u = W.T @ Z[:, a]
            Lp[q] = [u @ Z[perms[offset[q] + p], b] for p in range(ROW_P)]
    return {"coords": coords, "X": X, "live": live, "offset": offset, "words": words, "L": L, "L_perm": Lp,
            "count": (np.abs(Lp) >= np.abs(L)[:, None]).sum(axis=1)}


@functools.lru_cache(maxsize=None)
def grid_case(oracle):
    """One block of GRID_P permutations shared by the whole grid."""
    coords, X, W, Z = _operands(oracle, GRID_N, GRID_X + GRID_Y, GRID_SEED)
    gx, gy = np.arange(GRID_X), np.arange(GRID_X, GRID_X + GRID_Y)
    perms, words = oracle.perm_table(GRID_SEED, GRID_N, GRID_P)
    L = Z[:, gx].T @ (W @ Z[:, gy])
    U = W.T @ Z[:, gx]
    Lp = np.stack([U.T @ Z[perms[p]][:, gy] for p in range(GRID_P)])
    return {"coords": coords, "X": X, "gx": gx, "gy": gy, "words": words, "L": L, "L_perm": Lp,
            "count": (np.abs(Lp) >= np.abs(L)[None]).sum(axis=0)}


def near_ties(L, Lp):
    """Comparisons |L_perm| >= |L| closer than NEAR_TIE (L broadcast against the permutation axis by the caller)."""
    return int((np.abs(np.abs(Lp) - np.abs(L)) < NEAR_TIE * np.abs(L)).sum())
