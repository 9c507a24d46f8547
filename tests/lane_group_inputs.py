"""Inputs that take the "lanes = classes / components" kernels of sc_annotate.hip and sc_nmf.hip past one lane-group fetch
(plain numpy, no GPU).

A group of w lanes serves one row and fetches w stored entries per trip of its outer loop, adds them four at a time and
ends with a scalar tail of cnt % 4.  ``ladder_lengths`` walks that loop: no trip, one partial trip with every tail, a
full first trip followed by every tail, a second and a third trip, and the row that stores every gene.  The rows are laid
out longest, shortest, second longest, second shortest, ... so that the groups which share a wavefront (w <= 32) run
different trip counts around their shuffles.

Every case keeps one all-zero gene, at column 0 or at column G - 1 (the two ends of the column-pointer search and of the
chunk scan of sc_colsort.h); the "full" row stores every other gene.  ``tall_counts`` has gene columns of 511, 512, 513
and 1029 stored entries (one 512-entry chunk short by one, exact, one past, and two full chunks with a tail of five).

Every input comes from a fixed seed and carries its own structure asserts; ``ladder_facts`` / ``tall_facts`` return what
tests/test_cpu_annotation_lanes.py and tests/test_cpu_nmf_lanes.py print and check.  The restatements are computed once
per process (functools.lru_cache) and handed to the CPU and the GPU tests alike; nobody writes to them."""
import functools

import numpy as np
from scipy import sparse

import annotation_restated as AR
import nmf_restated as NR

TPB = 256                                   # threads per workgroup of every row and column pass
TALL_COLUMNS = (511, 512, 513, 1029)        # stored entries of the first four gene columns of a tall case
CONF_KEYS = ("confidence_raw", "raw", "zscore", "softmax", "minmax")
LOSSES = (NR.LOSS_FRO, NR.LOSS_KL)

# annotation: T of the lane-group sweep (w = lanes(T) = 4, 4, 16, 16, 32, 32, then a full wavefront) and of the class blocks
# (NB = 2 short and full, 3 with one class, two classes, full, 4 with one class, AN_TMAX)
SWEEP_T = (3, 4, 9, 16, 17, 32, 33, 64)
BLOCK_T = (65, 128, 129, 130, 192, 193, 256)
PREDICTIONS = tuple((T, "first") for T in SWEEP_T + BLOCK_T) + tuple((T, "last") for T in BLOCK_T)   # (T, tie construction)
TRANSFORM_T = (128, 192, 193, 256)
PASSES_T = (3, 17, 64, 129, 193, 256)
TALL_T = 193
F32_T = (7, 193)                            # one w = 8 case and one w = 64, NB = 4 case
# nmf: K of the lane-group sweep (kp = 2, 4, 4, 8, 16, 16, 32, 32, 64, 64)
SWEEP_K = (2, 3, 4, 8, 9, 16, 17, 32, 33, 64)
TALL_K = (17, 64)
TALL_N_NMF = 1097                           # one past a multiple of 8 and of 4 rows per workgroup, two cell chunks
KEY_G = (256, 257)                          # 8 key bits exactly; 9 key bits, one above a power of two
KEY_K = 8
ITERS = 3


def kp_of(K):
    kp = 1
    while kp < K:
        kp *= 2
    return kp


# ---- the ladder ------------------------------------------------------------------------------------------------------------
def ladder_lengths(w, G):
    """Row lengths for a group of w lanes over G genes of which one is all zero, ascending and unique.  G - 1 stands for
    "every gene stored": the all-zero gene is stored by nobody."""
    full = G - 1
    raw = [0, 1, 2, 3, 4, 5, 7, 8, w - 1, w, w + 1, w + 2, w + 3, w + 4, 2 * w - 1, 2 * w, 2 * w + 1, 3 * w + 3, full]
    return sorted({L for L in raw if 0 <= L <= full})


def ladder_pattern(w, G):
    """longest, shortest, second longest, second shortest, ..."""
    up = ladder_lengths(w, G)
    out = []
    lo, hi = 0, len(up) - 1
    while lo <= hi:
        out.append(up[hi])
        if lo < hi:
            out.append(up[lo])
        lo, hi = lo + 1, hi - 1
    return out


def ladder_rows(w):
    """n: one past a multiple of the rows per workgroup and at least two workgroups, in the low hundreds."""
    per = TPB // w
    return per * max(2, 128 // per) + 1


@functools.lru_cache(maxsize=None)
def ladder_counts(w, G, zero_gene, seed):
    """Counts (float64 CSR, n x G) whose row lengths repeat ``ladder_pattern``; the genes of a row are drawn with a fixed
    seed from every gene but ``zero_gene``; values are 1 + Poisson(1.5)."""
    assert zero_gene in (0, G - 1)
    n = ladder_rows(w)
    pattern = ladder_pattern(w, G)
    rng = np.random.default_rng(seed)
    storable = np.setdiff1d(np.arange(G), [zero_gene])
    A = np.zeros((n, G))
    for i in range(n):
        L = pattern[i % len(pattern)]
        cols = rng.choice(storable, L, replace=False)
        A[i, cols] = 1.0 + rng.poisson(1.5, L)
    X = sparse.csr_matrix(A)
    X.sort_indices()
    assert X.has_canonical_format and X.data.min() >= 1.0
    assert list(np.diff(X.indptr)) == [pattern[i % len(pattern)] for i in range(n)]
    assert n % (TPB // w) == 1 and n > 2 * (TPB // w) - 1 and n < 400
    per_col = np.diff(X.tocsc().indptr)
    assert per_col[zero_gene] == 0 and np.all(np.delete(per_col, zero_gene) >= 1)      # the full row stores the others
    return X


def ladder_facts(X, w, zero_gene):
    """What a ladder case claims about itself, from the matrix alone."""
    n, G = X.shape
    lens = np.diff(X.indptr)
    trips = -(-lens // w)
    per_col = np.diff(X.tocsc().indptr)
    facts = {"n": n, "G": G, "w": w, "lengths": sorted(set(lens.tolist())), "longest": int(lens.max()),
             "over_w": int((lens > w).sum()), "over_2w": int((lens > 2 * w).sum()), "over_3w": int((lens > 3 * w).sum()),
             "entries_after_a_full_block": sorted({int(L - w) for L in lens if w <= L <= w + 4}),
             "zero_columns": np.flatnonzero(per_col == 0).tolist(), "rows_per_workgroup": TPB // w,
             "remainder": n % (TPB // w), "last_gene_stored": int(per_col[G - 1]), "longest_column": int(per_col.max())}
    if w <= 32:      # the rows that share a wavefront
        share = 64 // w
        windows = [trips[a:a + share] for a in range(0, n - share + 1, share)]
        third = min(3 * w + 3, G - 1)
        facts["wavefronts"] = len(windows)
        facts["wavefronts_with_unequal_trips"] = sum(int(t.max() > t.min()) for t in windows)
        facts["wavefronts_with_an_empty_row_beside_the_third_block"] = sum(
            int(np.any(lens[a:a + share] == 0) and np.any(lens[a:a + share] == third)) for a in range(0, n - share + 1, share))
    return facts


def expected_over(w, G, n, factor):
    """Rows longer than factor * w, from the pattern."""
    pattern = ladder_pattern(w, G)
    return sum(1 for i in range(n) if pattern[i % len(pattern)] > factor * w)


# ---- the tall cases ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tall_counts(n, G, zero_gene, seed):
    """Counts (float64 CSR) with gene columns 0 .. 3 of 511, 512, 513 and 1029 stored entries over a Poisson(0.6)
    background, built as ``_edge_matrix`` of tests/test_gpu_annotation.py; columns 1 .. 4 when gene 0 is the zero gene."""
    assert zero_gene in (0, G - 1) and n >= max(TALL_COLUMNS) and n > AR.CELL_CHUNK
    first = 1 if zero_gene == 0 else 0
    rng = np.random.default_rng(seed)
    A = rng.poisson(0.6, size=(n, G)).astype(np.float64)
    for g, cnt in enumerate(TALL_COLUMNS, start=first):
        A[:, g] = 0
        A[rng.choice(n, cnt, replace=False), g] = rng.integers(1, 6, size=cnt)
    A[:, zero_gene] = 0
    X = sparse.csr_matrix(A)
    X.sort_indices()
    assert list(np.diff(X.tocsc().indptr)[first:first + 4]) == list(TALL_COLUMNS)
    return X


def tall_facts(X, w, zero_gene):
    per_col = np.diff(X.tocsc().indptr)
    first = 1 if zero_gene == 0 else 0
    return {"n": X.shape[0], "G": X.shape[1], "columns": per_col[first:first + 4].tolist(),
            "chunks_of_the_longest": int(-(-per_col.max() // AR.COL_CHUNK)), "zero_columns": np.flatnonzero(per_col == 0).tolist(),
            "remainder": X.shape[0] % (TPB // w), "cell_chunks": int(-(-X.shape[0] // AR.CELL_CHUNK)),
            "longest_row": int(np.diff(X.indptr).max())}


# ---- annotation cases ----------------------------------------------------------------------------------------------------------
def zero_gene_of(T, G):
    """Column 0 and column G - 1 by turns over the cases; G = 257 keeps gene 256 stored."""
    return 0 if (G == 257 or T % 2 == 0) else G - 1


def annotation_genes(T):
    return 257 if T == 129 else 200      # one case with nine key bits, gene 256 stored


def annotation_counts(T):
    G = annotation_genes(T)
    return ladder_counts(AR.lanes(T), G, zero_gene_of(T, G), 500 + T)


def tie_classes(T, tie):
    """"first": classes 0, 64 (the same lane, one block later) and T - 1 tie; for T < 65 classes 0 and T - 1.
    "last": the first class of the last block and class T - 1 tie (one class where the last block holds one)."""
    if tie == "first":
        return sorted({0, T - 1} | ({64} if T >= 65 else set()))
    assert T >= 65
    return sorted({64 * ((T + 63) // 64 - 1), T - 1})


@functools.lru_cache(maxsize=None)
def prediction_case(T, tie="first", f32=False):
    """The ladder of lanes(T), a random model on its expressed genes whose tied classes share one coefficient row and a
    raised intercept, and the ordered restatement of its prediction with the ulp tolerances of the exp-bearing keys.
    ``f32``: the restatement reads the log1p values rounded to float32."""
    counts = annotation_counts(T)
    G = counts.shape[1]
    keep = np.setdiff1d(np.arange(G), [zero_gene_of(T, G)])
    C = counts[:, keep]
    X = AR.log1p_10k(C)
    if f32:
        X = X.astype(np.float32).astype(np.float64)
    mean, scale = AR.scaler(X)
    rng = np.random.default_rng(900 + T)
    # small coefficients: the winning score stays within a few units, where expit is not saturated and the fp64 raw
    # confidence shows the last bits of the fp64 score (the stored scores are float32)
    coef, b = rng.normal(0, 0.05, size=(T, keep.size)), rng.normal(0, 0.5, size=T)
    tied = tie_classes(T, tie)
    # the intercept is raised by the median lead of the other classes (and an eighth, so that the median cell itself is
    # no accidental tie with another class): the tied classes win about half of the cells
    S = AR.dense_scores(X, coef, b, mean, scale)
    b[tied[0]] += np.median(np.delete(S, tied, axis=1).max(axis=1) - S[:, tied[0]]) + 0.125
    for t in tied[1:]:
        coef[t], b[t] = coef[tied[0]], b[tied[0]]
    want, tol = AR.ulp_tolerance(lambda e: AR.ordered_predict(X, coef, b, mean, scale, e), CONF_KEYS)
    for a in (coef, b, mean, scale, *want.values(), *tol.values()):
        a.setflags(write=False)
    return {"counts": C, "X": X, "keep": keep, "coef": coef, "intercept": b, "mean": mean, "scale": scale, "want": want,
            "tol": tol, "tied": tied, "empty": np.flatnonzero(np.diff(C.indptr) == 0)}


@functools.lru_cache(maxsize=None)
def transform_matrix(T, dtype):
    """About 200 rows of scores: row 0 all equal (the sd and the range guard), row 1 with its maximum in the last class,
    row 2 with its maximum in class 64, row 3 with the maximum in both (the first wins), the rest normal."""
    rng = np.random.default_rng(1300 + T)
    S = rng.normal(0, 2.0, size=(201, T))
    S[0] = 1.25
    S[1, T - 1] = S[1].max() + 1.5
    S[2, 64] = S[2].max() + 1.5
    S[3, 64] = S[3, T - 1] = S[3].max() + 0.5
    S = S.astype(dtype)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def transform_case(T, dtype):
    S = transform_matrix(T, dtype)
    keys = ("raw", "zscore", "softmax", "minmax")
    want, tol = AR.ulp_tolerance(lambda e: AR.confidences(S.astype(np.float64), e), keys)
    return S, want, tol


def plain_confidences(F):
    """The four transforms with numpy's own sums (no particular order), float64."""
    F = np.asarray(F, dtype=np.float64)
    T = F.shape[1]
    best = F.max(axis=1)
    mean = np.sum(F, axis=1) / T
    sd = np.sqrt(np.sum((F - mean[:, None]) ** 2, axis=1) / T)
    sd = np.where(sd < 1e-10, 1.0, sd)
    mn = F.min(axis=1)
    rng = np.where(best - mn < 1e-10, 1.0, best - mn)
    return {"raw": best, "zscore": 1.0 / (1.0 + np.exp(-((best - mean) / sd))), "softmax": 1.0 / np.sum(np.exp(F - best[:, None]), axis=1),
            "minmax": (best - mn) / rng, "argmax": np.argmax(F, axis=1)}


@functools.lru_cache(maxsize=None)
def passes_case(T):
    """The ladder of lanes(T) with its all-zero gene left in (log1p values), and labels."""
    X = AR.log1p_10k(annotation_counts(T))
    labels = np.random.default_rng(1100 + T).integers(0, T, X.shape[0]).astype(np.int32)
    return X, labels


@functools.lru_cache(maxsize=None)
def tall_annotation_case():
    """n = 1029, G = 70, T = 193: gene columns of 511, 512, 513 and 1029 (512 + 512 + 5) stored entries at NB = 4."""
    n, G = 1029, 70
    C = tall_counts(n, G, G - 1, 71)
    assert np.diff(C.indptr).min() >= 1                                   # (the full column: no empty cell)
    labels = np.random.default_rng(72).integers(0, TALL_T, n).astype(np.int32)
    return AR.log1p_10k(C), labels


# ---- nmf cases -----------------------------------------------------------------------------------------------------------------
def nmf_counts(K, G=200):
    zero = 0 if (G == 257 or K % 2 == 0) else G - 1
    return ladder_counts(kp_of(K), G, zero, 700 + K + G), zero


@functools.lru_cache(maxsize=None)
def nmf_case(K, G=200):
    X, _ = nmf_counts(K, G)
    W0, H0 = NR.start(X, K, 800 + K)
    return X, W0, H0


@functools.lru_cache(maxsize=None)
def nmf_tall_case(K):
    X = tall_counts(TALL_N_NMF, 70, 0 if K % 2 == 0 else 69, 73)
    W0, H0 = NR.start(X, K, 74 + K)
    return X, W0, H0


@functools.lru_cache(maxsize=None)
def nmf_ordered(kind, K, G, loss, update_H=True):
    """The restatement in the device's order over ITERS iterations without a check (tol = 0), computed once."""
    X, W0, H0 = nmf_tall_case(K) if kind == "tall" else nmf_case(K, G)
    if not update_H:
        W0 = projection_start(X, K)
    out = NR.ordered(X, W0, H0, loss, update_H=update_H, max_iter=ITERS, tol=0.0)
    assert out["n_iter"] == ITERS and len(out["error_trace"]) == 1
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def projection_start(X, K):
    """sklearn's constant start of NMF.transform."""
    return np.full((X.shape[0], K), np.sqrt(X.mean() / K))
