"""The restatement of local Moran and local Lee (tests/local_restated.py) pinned to what the reference runs, without a
device: scipy's sparse product, the oracle's local_morans_i, and the reference's own goldens -- all bit for bit.  Only
then is it fit to judge the device (tests/test_gpu_local.py)."""
import numpy as np
import pytest
from scipy import sparse

import local_restated as lr
from conftest import load_golden, synth

N, G, P, K, BATCH, SEED = 2000, 150, 37, 6, 100, 3
FIELDS = ("z", "lag", "I", "p")


def restated_local_morans(oracle, coords, X, k, n_perm, seed, batch):
    """The reference's flow on top of the restatement: arrays once, counts per batch of genes from one generator,
    p = float32((count + 1) / (P + 1)); flagged genes get z = lag = I = 0 and p = 1."""
    X = np.asarray(X)
    n, genes = X.shape
    W = oracle.reference_weights(coords, k)
    assert W.dtype == np.float32 and W.has_sorted_indices
    z, lag, I, zero = lr.local_moran_arrays(X, X.dtype.type, W.indptr, W.indices, W.data)
    p = np.ones((n, genes), dtype=np.float32)
    if n_perm > 0:
        batches = range(0, genes, batch)
        table, _ = oracle.perm_table(seed, n, n_perm * len(batches))
        for bi, b0 in enumerate(batches):
            b1 = min(b0 + batch, genes)
            cnt = lr.local_moran_counts(W.indptr, W.indices, W.data, z[:, b0:b1], I[:, b0:b1],
                                        table[bi * n_perm:(bi + 1) * n_perm])
            p[:, b0:b1] = lr.pvalue32(cnt, n_perm)
    for a in (z, lag, I):
        a[:, zero] = 0.0
    p[:, zero] = 1.0
    return {"z": z, "lag": lag, "I": I, "p": p, "zero": zero, "W": W}


def graphs(oracle, n=700, k=6):
    """(name, float32 CSR): a kNN graph, unequal float32 weights, a graph with empty rows."""
    coords = lr.uniform_coords(n, 2)
    idx = oracle.knn_bruteforce(coords, k)
    out = [("knn", oracle.reference_weights(coords, k))]
    ip, ix, w = lr.thinned_csr(idx, seed=4)
    out.append(("unequal", sparse.csr_matrix((w.astype(np.float32), ix, ip), shape=(n, n))))
    ip, ix, w = lr.thinned_csr(idx, seed=5, equal_weights=True, empty_every=9)
    assert (np.diff(ip) == 0).any()
    out.append(("empty-rows", sparse.csr_matrix((w.astype(np.float32), ix, ip), shape=(n, n))))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_sequential_is_scipys_product(oracle, dtype):
    rng = np.random.default_rng(8)
    for name, W in graphs(oracle):
        Y = rng.normal(size=(W.shape[0], 7)).astype(dtype)
        for y in (Y, Y[:, 0].copy()):
            got = lr.row_sequential(W.indptr, W.indices, W.data, y)
            want = W @ y
            assert got.dtype == want.dtype == dtype
            np.testing.assert_array_equal(got, want, err_msg=name)


_CASES = {}


def oracle_case(oracle, kind):
    """(oracle's result, restated result) of one input, computed once."""
    if kind in _CASES:
        return _CASES[kind]
    coords, X = synth(N, G, 21, dtype=np.float64 if kind == "counts-f64" else np.float32, normalize=kind == "lognorm-f32")
    X = X.tolil(); X[:, 5] = 3.0; X[:, 140] = 0.0; X = X.tocsr()      # a constant and an empty column
    want = oracle.local_morans_i(coords, X, np.arange(G), K, P, SEED, batch_size=BATCH)
    got = restated_local_morans(oracle, coords, X.toarray(), K, P, SEED, BATCH)
    _CASES[kind] = (want, got)
    return want, got


@pytest.mark.parametrize("kind", ["counts-f32", "counts-f64", "lognorm-f32"])
def test_restatement_reproduces_the_oracle(oracle, kind):
    """n = 2000, G = 150 in batches of 100 and 50, P = 37, k = 6: count data as float32 and float64, and one
    log-normalised float32 matrix."""
    want, got = oracle_case(oracle, kind)
    np.testing.assert_array_equal(got["zero"], want["zero_variance"])
    # (the constant column is flagged only where numpy's q - m m comes out as 0: at 2000 cells in float64, not in float32)
    assert got["zero"][140] and got["zero"][5] == (kind == "counts-f64")
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype == np.float32
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{kind} {f}")


def test_count_data_is_full_of_exact_ties(oracle):
    """A tenth of the (cell, gene, permutation) triples of the count input are exact ties |I_perm| == |I|: the >= of the
    count is exercised, and a rounding that differs in the last bit changes counts."""
    kind = "counts-f32"
    _, got = oracle_case(oracle, kind)
    W, keep = got["W"], ~got["zero"]
    z, absI = got["z"][:, keep], np.abs(got["I"][:, keep])
    table, _ = oracle.perm_table(11, N, 10)
    ties = np.mean([(np.abs(z[p] * lr.row_sequential(W.indptr, W.indices, W.data, z[p])) == absI).mean() for p in table])
    print(f"{kind}: exact ties in {100 * ties:.2f} % of the (cell, gene, permutation) triples")
    assert ties > 0.01


def test_restatement_reproduces_the_local_moran_goldens(oracle):
    g = load_golden("ref_local_morans.npz")
    assert int(g["n_cases"]) == 3
    for ci in range(3):
        X = g[f"c{ci}_X"]
        got = restated_local_morans(oracle, g[f"c{ci}_coords"], X, int(g[f"c{ci}_k"]), int(g[f"c{ci}_P"]),
                                    int(g[f"c{ci}_seed"]), int(g[f"c{ci}_batch"]))
        for f in FIELDS:
            np.testing.assert_array_equal(got[f], g[f"c{ci}_{f}"], err_msg=f"case {ci} {f}")
        assert [f"g{i}" for i in np.flatnonzero(got["zero"])] == list(g[f"c{ci}_zero_variance_genes"])


def test_restatement_reproduces_the_local_lee_golden(oracle):
    """numpy's own z-scores; one generator for all pairs, which draws the P rows of the global statistic before the P
    rows of the per-cell counts."""
    g = load_golden("ref_lees_l_local.npz")
    coords, X, k, n_perm = g["coords"], g["X"], int(g["k"]), int(g["P"])
    W = oracle.reference_weights(coords, k)
    pairs = g["pairs"]
    table, _ = oracle.perm_table(int(g["seed"]), X.shape[0], 2 * n_perm * len(pairs))
    for gi, (a, b) in enumerate(pairs):
        zx, zy = lr.zscores64(X[:, a]), lr.zscores64(X[:, b])
        L = zx * lr.row_sequential(W.indptr, W.indices, W.data, zy)
        rows = table[2 * n_perm * gi + n_perm:2 * n_perm * (gi + 1)]
        cnt = lr.lee_local_counts(W.indptr, W.indices, W.data, zx, zy, L, rows)
        np.testing.assert_array_equal(L.astype(np.float32), g[f"p{gi}_L_local"])
        np.testing.assert_array_equal(lr.pvalue32(cnt, n_perm), g[f"p{gi}_pvalue"])


def test_local_lee_inputs_have_no_near_ties(oracle):
    """Every local Lee input of tests/test_gpu_local.py: no (cell, permutation) of a non-empty row lies within the
    near-tie distance (relative 1e-11) of the observed value, so z-scores that differ from numpy's in their last bits
    cannot change a count and the device comparison may be exact."""
    sx, sy = lr.LEE_PAIR
    total = 0
    for n in lr.LEE_SIZES:
        coords, X = lr.lee_input(n)
        idx = oracle.knn_bruteforce(coords, lr.LEE_K)
        tables = [oracle.perm_table(lr.LEE_TABLE_SEED, n, lr.LEE_TABLE_ROWS)[0]]
        if n == lr.LEE_SIZES[-1]:
            tables += [oracle.perm_table(lr.LEE_SEEDED_SEED, n, pg + pl)[0][pg:] for pg, pl in lr.LEE_SEEDED]
        for kind in lr.LEE_GRAPHS:
            ip, ix, w = lr.lee_graph(kind, idx)
            for a, b in ((sx, sy), (sy, sx)):
                for t in tables:
                    total += lr.lee_near_ties(ip, ix, w, lr.zscores64(X[:, a]), lr.zscores64(X[:, b]), t)
    api = lr.LEE_API
    coords, X = lr.lee_input(api["n"])
    ip, ix, w = lr.knn_csr(oracle.knn_bruteforce(coords, api["k"]), lr.knn_weight(api["k"]))
    table, _ = oracle.perm_table(api["seed"], api["n"], 2 * api["P"] * len(api["pairs"]))
    for gi, (a, b) in enumerate(api["pairs"]):
        rows = table[2 * api["P"] * gi + api["P"]:2 * api["P"] * (gi + 1)]
        total += lr.lee_near_ties(ip, ix, w, lr.zscores64(X[:, a]), lr.zscores64(X[:, b]), rows)
    print(f"near ties of the local Lee inputs: {total}")
    assert total == 0


def test_count_hist_and_classify():
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 8, (50, 3))
    h = lr.count_hist(cnt, 7)
    assert h.shape == (3, 8) and (h.sum(axis=1) == 50).all() and h[1, 4] == (cnt[:, 1] == 4).sum()
    g = load_golden("ref_fdr_quadrants.npz")
    np.testing.assert_array_equal(lr.classify(g["z"], g["lag"], g["pq"], 0.05, np.zeros(3, bool)), g["quad_sig"])
    np.testing.assert_array_equal(lr.classify(g["z"], g["lag"], None, 0.05, np.zeros(3, bool)), g["quad_nosig"])
    flagged = lr.classify(g["z"], g["lag"], None, 0.05, np.array([False, True, False]))
    assert (flagged[:, 1] == 0).all() and (flagged[:, [0, 2]] == g["quad_nosig"][:, [0, 2]]).all()
