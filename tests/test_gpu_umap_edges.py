"""sc_fuzzy_graph and sc_umap_layout at the constants of their kernels (sc_umap.hip), against the numpy restatement
(tests/umap_restated.py: ``fuzzy_edge_recipes``, ``layout_edge_recipes``), whose recipes' properties are asserted on the
host in tests/test_cpu_umap.py.  tests/test_gpu_umap.py chose its inputs for the algorithm's branches; these are chosen for

- the global mean distance (k_um_chunk_sum, k_um_mean): ``mixed`` has rows with rho = 0 beside ordinary ones, so the mean
  is not zero and reaches sigma; n = 1023, 1024, 1025 and 2049 stand around SUM_CHUNK = 1024, and in each the chunked
  order gives other bits than a plain running sum;
- the list widths on both sides of k_um_sigma<8>, <16> and <32>: k = 8, 9, 16, 17, 31 and 2, the least the search admits;
- the negatives' blocks of four per Philox call in k_um_epoch: neg = 1, 3, 4, 8, 9, 16;
- the Philox key's high word: a seed above 2^32;
- k_um_wmax's grid of 2048 x 256 threads: a graph of 560,000 stored entries whose largest weight is among the last 29;
- rows without entries, gamma = 0, another a and b, and epoch indices near 10^9 of a 2^31 - 1 epoch schedule.

The policy is the one of tests/test_gpu_umap.py.  What is derivable is compared byte for byte: rho, the union's pattern,
sigma of the rho = 0 rows (one sum in a pinned order, one division, one product), rows without entries, and every
statement about one run against another.  The other sigma, the weights and the positions go through exp and pow;
MEASURED_* are the largest differences over the inputs of this file as scripts/umap_probe.py --tolerances measured them on
an MI355X (profiles/umap_1m.json, "tolerances_edges"); the tests assert ten times those figures and never more than 1e-9."""
import functools

import numpy as np
import pytest
from scipy import sparse

import diffusion_restated as R
import umap_restated as U

pytestmark = pytest.mark.gpu

CAP = 1e-9
MEASURED_SIGMA = 0.0            # every sigma came out bit-equal, at every list width and in the rows floored at a row mean
MEASURED_W = 4.38e-16           # (mixed-n1025-k17)
MEASURED_LAYOUT = 4.66e-13      # of the start's extent (neg16-C2, whose restatement itself moves by 4.8e-13 under a one-ulp
#                                 change of its pow: tests/test_cpu_umap.py; the next, late-epochs, gave 3.2e-14)
TOL_SIGMA, TOL_W, TOL_LAYOUT = (min(10 * m, CAP) for m in (MEASURED_SIGMA, MEASURED_W, MEASURED_LAYOUT))
NORMAL = 1e-300                 # below this a double has lost bits and a relative difference says nothing


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


def _rel(got, ref):
    """Largest relative difference over the normal-range entries; the others must be tiny on both sides."""
    big = ref >= NORMAL
    assert np.all(got[~big] < 10 * NORMAL)
    return float(np.max(np.abs(got[big] - ref[big]) / ref[big])) if big.any() else 0.0


# ---- 1. the fuzzy graph ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fuzzy_truth(name):
    X, k = U.fuzzy_edge_recipes()[name]
    idx, d2 = R.knn(X, k)
    return X, k, idx, d2, U.fuzzy_graph(idx, d2)


@pytest.mark.parametrize("name", list(U.fuzzy_edge_recipes()))
def test_fuzzy_graph_equals_the_restatement_at_chunk_and_width_edges(name):
    X, k, idx, d2, g = _fuzzy_truth(name)
    n = X.shape[0]
    ctx = _ctx()
    got_idx, got_d2 = ctx.knn_dense(X, k)
    assert np.array_equal(got_idx, idx) and got_d2.tobytes() == d2.tobytes()
    info = ctx.fuzzy_graph()
    indptr, indices, w, T = ctx.diffmap_graph_get(transition=True)
    assert info["n_edges"] == indices.size == g["indices"].size
    assert indptr.tobytes() == g["indptr"].tobytes() and indices.tobytes() == g["indices"].tobytes()
    assert info["rho"].tobytes() == g["rho"].tobytes()
    zero = g["rho"] == 0
    if name.startswith("mixed"):
        assert zero.sum() == k + 2 and np.all(g["sigma"][zero] == 1e-3 * g["info"]["global_mean"])
        print(f"{name}: sigma of the rho = 0 rows {info['sigma'][zero][0]!r}, restated {g['sigma'][zero][0]!r}")
    else:
        assert not zero.any()
    assert info["sigma"][zero].tobytes() == g["sigma"][zero].tobytes()             # the global mean in its pinned order
    rel_sigma, rel_w = _rel(info["sigma"][~zero], g["sigma"][~zero]), _rel(w, g["w"])
    print(f"{name}: max relative difference sigma {rel_sigma:.3e}, w {rel_w:.3e}")
    assert rel_sigma <= TOL_SIGMA and rel_w <= TOL_W
    A = sparse.csr_matrix((w, indices, indptr), shape=(n, n))
    At = A.T.tocsr()
    At.sort_indices()
    assert np.array_equal(At.indices, indices) and At.data.tobytes() == w.tobytes()          # bit-symmetric
    assert info["n_components"] == R.n_components(indptr, indices)
    assert np.all(np.isfinite(T)) and np.all(T >= 0)


def test_the_search_admits_no_list_shorter_than_the_shortest_width_tested():
    with pytest.raises(ValueError, match="need 2 <= k"):
        _ctx().knn_dense(U.features(129, 8), min(U.WIDTH_KS) - 1)


# ---- 2. the layout ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cases():
    return U.layout_edge_recipes()


@functools.lru_cache(maxsize=None)
def _layout_truth(name):
    return U.layout_case_epochs(_cases()[name])


def _device(case, e0=None, e1=None, Y=None, **change):
    run = {**case["run"], **change}
    return _ctx().umap_layout(case["graph"], case["Y0"] if Y is None else Y, run["a"], run["b"], run["gamma"], 1.0, run["neg"],
                              run["n_epochs"], run["seed"], run["e0"] if e0 is None else e0, run["e1"] if e1 is None else e1)


@pytest.mark.parametrize("name", list(U.layout_edge_recipes()))
def test_layout_epochs_equal_the_restatement_at_the_edges(name):
    case = _cases()[name]
    Y0 = case["Y0"]
    empty = np.flatnonzero(np.diff(case["graph"][0]) == 0)
    assert empty.size == (2 if name == "star-empty-rows" else 0)
    for e1, ref in _layout_truth(name):
        got = _device(case, e1=e1)
        assert got.dtype == np.float64 and got.shape == Y0.shape
        diff = float(np.max(np.abs(got - ref))) / case["extent"]
        print(f"{name}: epochs [{case['run']['e0']}, {e1}): max |Y - restated| / {case['extent']:g} = {diff:.3e}")
        assert diff <= TOL_LAYOUT
        assert got[empty].tobytes() == Y0[empty].tobytes()                  # a row without entries copies Yold to Ynew
    assert not np.array_equal(got, Y0)


# ---- 3. one run against another, byte for byte -------------------------------------------------------------------------------
def test_the_seeds_high_word_reaches_the_philox_key():
    case = _cases()["seed-high-word"]
    assert case["run"]["seed"] == U.HIGH_SEED and U.HIGH_SEED & 0xFFFFFFFF == 11
    assert _device(case).tobytes() != _device(case, seed=11).tobytes()


def test_gamma_zero_gives_the_bytes_of_a_run_without_negatives():
    zero, none = _cases()["gamma0"], _cases()["gamma0-neg0"]
    assert zero["run"]["neg"] == 5 and none["run"]["neg"] == 0
    assert _device(zero).tobytes() == _device(none).tobytes()


@pytest.mark.parametrize("name", ["neg16-C2", "neg16-C3", "ring-wmax-tail"])
def test_a_second_run_gives_the_same_bytes(name):
    case = _cases()[name]
    assert _device(case).tobytes() == _device(case).tobytes()


@pytest.mark.parametrize("name", ["neg16-C2", "neg16-C3"])
def test_split_epoch_ranges_give_the_bytes_of_one_range(name):
    case = _cases()[name]
    assert _device(case, 2, 3, Y=_device(case, 0, 2)).tobytes() == _device(case, 0, 3).tobytes()
