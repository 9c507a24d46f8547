"""sc_hop_* and spatial.aggregate_neighbors on the device against tests/hops_restated.py: the shells byte for byte
(indptr and indices), the aggregates bit for bit against the restatement in the device's order, the public function's
columns, and the recipe end to end.

The row classes of the expansion (csrc/sc_hops.hip): a row whose key bound 1 + sum |shells so far| + sum of the degrees of
the current shell's members is at most WAVE_KEYS = 512 takes a wavefront's table in LDS, at most WG_KEYS = 16384 a
workgroup's, anything larger a table in global memory, in batches of at most GLOBAL_BATCH_BYTES = 64 MiB of tables.  The
star cases put a row's bound at each limit - 1, at it and at it + 1; hops_restated.key_bounds restates the bound and the
tests assert the figures they aim at."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import sparse

import hops_restated as R
from conftest import make_adata

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_KEYS, WG_KEYS, GLOBAL_BATCH_BYTES = 512, 16384, 64 << 20
DIMS = (1, 3, 16, 17, 64)


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


# ---- the graphs: name -> (pattern, hops) -----------------------------------------------------------------------------------------
def _star_cases():
    cases = {}
    for cls, cap in (("wave", WAVE_KEYS), ("wg", WG_KEYS)):
        for delta in (-1, 0, 1):
            # directed star: the hub's and leaf 1's bound are both h + 2, and leaf 1's table takes exactly that many keys
            cases[f"dstar-{cls}{delta:+d}"] = (functools.partial(R.directed_star, cap + delta - 2), cap + delta, cap + delta)
    for delta in (-1, 0, 1):
        target = WAVE_KEYS + delta
        # undirected star: a leaf's bound is h + 2; the hub's is 2 h + 1, or 2 h + 2 with the pendant cell
        cases[f"star-leaf-wave{delta:+d}"] = (functools.partial(R.star, target - 2), 2 * (target - 2) + 1, target)
        h, pendant = (target - 1) // 2 if target % 2 else (target - 2) // 2, target % 2 == 0
        cases[f"star-hub-wave{delta:+d}"] = (functools.partial(R.star, h, pendant), target, h + 2)
    return cases


STARS = _star_cases()     # name -> (maker, the hub's bound, a leaf's bound) at the hop from shell 1 to shell 2


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name in R.KNN_CASES:
        return R.knn_case(name)
    if name in STARS:
        return STARS[name][0](), 3
    return {
        "directed": lambda: (R.directed(500, 4, 3), 4),
        "hub": lambda: (R.hub_graph(), 3),
        "path40": lambda: (R.path(40), 45),
        "isolated": lambda: (R.with_isolated_cell(R.knn_union(R.uniform_points(400, 7), 6), 123), 4),
        "components": lambda: (R.two_components(150, 37, 5, 8), 12),
    }[name]()


@functools.lru_cache(maxsize=None)
def _want(name):
    A, L = _graph(name)
    return R.shells_textbook(A, L)


@functools.lru_cache(maxsize=None)
def _device(name):
    """[(indptr, indices, (nnz, longest row, empty rows))] of the shells 1 .. L from sc_hop_begin / _next / _get."""
    A, L = _graph(name)
    ctx = _ctx()
    ctx.hop_begin(A.indptr, A.indices, A.shape[0])
    try:
        degree = np.diff(A.indptr)
        out = [ctx.hop_get() + ((int(A.nnz), int(degree.max()), int(np.count_nonzero(degree == 0))),)]
        for _ in range(1, L):
            stats = ctx.hop_next()
            out.append(ctx.hop_get() + (stats,))
    finally:
        ctx.hop_end()
    return out


def _assert_shells(name):
    want, got = _want(name), _device(name)
    assert len(got) == len(want)
    for l, (S, (indptr, indices, stats)) in enumerate(zip(want, got), start=1):
        w_ptr, w_idx = R.as_arrays(S)
        assert indptr.dtype == np.int64 and indices.dtype == np.int32
        assert indptr.tobytes() == w_ptr.tobytes(), f"{name}: indptr of shell {l}"
        assert indices.tobytes() == w_idx.tobytes(), f"{name}: indices of shell {l}"
        rows = np.diff(w_ptr)
        assert stats == (int(S.nnz), int(rows.max()), int(np.count_nonzero(rows == 0))), f"{name}: counts of shell {l}"


# ---- 1. the shells ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.KNN_CASES) + ["directed", "isolated", "components"])
def test_shells_equal_the_restatement(name):
    _assert_shells(name)
    shells = _want(name)
    if name in R.KNN_CASES:
        print(f"{name}: largest visited set {R.largest_visited_set(shells)} keys")
    if name == "isolated":
        assert all(S[123].nnz == 0 and S[:, 123].nnz == 0 for S in shells)
    if name == "components":
        assert all(S[:150, 150:].nnz == 0 and S[150:, :150].nnz == 0 for S in shells) and shells[-1][150:].nnz == 0


@pytest.mark.parametrize("name", list(STARS))
def test_shells_on_stars_at_the_class_limits(name):
    from spatialcore_amd import _lib

    assert (WAVE_KEYS, WG_KEYS) == (_lib.HOP_WAVE_KEYS, _lib.HOP_WG_KEYS)
    A, _ = _graph(name)
    bound = R.key_bounds(A, _want(name)[:1])
    leaf = 1 if name.startswith("dstar") else 2     # (leaf 1 carries the pendant cell of the undirected stars)
    assert (int(bound[0]), int(bound[leaf])) == STARS[name][1:], "the case does not sit where its name says"
    _assert_shells(name)


def test_shells_on_the_hub_graph_take_the_global_class_in_batches():
    A, _ = _graph("hub")
    shells = _want("hub")
    assert np.diff(A.indptr)[0] >= 2490 and all(np.median(np.diff(S.indptr)) > 2400 for S in shells[1:])
    for l in (1, 2):
        bound = R.key_bounds(A, shells[:l])
        big = np.minimum(bound[bound > WG_KEYS], A.shape[0])
        tables = 4 * np.sum(2 ** np.ceil(np.log2(2 * big)).astype(np.int64))
        print(f"hub graph, hop {l} -> {l + 1}: {np.count_nonzero(bound <= WAVE_KEYS)} wavefront rows, "
              f"{np.count_nonzero((bound > WAVE_KEYS) & (bound <= WG_KEYS))} workgroup rows, {big.size} global rows, {tables >> 20} MiB of tables")
        assert big.size > 0
    assert tables > 2 * GLOBAL_BATCH_BYTES      # the hop 2 -> 3: three batches at least
    _assert_shells("hub")


def test_every_shell_past_the_diameter_is_empty():
    _assert_shells("path40")
    got = _device("path40")
    assert [s[2][0] for s in got[:39]] == [2 * (40 - l) for l in range(1, 40)]
    for indptr, indices, stats in got[39:]:
        assert stats == (0, 0, 40) and not indptr.any() and indices.size == 0


# ---- 2. the aggregates -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _embedding(n, dtype):
    X = (np.random.default_rng(4).normal(size=(n, 64)) * 2.5 + 0.5).astype(dtype)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _ordered(name, layer, dtype, width=64):
    """The restatement for the first `width` columns: a column's sums do not depend on the others, so the first d columns of
    this are the restatement of X[:, :d]."""
    return R.ordered(_want(name)[layer - 1], _embedding(_graph(name)[0].shape[0], dtype)[:, :width])


def _device_aggregates(name, layers, X):
    A, _ = _graph(name)
    ctx = _ctx()
    out = {}
    ctx.hop_begin(A.indptr, A.indices, A.shape[0])
    try:
        for l in range(1, max(layers) + 1):
            if l > 1:
                ctx.hop_next()
            if l in layers:
                out[l] = (ctx.hop_aggregate(X, "mean"), ctx.hop_aggregate(X, "var"))
    finally:
        ctx.hop_end()
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name,layers", [("knn3000k15", (1, 2, 3)), ("hub", (1,))])
def test_aggregates_equal_the_ordered_restatement_bit_for_bit(name, layers, d, dtype):
    X = np.ascontiguousarray(_embedding(_graph(name)[0].shape[0], dtype)[:, :d])
    got = _device_aggregates(name, layers, X)
    for l in layers:
        mean, var = _ordered(name, l, dtype)
        assert got[l][0].dtype == np.float64 and got[l][0].shape == X.shape
        assert got[l][0].tobytes() == np.ascontiguousarray(mean[:, :d]).tobytes(), f"mean, shell {l}"
        assert got[l][1].tobytes() == np.ascontiguousarray(var[:, :d]).tobytes(), f"variance, shell {l}"


@pytest.mark.parametrize("d,dtype", [(16, np.float32), (17, np.float64)], ids=["16-f32", "17-f64"])
def test_aggregates_over_rows_of_2500_entries(d, dtype):
    """Shell 2 of the hub graph: every row is about 2500 entries long."""
    X = np.ascontiguousarray(_embedding(5000, dtype)[:, :d])
    mean, var = _ordered("hub", 2, dtype, d)
    got = _device_aggregates("hub", (2,), X)[2]
    assert got[0].tobytes() == mean.tobytes() and got[1].tobytes() == var.tobytes()


def test_an_empty_shell_gives_exact_zeros():
    X = _embedding(400, np.float64)[:, :3].copy()
    got = _device_aggregates("isolated", (1, 4), X)
    for l in (1, 4):
        for a in got[l]:
            assert a[123].tobytes() == np.zeros(3).tobytes()
    A = R.path(40)
    ctx = _ctx()
    ctx.hop_begin(A.indptr, A.indices, 40)
    try:
        for _ in range(44):
            stats = ctx.hop_next()
        assert stats == (0, 0, 40)
        for what in ("mean", "var"):
            assert ctx.hop_aggregate(_embedding(40, np.float32)[:, :17].copy(), what).tobytes() == np.zeros((40, 17)).tobytes()
    finally:
        ctx.hop_end()


def test_calls_out_of_order_and_bad_arrays_are_refused():
    from spatialcore_amd import _lib

    ctx = _ctx()
    ctx.hop_end()
    for call in (ctx.hop_next, ctx.hop_get, ctx.hop_times, lambda: ctx.hop_aggregate(np.zeros((3, 2)), "mean")):
        with pytest.raises(_lib.SpatialCoreHipError, match="no graph is resident"):
            call()
    with pytest.raises(ValueError, match="row 1: columns are not strictly ascending"):
        ctx.hop_begin(np.array([0, 1, 3, 3]), np.array([1, 2, 0]), 3)
    with pytest.raises(_lib.SpatialCoreHipError, match="no graph is resident"):
        ctx.hop_next()
    A = R.path(5)
    ctx.hop_begin(A.indptr, A.indices, 5)
    try:
        X = np.ones((5, 2))
        X[4, 1] = np.nan
        with pytest.raises(ValueError, match=r"X\[4\]\[1\] is not finite"):
            ctx.hop_aggregate(X, "mean")
        with pytest.raises(ValueError, match="unknown aggregation"):
            ctx.hop_aggregate(np.ones((5, 2)), "median")
        np.testing.assert_array_equal(ctx.hop_aggregate(np.arange(10.0).reshape(5, 2), "mean")[0], [2.0, 3.0])
        times = ctx.hop_times()
        assert set(times) == {"count", "fill", "sort", "aggregate"} and times["aggregate"] > 0 and times["count"] == 0
    finally:
        ctx.hop_end()


# ---- 3. the public function --------------------------------------------------------------------------------------------------------
def _adata(n=1500, d=5, seed=21, dtype=np.float64):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(size=(n, 2))
    ad = make_adata(xy, np.zeros((n, 2)))
    ad.obsm["X_pca"] = rng.normal(size=(n, d)).astype(dtype)
    return ad, xy


def test_columns_and_uns_of_the_default_call():
    from spatialcore_amd.spatial import aggregate_neighbors

    ad, xy = _adata()
    A = R.knn_union(xy, 6)
    out = aggregate_neighbors(ad, n_layers=3)
    assert out is ad and ad.obsm["X_cellcharter"].dtype == np.float64 and ad.obsm["X_cellcharter"].shape == (1500, 20)
    assert ad.obsm["X_cellcharter"].tobytes() == R.features(A, ad.obsm["X_pca"], [0, 1, 2, 3], ["mean"]).tobytes()
    shells = R.shells_textbook(A, 3)
    uns = ad.uns["X_cellcharter"]
    assert uns["layers"] == [0, 1, 2, 3] and uns["aggregations"] == ["mean"] and uns["n_features"] == 5
    assert uns["graph"] == {"source": "knn_union", "n_neighbors": 6, "stored_entries": int(A.nnz)}
    assert uns["shell_entries"] == [int(S.nnz) for S in shells]
    assert uns["shell_max"] == [int(np.diff(S.indptr).max()) for S in shells] and uns["shell_empty"] == [0, 0, 0]
    assert uns["params"]["use_rep"] == "X_pca" and uns["params"]["n_neighbors"] == 6
    last = ad.uns["spatialcore_metadata"]["operations"][-1]
    assert last["function"] == "aggregate_neighbors" and last["outputs"] == {"obsm": "X_cellcharter", "uns": "X_cellcharter"}


@pytest.mark.parametrize("layers,aggs,dtype", [([1, 3], "mean", np.float64), (2, ["mean", "var"], np.float32), ([3, 0, 2], ["var", "mean"], np.float64)],
                         ids=["layers-1-3", "mean-var-f32", "unordered-var-mean"])
def test_columns_of_chosen_layers_and_aggregations(layers, aggs, dtype):
    from spatialcore_amd.spatial import aggregate_neighbors

    ad, xy = _adata(dtype=dtype)
    aggregate_neighbors(ad, n_layers=layers, aggregations=aggs, out_key="agg")
    asked = list(range(layers + 1)) if isinstance(layers, int) else layers
    want = R.features(R.knn_union(xy, 6), ad.obsm["X_pca"], asked, [aggs] if isinstance(aggs, str) else aggs)
    assert ad.obsm["agg"].shape == want.shape and ad.obsm["agg"].tobytes() == want.tobytes()
    assert ad.uns["agg"]["layers"] == sorted(asked) and len(ad.uns["agg"]["shell_entries"]) == max(asked)


def test_sample_key_keeps_overlapping_slides_apart():
    from spatialcore_amd.spatial import aggregate_neighbors

    ad, xy = _adata(n=1200)
    slide = np.where(np.random.default_rng(5).uniform(size=1200) < 0.4, "s1", "s2")    # both cover the same unit square
    ad.obs["slide"] = slide
    aggregate_neighbors(ad, n_layers=2, aggregations=["mean", "var"], sample_key="slide")
    got = ad.obsm["X_cellcharter"]
    entries = 0
    for s in ("s1", "s2"):
        rows = np.flatnonzero(slide == s)
        alone = make_adata(xy[rows], np.zeros((rows.size, 2)))
        alone.obsm["X_pca"] = ad.obsm["X_pca"][rows]
        aggregate_neighbors(alone, n_layers=2, aggregations=["mean", "var"])
        assert got[rows].tobytes() == alone.obsm["X_cellcharter"].tobytes()
        entries += alone.uns["X_cellcharter"]["graph"]["stored_entries"]
        A = R.knn_union(xy[rows], 6)
        assert alone.obsm["X_cellcharter"].tobytes() == R.features(A, alone.obsm["X_pca"], [0, 1, 2], ["mean", "var"]).tobytes()
    assert ad.uns["X_cellcharter"]["graph"] == {"source": "knn_union within obs['slide']", "n_neighbors": 6, "stored_entries": entries}


def test_a_graph_from_obsp_and_copy():
    from spatialcore_amd.spatial import aggregate_neighbors

    ad, _ = _adata(n=500)
    G = R.directed(500, 4, 3).tolil()
    G.setdiag(2.0)                      # a diagonal and weights: both ignored
    ad.obsp["directed"] = sparse.csr_matrix(G) * 0.25
    before = (dict(ad.obsm), dict(ad.uns))
    out = aggregate_neighbors(ad, n_layers=[2, 1], aggregations="var", connectivity_key="directed", copy=True)
    assert out is not ad and set(ad.obsm) == set(before[0]) and set(ad.uns) == set(before[1])
    want = R.features(R.directed(500, 4, 3), ad.obsm["X_pca"], [1, 2], ["var"])
    assert out.obsm["X_cellcharter"].tobytes() == want.tobytes()
    assert out.uns["X_cellcharter"]["graph"] == {"source": "obsp['directed']", "n_neighbors": None, "stored_entries": int(R.directed(500, 4, 3).nnz)}
    with_matrix = aggregate_neighbors(ad, n_layers=[2, 1], aggregations="var", connectivity_key=ad.obsp["directed"], copy=True)
    assert with_matrix.obsm["X_cellcharter"].tobytes() == want.tobytes() and with_matrix.uns["X_cellcharter"]["graph"]["source"] == "matrix"


# ---- 4. the same bytes ---------------------------------------------------------------------------------------------------------------
_CHILD = """
import hashlib, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import hops_restated as R
from conftest import make_adata
from spatialcore_amd.spatial import aggregate_neighbors
for name, A in (("knn3000k15", R.knn_case("knn3000k15")[0]), ("hub", R.hub_graph())):
    n = A.shape[0]
    ad = make_adata(np.zeros((n, 2)), np.zeros((n, 2)))
    ad.obsm["X_pca"] = np.random.default_rng(4).normal(size=(n, 17)).astype(np.float32)
    aggregate_neighbors(ad, n_layers=3, aggregations=["mean", "var"], connectivity_key=A)
    print(name, hashlib.sha256(ad.obsm["X_cellcharter"].tobytes()).hexdigest(), ad.uns["X_cellcharter"]["shell_entries"])
"""


def _digests():
    from spatialcore_amd.spatial import aggregate_neighbors

    lines = []
    for name in ("knn3000k15", "hub"):
        A = _graph(name)[0]
        n = A.shape[0]
        ad = make_adata(np.zeros((n, 2)), np.zeros((n, 2)))
        ad.obsm["X_pca"] = np.random.default_rng(4).normal(size=(n, 17)).astype(np.float32)
        aggregate_neighbors(ad, n_layers=3, aggregations=["mean", "var"], connectivity_key=A)
        lines.append(f"{name} {hashlib.sha256(ad.obsm['X_cellcharter'].tobytes()).hexdigest()} {ad.uns['X_cellcharter']['shell_entries']}")
    return lines


def test_two_calls_and_a_child_on_four_hardware_queues_give_the_same_bytes(tmp_path):
    """A second call here, and a fresh child held to GPU_MAX_HW_QUEUES=4 (this process asked for 24)."""
    first = _digests()
    assert _digests() == first
    script = tmp_path / "hops_child.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    run = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert [line for line in run.stdout.splitlines() if line.startswith(("knn3000k15 ", "hub "))] == first


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
def test_domains_from_aggregated_features_end_to_end():
    """The recipe of hops_restated.domain_recipe, seed 0: k-means on the aggregated layers 1 .. 3 recovers the two domains
    (ARI >= 0.85; the restatement with sklearn's k-means gives 0.897, 0.912, 0.920 for the seeds 0 .. 2), the raw embedding
    does not (<= 0.17)."""
    from spatialcore_amd.spatial import aggregate_neighbors, identify_niches

    xy, X, domain = R.domain_recipe(0)
    ad = make_adata(xy, np.zeros((4000, 2)))
    ad.obsm["X_pca"] = X
    aggregate_neighbors(ad, n_layers=[1, 2, 3], n_neighbors=6)
    want = R.features(R.knn_union(xy, 6), X, [1, 2, 3], ["mean"])
    assert ad.obsm["X_cellcharter"].tobytes() == want.tobytes()
    identify_niches(ad, 2, neighborhood_key="X_cellcharter")
    restated = make_adata(xy, np.zeros((4000, 2)))
    restated.obsm["X_cellcharter"] = want
    identify_niches(restated, 2, neighborhood_key="X_cellcharter")
    assert np.array_equal(np.asarray(ad.obs["niche"].cat.codes), np.asarray(restated.obs["niche"].cat.codes))
    raw = make_adata(xy, np.zeros((4000, 2)))
    raw.obsm["X_pca"] = X
    identify_niches(raw, 2, neighborhood_key="X_pca")
    score, score_raw = R.ari(ad.obs["niche"].cat.codes, domain), R.ari(raw.obs["niche"].cat.codes, domain)
    print(f"ARI against the domain: aggregated {score:.3f}, raw embedding {score_raw:.3f}")
    assert score >= 0.85 and score_raw <= 0.17


def test_sixty_four_columns_go_through_neighbors_and_louvain():
    from spatialcore_amd.cluster import louvain
    from spatialcore_amd.neighbors import neighbors
    from spatialcore_amd.spatial import aggregate_neighbors

    xy, X, _ = R.domain_recipe(1, n=2000, d=16)
    ad = make_adata(xy, np.zeros((2000, 2)))
    ad.obsm["X_pca"] = X
    aggregate_neighbors(ad, n_layers=3)
    assert ad.obsm["X_cellcharter"].shape == (2000, 64)
    neighbors(ad, use_rep="X_cellcharter")
    louvain(ad, graph="connectivities")
    assert ad.obs["louvain"].nunique() >= 2
