"""GPU: sc_domains_2d and make_spatial_domains against the numpy / scipy restatement (tests/domains_restated.py).

Component ids are integers and compared exactly.  A cell is left out of the label comparison only if its restated,
UNCLAMPED clearance is within 1e-6 d of s (the restatement is rerun with the cap s + 2e-6 d to see that side of s
too); the band may hold at most 1 % of the cells in U.  On inputs A, B and C it holds no cell: the closest cell is
5.4e-3, 2.4e-2 and 4.9e-2 from s, so nothing is left out.

The clearance tolerance is measured, not guessed: the restatement runs on A - C in float64 and in np.longdouble; the
largest difference between the two, 6.2e-14 (4.6e-14, 5.3e-14, 6.2e-14), is the formula's own rounding noise on these
inputs, and the device gets ten times that, 6.2e-13 -- two correct fp64 evaluation orders can differ by a few times one
order's error.  The figure is taken again at run time by the ``noise`` fixture, which also asserts that it has not
moved by more than a factor of two from the one written here.
"""
import logging

import numpy as np
import pytest

from conftest import make_adata
from domains_restated import assign, clearance, components, make_input, reduce_and_number

pytestmark = pytest.mark.gpu

NOISE_WRITTEN = 6.2e-14


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


@pytest.fixture(scope="module")
def restated():
    """Per input: coordinates, target mask, d, s, and the restatement with ALL cells as queries (computed once)."""
    out = {}
    for name in "ABC":
        xy, target, d, m = make_input(name)
        s = d - m
        T = xy[target]
        comp_t = components(T, d)
        clear = clearance(T, xy, d, s)
        _, comp_q, _ = assign(T, xy, d, s, comp_t=comp_t, clear=clear)
        wide = clearance(T, xy, d, s + 2e-6 * d)                       # the clearance seen from both sides of s
        band = (clear >= 0) & (np.abs(wide - s) < 1e-6 * d)
        long = clearance(T, xy, d, s, dtype=np.longdouble)
        in_u = clear >= 0
        assert ((long >= 0) == in_u).all()
        out[name] = dict(xy=xy, target=target, d=d, m=m, s=s, comp_t=comp_t, comp_q=comp_q, clear=clear, band=band,
                         noise=float(np.abs(clear[in_u] - long[in_u]).max()))
    return out


@pytest.fixture(scope="module")
def noise(restated):
    worst = max(r["noise"] for r in restated.values())
    print(f"float64 against longdouble restatement: {[r['noise'] for r in restated.values()]}, worst {worst:.3e}")
    assert NOISE_WRITTEN / 2 <= worst <= NOISE_WRITTEN * 2
    return worst


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_components_labels_and_clearance_equal_the_restatement(restated, noise, name):
    r = restated[name]
    xy, T, d, s = r["xy"], r["xy"][r["target"]], r["d"], r["s"]
    comp_t, comp_q, clear = _ctx().domains(T, xy, d, s)
    assert comp_t.dtype == np.int32 and comp_q.dtype == np.int32 and clear.dtype == np.float64
    np.testing.assert_array_equal(comp_t, r["comp_t"])
    in_u = r["clear"] >= 0
    band = r["band"]
    print(f"input {name}: {band.sum()} of {in_u.sum()} cells of U in the band")
    assert band.sum() <= 0.01 * in_u.sum()
    np.testing.assert_array_equal(comp_q[~band], r["comp_q"][~band])
    np.testing.assert_array_equal(comp_q[r["target"]], comp_t)           # every target is in its own region
    np.testing.assert_array_equal(clear < 0, ~in_u)
    np.testing.assert_array_equal(clear[~in_u], -1.0)
    np.testing.assert_array_equal(comp_q[~in_u], -1)
    err = np.abs(clear - r["clear"]).max()
    print(f"input {name}: max |device - restated clearance| = {err:.3e}, bound {10 * noise:.3e}")
    assert err <= 10 * noise
    assert ((comp_q >= 0) == (clear >= s))[~band].all()


def test_input_a_has_the_stated_shape(restated):
    r = restated["A"]
    t = r["target"]
    sizes = np.bincount(r["comp_t"])[np.unique(r["comp_t"])]
    assert (t.sum(), sizes.size, (sizes <= 10).sum()) == (294, 63, 55)
    assert ((r["comp_q"] >= 0) & ~t).sum() == 237 and ((r["clear"] >= 0) & (r["clear"] < r["s"])).sum() == 581
    sizes_b = np.bincount(restated["B"]["comp_t"])
    assert (restated["B"]["target"].sum(), (sizes_b > 0).sum(), sizes_b.max()) == (448, 8, 372)
    assert np.unique(restated["C"]["comp_t"]).size == 111


def _spiral(n, step, arm):
    """n points at arc-length spacing ``step`` along r = arm theta / (2 pi), from the second turn outwards."""
    a = arm / (2 * np.pi)
    theta = np.linspace(2 * np.pi, 2 * np.pi + 2 * np.sqrt(n * step / a) + 10, 400000)
    arc = a / 2 * (theta * np.sqrt(1 + theta * theta) + np.arcsinh(theta))
    th = np.interp(arc[0] + step * np.arange(n), arc, theta)
    assert th[-1] < theta[-1]
    return np.stack([a * th * np.cos(th), a * th * np.sin(th)], axis=1)


def test_snake_of_3000_targets_is_one_component_run_to_run():
    d = 1.0
    chain = _spiral(3000, 1.9 * d, 6.0 * d)                              # neighbours 1.9 d apart, arms 6 d apart
    far = np.stack([200.0 + 10.0 * d * np.arange(20), np.full(20, 500.0)], axis=1)
    T = np.concatenate([chain, far])
    T = T[np.random.default_rng(8).permutation(T.shape[0])]
    want = components(T, d)
    sizes = np.bincount(want)
    assert (sizes > 0).sum() == 21 and sizes.max() == 3000
    first, _, _ = _ctx().domains(T, None, d, 0.5 * d)
    second, _, _ = _ctx().domains(T, None, d, 0.5 * d)
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, first)


def test_lattice_ties_join_at_exactly_two_d():
    """40 x 40 integer lattice, every other row a target row, 2 d = 1.0 exactly: horizontal neighbours sit at
    dist2 == (2d)^2 and are joined (closed), rows two apart are not.  Components only."""
    from spatialcore_amd.spatial import make_spatial_domains

    g = np.arange(40, dtype=np.float64)
    xy = np.stack(np.meshgrid(g, g, indexing="xy"), axis=-1).reshape(-1, 2)      # cell = 40 * row + column
    row = np.arange(1600) // 40
    target = row % 2 == 0
    comp, _, _ = _ctx().domains(xy[target], None, 0.5, 0.25)
    np.testing.assert_array_equal(comp, (np.arange(800) // 40) * 40)            # a row's first target names it
    np.testing.assert_array_equal(comp, components(xy[target], 0.5))
    ad = make_adata(xy, np.zeros((1600, 1)), labels=np.where(target, "T", "S"))
    make_spatial_domains(ad, "cell_type == 'T'", cell_dist_um=0.5, shrink_margin_um=0.25, assign_all_cells=False)
    col = ad.obs["spatial_domain"]
    assert col.dtype == object and col[~target].isna().all()
    # twenty domains of 40 cells each: the tie goes to the smaller component id, i.e. the lower row
    assert col[target].tolist() == [f"T_{r // 2 + 1}" for r in row[target]]


def test_duplicates_outside_queries_one_target_and_no_queries(noise):
    rng = np.random.default_rng(12)
    base = rng.uniform(0, 120, (150, 2))
    T = np.concatenate([base, base[:60], base[:20], base[:20]])                 # up to four targets on one spot
    T = T[rng.permutation(T.shape[0])]
    d, m = 9.0, 3.0
    s = d - m
    lo, hi = T.min(axis=0), T.max(axis=0)
    outside = np.array([[lo[0] - 3 * d, 60.0], [hi[0] + 3 * d, 60.0], [60.0, lo[1] - 3 * d], [60.0, hi[1] + 3 * d],
                        [lo[0] - 50 * d, lo[1] - 50 * d], [hi[0] + 1e6, hi[1] + 1e6]])
    Q = np.concatenate([rng.uniform(-5, 125, (600, 2)), base[:5], base[100:105], outside])
    comp_t, comp_q, clear = _ctx().domains(T, Q, d, s)
    want_t, want_q, want_c = assign(T, Q, d, s)
    wide = clearance(T, Q, d, s + 2e-6 * d)
    band = (want_c >= 0) & (np.abs(wide - s) < 1e-6 * d)
    assert band.sum() <= 0.01 * (want_c >= 0).sum()
    np.testing.assert_array_equal(comp_t, want_t)
    np.testing.assert_array_equal(comp_q[~band], want_q[~band])
    assert np.abs(clear - want_c).max() <= 10 * noise
    np.testing.assert_array_equal(clear[600:610], s)                             # a query on a target's spot
    assert (comp_q[600:610] >= 0).all()
    np.testing.assert_array_equal(clear[-6:], -1.0)
    np.testing.assert_array_equal(comp_q[-6:], -1)
    # one target: a disc; clearance is d - r capped at s
    one = np.array([[3.0, 4.0]])
    q1 = np.array([[3.0, 4.0], [3.0, 4.0 + 2.0], [3.0 + 5.0, 4.0], [3.0, 4.0 - 9.0], [3.0 - 9.5, 4.0]])
    ct, cq, cl = _ctx().domains(one, q1, d, s)
    assert ct.tolist() == [0] and cq.tolist() == [0, 0, -1, -1, -1]
    np.testing.assert_allclose(cl, [s, s, 4.0, 0.0, -1.0], atol=1e-14)
    # no queries: components only
    ct, cq, cl = _ctx().domains(T, None, d, s)
    np.testing.assert_array_equal(ct, want_t)
    assert cq.size == 0 and cl.size == 0
    for bad in (dict(cell_dist=0.0, shrink=0.0), dict(cell_dist=np.nan, shrink=1.0), dict(cell_dist=5.0, shrink=5.0),
                dict(cell_dist=5.0, shrink=-1.0)):
        with pytest.raises(ValueError, match="cell_dist|shrink"):
            _ctx().domains(T, Q, **bad)


class _Collect(logging.Handler):
    def __init__(self):
        super().__init__(logging.DEBUG)
        self.records = []

    def emit(self, record):
        self.records.append(record)


def _run_a(restated, **kw):
    from spatialcore_amd.spatial import make_spatial_domains

    r = restated["A"]
    ad = make_adata(r["xy"], np.zeros((r["xy"].shape[0], 1)), labels=np.where(r["target"], "Tumor", "Other"))
    args = dict(filter_expression="cell_type == 'Tumor'", cell_dist_um=r["d"], shrink_margin_um=r["m"])
    args.update(kw)
    return ad, make_spatial_domains(ad, **args)


def _expected_names(r, min_target, min_total=None, all_cells=True, prefix="Tumor"):
    t = r["target"]
    comp_q = r["comp_q"][~t] if all_cells else np.zeros(0, dtype=np.int32)
    rank_t, rank_q = reduce_and_number(r["comp_t"], comp_q, min_target, min_total)
    rank = np.zeros(t.size, dtype=np.int64)
    rank[t] = rank_t
    if all_cells:
        rank[~t] = rank_q
    return rank, [f"{prefix}_{k}" if k else np.nan for k in rank]


def _same_column(col, names):
    got = col.tolist()
    assert len(got) == len(names)
    assert all((g == w) or (g != g and w != w) for g, w in zip(got, names))


def test_public_api_on_input_a(restated):
    from spatialcore_amd.spatial import calculate_domain_distances, get_domain_summary

    r = restated["A"]
    assert not r["band"].any()
    ad, out = _run_a(restated)
    assert out is ad and "_filter" not in ad.obs.columns
    rank, names = _expected_names(r, 10)
    assert rank.max() == 8
    _same_column(ad.obs["spatial_domain"], names)
    assert ad.obs["spatial_domain"].dtype == object
    counts = np.bincount(rank)[1:]
    assert (np.diff(counts) <= 0).all() and ad.obs["spatial_domain"].value_counts()["Tumor_1"] == counts[0]
    # the provenance entry
    entry = ad.uns["spatialcore_metadata"]["operations"][-1]
    assert entry["function"] == "make_spatial_domains"
    assert set(entry["parameters"]) == {"filter_expression", "cell_dist_um", "cell_dist_um_user_provided", "platform",
                                        "platform_user_provided", "shrink_margin_um", "domain_prefix",
                                        "min_target_cells_domain", "min_total_cells_domain", "output_column",
                                        "assign_all_cells", "domain_expansion_warn_ratio"}
    assert set(entry["outputs"]) == {"obs", "n_domains", "n_cells_assigned", "n_target_cells", "domains"}
    assert entry["outputs"]["n_domains"] == 8 and entry["outputs"]["n_target_cells"] == 294
    assert entry["outputs"]["n_cells_assigned"] == int((rank > 0).sum())
    assert entry["parameters"]["domain_prefix"] == "Tumor" and entry["parameters"]["cell_dist_um_user_provided"] is True
    # the summary and the distances take the column as it is
    df = get_domain_summary(ad)
    assert df["domain"].iloc[0] == "Tumor_1" and df["n_cells"].tolist() == sorted(counts.tolist(), reverse=True)
    calculate_domain_distances(ad, "spatial_domain", "spatial_domain", distance_metric="centroid", output_mode="matrix")
    assert sorted(ad.uns["domain_distances"]["source_domains"]) == [f"Tumor_{k}" for k in range(1, 9)]


def test_public_api_thresholds_are_closed(restated):
    r = restated["A"]
    t = r["target"]
    n_target = np.bincount(r["comp_t"], minlength=t.sum())
    sizes = np.sort(n_target[n_target > 0])
    v = int(sizes[-3])                                   # a size that exists: components of exactly v targets go
    assert (n_target == v).any() and (n_target > v).any()
    ad, _ = _run_a(restated, min_target_cells_domain=v, domain_prefix="D", output_column="dom")
    rank, names = _expected_names(r, v, prefix="D")
    assert rank.max() == (n_target > v).sum()
    _same_column(ad.obs["dom"], names)
    # ... and the same for the total
    n_total = n_target + np.bincount(r["comp_q"][~t][r["comp_q"][~t] >= 0], minlength=t.sum())
    kept = n_total[n_target > 10]
    w = int(np.sort(kept)[2])
    ad, _ = _run_a(restated, min_total_cells_domain=w)
    rank, names = _expected_names(r, 10, w)
    assert rank.max() == (kept > w).sum() < kept.size
    _same_column(ad.obs["spatial_domain"], names)


def test_public_api_targets_only_copy_and_warning(restated):
    r = restated["A"]
    t = r["target"]
    ad, out = _run_a(restated, assign_all_cells=False, copy=True)
    assert out is not ad and "spatial_domain" not in ad.obs.columns and "spatialcore_metadata" not in ad.uns
    col = out.obs["spatial_domain"]
    assert col[~t].isna().all()
    _, names = _expected_names(r, 10, all_cells=False)
    _same_column(col, names)
    # the expansion warning: 223 cells assigned on 294 targets is a ratio of 0.8
    log = logging.getLogger("spatialcore_amd.spatial.domains")
    seen = _Collect()
    log.addHandler(seen)
    try:
        _run_a(restated, domain_expansion_warn_ratio=0.5)
        warned = [x for x in seen.records if x.levelno == logging.WARNING]
        assert len(warned) == 1 and "Domain expansion ratio 0.8x exceeds threshold (0.5x)" in warned[0].getMessage()
        seen.records.clear()
        _run_a(restated, domain_expansion_warn_ratio=1.0)
        assert not [x for x in seen.records if x.levelno == logging.WARNING]
        assert any("Created 8 domains, assigned 223/2,000 cells" in x.getMessage() for x in seen.records)
    finally:
        log.removeHandler(seen)
