"""CPU-only: the host logic of calculate_domain_distances (label codes, segmented reductions, table
assembly) against the reference's golden output, with the three device calls replaced by the stand-in of
tests/distance_restated.py (the product has no CPU path; the GPU tests run the same goldens through HIP)."""
import numpy as np
import pandas as pd
import pytest

from conftest import load_golden
from distance_restated import ScipyGeometry as _ScipyGeometry


def _domain_adata(g):
    from spatialcore_amd import SimpleAnnData

    coords = g["coords"]
    obs = pd.DataFrame({"dom_a": [x if x else None for x in g["dom_a"]], "dom_b": [x if x else None for x in g["dom_b"]]},
                       index=pd.RangeIndex(len(coords)).astype(str))
    return SimpleAnnData(np.zeros((len(coords), 1)), obs=obs, var_names=["g0"], obsm={"spatial": coords})


CASES = {
    "min_both": dict(source_domain_column="dom_a", target_domain_column="dom_b", distance_metric="minimum", output_mode="both"),
    "min_matrix": dict(source_domain_column="dom_a", target_domain_column="dom_b", distance_metric="minimum", output_mode="matrix"),
    "mean_both": dict(source_domain_column="dom_a", target_domain_column="dom_b", distance_metric="mean", output_mode="both"),
    "centroid_both": dict(source_domain_column="dom_a", target_domain_column="dom_b", distance_metric="centroid", output_mode="both"),
    "self_min": dict(source_domain_column="dom_a", target_domain_column="dom_a", distance_metric="minimum", output_mode="both"),
    "self_centroid": dict(source_domain_column="dom_a", target_domain_column="dom_a", distance_metric="centroid", output_mode="both"),
    "subset_min": dict(source_domain_column="dom_a", target_domain_column="dom_b", source_domain_subset=["B_1", "B_3"],
                       target_domain_subset=["T_2"], distance_metric="minimum", output_mode="both"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_domain_distance_host_logic_matches_reference_golden(monkeypatch, name):
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import calculate_domain_distances, get_distance_matrix

    monkeypatch.setattr(_lib, "default_context", lambda device=0: _ScipyGeometry())
    g = load_golden("ref_distance.npz")
    kw = CASES[name]
    ad = _domain_adata(g)
    calculate_domain_distances(ad, **kw)
    m = get_distance_matrix(ad)
    assert list(m.index) == list(g[f"{name}_rows"]) and list(m.columns) == list(g[f"{name}_cols"])
    np.testing.assert_allclose(m.values.astype(float), g[f"{name}_matrix"], rtol=1e-12)
    np.testing.assert_allclose([ad.uns["domain_distances"]["summary_statistics"][k] for k in
                                ("min_distance", "max_distance", "mean_distance", "median_distance")],
                               g[f"{name}_summary"], rtol=1e-12)
    if kw["output_mode"] in ("cell", "both"):
        np.testing.assert_allclose(ad.obs["distance_to_target"].values.astype(float), g[f"{name}_dist"], rtol=1e-13,
                                   equal_nan=True)
        near = np.array([x if isinstance(x, str) else "" for x in ad.obs["nearest_target_domain"].values])
        np.testing.assert_array_equal(near, g[f"{name}_nearest"])


def test_domain_distance_rejects_3d_coordinates(monkeypatch):
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial import calculate_domain_distances

    monkeypatch.setattr(_lib, "default_context", lambda device=0: _ScipyGeometry())
    g = load_golden("ref_distance.npz")
    ad = _domain_adata(g)
    ad.obsm["spatial"] = np.concatenate([ad.obsm["spatial"], np.zeros((ad.n_obs, 1))], axis=1)
    with pytest.raises(ValueError, match="only 2-D coordinates"):
        calculate_domain_distances(ad, "dom_a", "dom_b")
