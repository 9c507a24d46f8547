"""spatialcore_amd.annotation without a device: the restated definition against sklearn and against itself, the model
file, every argument error (raised before a device context exists), the host's vote / ensemble / optimiser, and the cap
the GPU end-to-end test leans on, from the reference alone."""
import logging
import os

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

import annotation_restated as R
from conftest import make_adata

END_TO_END = (777, 37, 5, 32)     # the shape the GPU end-to-end test trains and predicts on


def _model(n, G, T, seed, rng_seed=5):
    r = R.recipe(n, G, T, seed)
    keep = np.flatnonzero(np.diff(r["X"].tocsc().indptr) > 0)
    X = r["X"][:, keep]
    mean, scale = R.scaler(X)
    rng = np.random.default_rng(rng_seed)
    return r, keep, X, mean, scale, rng.normal(0, 0.7, size=(T, keep.size)), rng.normal(0, 1.0, size=T)


@pytest.fixture
def no_context(monkeypatch):
    from spatialcore_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was requested")

    monkeypatch.setattr(_lib, "default_context", boom)


@pytest.mark.parametrize("n,G,T,seed", R.SHAPES + R.WIDE_SHAPES)
def test_recipe_has_the_structure_the_tests_rely_on(n, G, T, seed):
    r, keep, X, mean, scale, _, _ = _model(n, G, T, seed)
    Z = R.dense_z(X, mean, scale)
    raw = (np.asarray(X.todense()) - mean) / scale
    assert 1 <= int((raw > R.CLIP).sum()) <= 3 and Z.max() == R.CLIP            # clipped entries, all in the rare gene
    assert np.all((raw > R.CLIP).sum(axis=0)[1:] == 0) and keep[0] == r["rare"]
    assert r["zero_gene"] not in keep and keep.size == G - 1                     # the all-zero gene leaves the features
    assert X[r["empty"]].nnz == 0 and X[r["full"]].nnz == keep.size              # the empty cell and the full cell
    assert np.bincount(r["labels"], minlength=T).min() == 5


@pytest.mark.parametrize("n,G,T,seed", R.SHAPES)
def test_dense_matches_sklearn_scaler_and_clip(n, G, T, seed):
    from sklearn.preprocessing import StandardScaler

    _, _, X, mean, scale, coef, b = _model(n, G, T, seed)
    Xd = np.asarray(X.todense())
    sk = StandardScaler().fit(Xd)
    np.testing.assert_allclose(mean, sk.mean_, rtol=1e-13, atol=0)
    np.testing.assert_allclose(scale, sk.scale_, rtol=1e-12, atol=0)
    Zs = np.minimum(sk.transform(Xd), 10.0)
    np.testing.assert_allclose(R.dense_z(X, mean, scale), Zs, rtol=0, atol=1e-11)
    np.testing.assert_allclose(R.dense_scores(X, coef, b, mean, scale), Zs @ coef.T + b, rtol=0, atol=1e-10)


def test_constant_feature_scales_by_one_as_sklearn():
    from sklearn.preprocessing import StandardScaler

    X = sparse.csr_matrix(np.array([[0.7, 1.0], [0.7, 0.0], [0.7, 2.0]]))
    mean, scale = R.scaler(X)
    assert scale[0] == 1.0 == StandardScaler().fit(X.toarray()).scale_[0]


@pytest.mark.parametrize("n,G,T,seed", R.SHAPES)
def test_identity_and_ordered_against_dense(n, G, T, seed):
    r, _, X, mean, scale, coef, b = _model(n, G, T, seed)
    z0, D = R.d_values(X, mean, scale)
    assert np.all(z0 <= 0)
    assert np.array_equal(D.indices, X.indices) and np.array_equal(D.indptr, X.indptr)      # nothing is densified
    Z = R.dense_z(X, mean, scale)
    assert np.max(np.abs(z0[None, :] + np.asarray(D.todense()) - Z)) <= 1e-12
    S, base = R.ordered_scores(X, coef, b, mean, scale)
    dense = R.dense_scores(X, coef, b, mean, scale)
    assert np.max(np.abs(S - dense)) <= 1e-12 * max(1.0, np.abs(dense).max()) * X.shape[1]
    assert np.array_equal(S[r["empty"]], base)                                             # the empty cell is the base


def test_confidences_follow_the_golden_reference():
    """The restatement against the reference's recorded results, and the structure of the matrices as they are FED: the
    float32 rounding (what the reference reads from obsm) and the float64 values themselves."""
    from conftest import load_golden

    g = load_golden("ref_annotation.npz")
    for case in g["cases"]:
        S = g[f"{case}_scores"]
        for wide, M in (("f32", S.astype(np.float32).astype(np.float64)), ("f64", S)):
            mine = R.confidences(M)
            for method in g["methods"]:
                dev = np.max(np.abs(g[f"{case}_{method}_{wide}"].astype(np.float64) - mine[method]))
                assert dev == g[f"{case}_{method}_{wide}_dev"], (case, method, wide)
                assert dev <= (3e-7 if wide == "f32" else 1e-15)
    sp, tiny = g["special_scores"], g["tiny_scores"]
    sp32, tiny32 = (M.astype(np.float32).astype(np.float64) for M in (sp, tiny))
    for M in (sp, sp32):
        assert np.ptp(M[0]) == 0 and (M[2] == M[2].max()).sum() == 3 and int(R.confidences(M)["argmax"][2]) == 0
        assert (M[3] < 0).all() and (M[4] < 0).all()
    assert 0 < np.ptp(sp[1]) < 1e-10 and np.ptp(sp32[1]) == 0        # float32 rounds that row to all equal ...
    for M in (tiny, tiny32):                                        # ... these rows keep their ranges in both forms
        rng, std = np.ptp(M, axis=1), np.std(M, axis=1)
        assert 0 < rng[0] < 1e-10 and 0 < std[0] < 1e-10             # both guards taken, away from 0
        assert rng[1] > 1e-10 and std[1] > 1e-10                     # neither guard, just above
        assert rng[2] > 1e-10 and 0 < std[2] < 1e-10                 # the std guard alone
        assert 0 < rng[3] < 1e-10 and 0 < std[3] < 1e-10 and (M[3] < 0).all()
        c = R.confidences(M)
        # the guards change the result: without them row 0 would give minmax 1 and a z-score of about 1.5
        assert c["minmax"][0] == rng[0] and abs(c["zscore"][0] - 0.5) < 1e-10 and c["minmax"][1] == 1.0
        assert abs(c["zscore"][2] - 0.5) < 1e-9 and c["minmax"][2] == 1.0
    assert g["two_scores"].shape[1] == 2


def test_model_round_trip_and_pickle_refusal(tmp_path):
    from spatialcore_amd.annotation import CellTypeModel

    rng = np.random.default_rng(3)
    m = CellTypeModel.from_arrays(["g2", "g0", "g7"], ["B", "T"], rng.normal(size=(2, 3)), rng.normal(size=2),
                                  np.abs(rng.normal(size=3)), 1 + np.abs(rng.normal(size=3)))
    path = m.write(tmp_path / "sub" / "m.npz")
    back = CellTypeModel.load(path)
    for k in CellTypeModel.__slots__:
        assert np.array_equal(getattr(m, k), getattr(back, k)) and getattr(back, k).dtype == getattr(m, k).dtype
    assert back.coef.dtype == np.float64 and list(back.cell_types) == ["B", "T"]
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(CellTypeModel.__slots__)
    pkl = tmp_path / "Immune_All_Low.pkl"
    pkl.write_bytes(b"\x80\x04not run")
    with pytest.raises(ValueError, match="never"):
        CellTypeModel.load(pkl)
    with pytest.raises(ValueError, match="npz"):
        m.write(tmp_path / "m.pkl")
    with pytest.raises(ValueError, match="shape"):
        CellTypeModel(["a", "b"], ["x", "y"], np.zeros((2, 3)), np.zeros(2), np.zeros(2), np.ones(2))
    with pytest.raises(ValueError, match="one row per cell type"):
        CellTypeModel(["a", "b"], ["x", "y"], np.zeros((1, 2)), np.zeros(1), np.zeros(2), np.ones(2))
    with pytest.raises(ValueError, match="scaler_scale"):
        CellTypeModel(["a", "b"], ["x", "y"], np.zeros((2, 2)), np.zeros(2), np.zeros(2), np.array([1.0, 0.0]))
    with pytest.raises(ValueError, match="2 to 256"):
        CellTypeModel(["a"], ["x"], np.zeros((1, 1)), np.zeros(1), np.zeros(1), np.ones(1))


def _labelled(n=40, G=6, seed=0, log1p=True):
    rng = np.random.default_rng(seed)
    C = sparse.csr_matrix(rng.poisson(1.0, size=(n, G)).astype(np.float64))
    ad = make_adata(rng.uniform(0, 10, (n, 2)), R.log1p_10k(C) if log1p else C)
    ad.obs["unified_cell_type"] = np.where(np.arange(n) % 2 == 0, "a", "b")
    return ad


def _tiny_model(G=6, extra=()):
    from spatialcore_amd.annotation import CellTypeModel

    names = [f"g{i}" for i in range(G)] + list(extra)
    rng = np.random.default_rng(1)
    return CellTypeModel(names, ["a", "b"], rng.normal(size=(2, len(names))), np.zeros(2), np.full(len(names), 0.5),
                         np.ones(len(names)))


def test_training_argument_errors_come_before_any_context(no_context, tmp_path):
    from spatialcore_amd.annotation import train_celltypist_model as train

    ad = _labelled()
    with pytest.raises(ValueError, match="Label column 'nope' not found. Available:"):
        train(ad, label_column="nope")
    with pytest.raises(NotImplementedError):
        train(ad, feature_selection=True)
    one = _labelled()
    one.obs["unified_cell_type"] = "a"
    with pytest.raises(ValueError, match="at least 2 cell types"):
        train(one)
    missing = _labelled()
    missing.obs.loc[missing.obs.index[3], "unified_cell_type"] = None
    with pytest.raises(ValueError, match="missing"):
        train(missing)
    for kw in ({"max_iter": 0}, {"max_iter": 2.5}, {"C": 0.0}, {"C": float("nan")}, {"tol": -1.0}, {"tol": "x"}):
        with pytest.raises(ValueError):
            train(ad, **kw)
    with pytest.raises(ValueError, match="never as a pickle"):
        train(ad, output_path=tmp_path / "model.pkl")
    with pytest.raises(ValueError, match="Genes not found"):
        train(ad, genes=["g0", "zz"])
    bad = _labelled()
    bad.X = bad.X * 3.7     # neither counts nor log1p(10k)
    with pytest.raises(ValueError, match="Cannot prepare data for CellTypist"):
        train(bad)
    neg = _labelled()
    neg.X = -neg.X
    with pytest.raises(ValueError, match="negative"):
        train(neg)


def test_annotation_argument_errors_come_before_any_context(no_context, tmp_path):
    from spatialcore_amd.annotation import annotate_celltypist as annotate

    ad, m = _labelled(), _tiny_model()
    with pytest.raises(ValueError, match="downloads nothing"):
        annotate(ad)
    with pytest.raises(ValueError, match="downloads nothing"):
        annotate(ad, tissue="liver", ensemble_mode=True)
    for bs in (0, -3, True, 2.5):
        with pytest.raises(ValueError, match="batch_size must be a positive integer or None"):
            annotate(ad, model=m, batch_size=bs)
    with pytest.raises(ValueError, match="batch_size requires majority_voting=False"):
        annotate(ad, model=m, batch_size=10, majority_voting=True, over_clustering="unified_cell_type")
    with pytest.raises(ValueError, match="majority_voting=True requires a valid cluster column"):
        annotate(ad, model=m, majority_voting=True)
    with pytest.raises(ValueError, match="majority_voting=True requires a valid cluster column"):
        annotate(ad, model=m, majority_voting=True, over_clustering="nope")
    with pytest.raises(ValueError, match="Unknown confidence method"):
        annotate(ad, model=m, confidence_transform="sigmoid")
    with pytest.raises(ValueError, match="No models passed gene overlap threshold"):
        annotate(ad, model=_tiny_model(1, extra=[f"x{i}" for i in range(9)]))
    with pytest.raises(ValueError, match="never"):
        annotate(ad, custom_model_path=tmp_path / "model.pkl")
    with pytest.raises(ValueError, match="not both"):
        annotate(ad, custom_model_path=tmp_path / "m.npz", model=m)
    with pytest.raises(ValueError, match="CellTypeModel or a path"):
        annotate(ad, model=[m, 3])
    bad = _labelled()
    bad.X = bad.X * 3.7
    with pytest.raises(ValueError, match="Cannot prepare data for CellTypist"):
        annotate(bad, model=m)


def test_transform_confidence_argument_errors_come_before_any_context(no_context):
    from spatialcore_amd.annotation import transform_confidence

    with pytest.raises(ValueError, match="Expected 2D array"):
        transform_confidence(np.zeros(5))
    with pytest.raises(ValueError, match="Expected at least 2 cell types, got 1"):
        transform_confidence(np.zeros((5, 1)))
    with pytest.raises(ValueError, match="Unknown confidence method: sigmoid"):
        transform_confidence(np.zeros((5, 3)), method="sigmoid")
    with pytest.raises(ValueError, match="NaN"):
        transform_confidence(np.array([[0.0, np.nan]]))
    with pytest.raises(ValueError, match="at most 256"):
        transform_confidence(np.zeros((2, 257)))


def test_input_state_and_modes():
    from spatialcore_amd.annotation import _input

    rng = np.random.default_rng(4)
    C = sparse.csr_matrix(rng.poisson(0.8, size=(60, 12)).astype(np.float32))
    X = R.log1p_10k(C)
    cols = np.arange(12)
    assert _input.prepare(C, cols)[1] == "counts" and _input.prepare(C.astype(np.int32), cols[:5])[1] == "counts"
    assert _input.prepare(X, cols)[1] == "log1p" and _input.prepare(X, cols[2:9])[1] == "log1p_renorm"
    assert _input.prepare(X.toarray(), cols)[1] == "log1p"
    Xc, _ = _input.prepare(C, cols[3:])
    assert Xc.dtype == np.float32 and Xc.has_sorted_indices and Xc.shape == (60, 9) and C.shape == (60, 12)
    cpm = X.copy()
    cpm.data = np.log1p(np.expm1(cpm.data) * 100.0)
    with pytest.raises(ValueError, match="Cannot prepare data for CellTypist"):
        _input.prepare(cpm, cols)


def test_majority_vote_and_ensemble_against_pandas():
    from spatialcore_amd.annotation.annotate import ensemble, majority_vote

    rng = np.random.default_rng(8)
    names = np.array(["B", "NK", "T", "mast"])
    codes = rng.integers(0, 4, 500)
    clusters = rng.integers(0, 9, 500).astype(str)
    codes[clusters == "3"] = np.resize([2, 1], (clusters == "3").sum() // 2 * 2 + 2)[: (clusters == "3").sum()]   # a tie
    tab = pd.crosstab(pd.Series(clusters, name="c"), pd.Series(names[codes], name="l"))
    for min_prop in (0.0, 0.3, 0.6):
        share = tab.max(axis=1) / tab.sum(axis=1)
        want = tab.idxmax(axis=1).where(share >= min_prop, "Heterogeneous")      # idxmax: the first column = sorted order
        got = majority_vote(codes, clusters, 4, min_prop)
        got = np.where(got < 0, "Heterogeneous", names[np.maximum(got, 0)])
        assert np.array_equal(got, want.loc[clusters].to_numpy())
    t3 = tab.loc["3"]
    if (clusters == "3").sum() % 2 == 0:
        assert t3["NK"] == t3["T"] == t3.max() and set(majority_vote(codes, clusters, 4, 0.0)[clusters == "3"]) == {1}
    conf = [rng.uniform(size=50), rng.uniform(size=50), rng.uniform(size=50)]
    conf[1][:10] = conf[0][:10] = 0.99          # ties: the first model wins
    conf[2][:10] *= 0.9
    frame = pd.DataFrame({k: c for k, c in enumerate(conf)})
    assert np.array_equal(ensemble(conf), frame.idxmax(axis=1).to_numpy()) and not ensemble(conf)[:10].any()


def test_no_cpu_fallback_without_gpu():
    from spatialcore_amd import _lib
    from spatialcore_amd.annotation import annotate_celltypist, train_celltypist_model, transform_confidence

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.SpatialCoreHipError):
        transform_confidence(np.zeros((3, 4)))
    with pytest.raises(_lib.SpatialCoreHipError):
        annotate_celltypist(_labelled(), model=_tiny_model())
    with pytest.raises(_lib.SpatialCoreHipError):
        train_celltypist_model(_labelled())


@pytest.mark.parametrize("balance", [True, False])
@pytest.mark.parametrize("n,G,T,seed", R.SHAPES[:2])
def test_host_optimiser_meets_its_stopping_rule_and_the_reference_bound(n, G, T, seed, balance):
    """annotation/training.py's lockstep L-BFGS on the numpy restatement of the device passes."""
    from spatialcore_amd.annotation.training import fit

    tol = 1e-10
    ref, r = R.reference_model(n, G, T, seed, balance), R.recipe(n, G, T, seed)
    s, Gk = ref["s"], ref["X"].shape[1]
    res = fit(R.NumpyProblem(ref["X"], r["labels"], s, T), T, Gk, float(s.sum()), 1.0, tol, 100)
    g = R.gradient(ref["Z"], r["labels"], s, res["coef"], res["intercept"], 1.0)
    assert np.abs(g).max() / s.sum() <= 2e-10 and res["converged"].all() and res["n_iter"].max() <= 60
    assert np.abs(R.gradient(ref["Z"], r["labels"], s, ref["coef"], ref["intercept"], 1.0)).max() / s.sum() <= 1e-11
    bound = R.coefficient_bound(ref["Z"], s, ref["coef"], ref["intercept"], 1.0, tol)
    diff = np.maximum(np.abs(res["coef"] - ref["coef"]).max(axis=1), np.abs(res["intercept"] - ref["intercept"]))
    assert np.all(diff <= bound), (diff / bound).max()
    few = fit(R.NumpyProblem(ref["X"], r["labels"], s, T), T, Gk, float(s.sum()), 1.0, tol, 3)
    assert not few["converged"].any() and few["n_iter"].max() == 3


def held_out_margins(balance=True):
    """Reference scores of the held-out cells of the end-to-end shape, the cells whose top-two margin exceeds the
    coefficient bound x (|z_i|_1 + 1), and the reference labels: shared with the GPU test."""
    n, G, T, seed = END_TO_END
    ref = R.reference_model(n, G, T, seed, balance)
    held = R.recipe(n, G, T, seed, held_out=True)
    Z = R.dense_z(held["X"][:, ref["keep"]], ref["mean"], ref["scale"])
    S = Z @ ref["coef"].T + ref["intercept"]
    bound = R.coefficient_bound(ref["Z"], ref["s"], ref["coef"], ref["intercept"], 1.0, 1e-10).max()
    top = np.sort(S, axis=1)
    decided = (top[:, -1] - top[:, -2]) > bound * (np.abs(Z).sum(axis=1) + 1.0)
    return held, ref, S, decided


def test_end_to_end_cap_from_the_reference_alone():
    _, _, S, decided = held_out_margins()
    assert (~decided).mean() <= 0.001
    assert len(set(np.argmax(S, axis=1).tolist())) >= 3


def test_ignored_keywords_are_logged_once(no_context, caplog):
    """The SGD keywords are accepted; the INFO line is emitted before the device is asked for."""
    from spatialcore_amd.annotation import train_celltypist_model

    lg = logging.getLogger("spatialcore_amd")
    lg.addHandler(caplog.handler)
    try:
        with caplog.at_level(logging.INFO, logger="spatialcore_amd"):
            with pytest.raises(AssertionError, match="device context"):
                train_celltypist_model(_labelled(), use_SGD=False, mini_batch=False, epochs=3, batch_size=7, batch_number=2, n_jobs=4)
    finally:
        lg.removeHandler(caplog.handler)
    assert sum("recorded and ignored" in rec.getMessage() for rec in caplog.records) == 1
