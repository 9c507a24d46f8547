"""sc_annotate.hip past one lane-group fetch (inputs: tests/lane_group_inputs.py, proved fair by
tests/test_cpu_annotation_lanes.py): every lane-group width tp = 4 .. 64 and every class-block count NB = 1 .. 4 on rows of
0 to 3 tp + 3 and of all stored entries, full and one-class last blocks, AN_TMAX, ties inside a lane across blocks, the
float32 upload, gene columns of several chunks at NB = 4, nine sort-key bits.

Prediction is compared bit for bit with the restatement in the device's order (float32 scores, labels, raw, minmax; the
exp-bearing keys within R.ulp_tolerance), the training passes with plain numpy within the bounds of
``_passes_against_numpy``.  No tolerance is new."""
import numpy as np
import pytest

import annotation_restated as R
import lane_group_inputs as L
from test_gpu_annotation import CONF_KEYS, _annotate, _check_prediction, _passes_against_numpy

pytestmark = pytest.mark.gpu

assert CONF_KEYS == L.CONF_KEYS


def _model(c, T):
    from spatialcore_amd.annotation import CellTypeModel

    return CellTypeModel([f"g{j}" for j in c["keep"]], [f"type{t:03d}" for t in range(T)], c["coef"], c["intercept"],
                         c["mean"], c["scale"])


def _cells(c, what="X"):
    from spatialcore_amd import SimpleAnnData

    return SimpleAnnData(c[what], var_names=[f"g{j}" for j in c["keep"]])


def _predict(c, what="X", mode="log1p", dtype=np.float64):
    from spatialcore_amd import _lib

    X = c[what].astype(dtype)
    assert X.data.dtype == dtype
    return _lib.default_context(0).annot_predict(X.indptr, X.indices, X.data, mode, c["coef"], c["intercept"], c["mean"],
                                                 c["scale"])


def _check_library_result(res, c, T):
    want, tol = c["want"], c["tol"]
    assert np.array_equal(res["scores"], want["scores"]) and np.array_equal(res["labels"], want["labels"])
    assert np.array_equal(res["raw"], want["raw"]) and np.array_equal(res["minmax"], want["minmax"])     # no exp in these
    for key in CONF_KEYS:
        d = np.abs(res[key] - want[key])
        print(f"T={T} {key}: largest deviation {d.max():.3g}, tolerance at that cell {tol[key][np.argmax(d)]:.3g}")
        assert np.all(d <= tol[key]), key
    assert c["empty"].size >= 2
    assert np.array_equal(res["scores"][c["empty"]], np.tile(want["base"].astype(np.float32), (c["empty"].size, 1)))


@pytest.mark.parametrize("T,tie", L.PREDICTIONS)
def test_prediction_on_the_ladder_is_the_ordered_restatement(T, tie):
    c = L.prediction_case(T, tie)
    model = _model(c, T)
    ad = _annotate(_cells(c), model=model)
    _check_prediction(ad, model, c["want"], c["tol"], T)
    assert ad.uns["spatialcore_metadata"]["operations"][-1]["parameters"]["input_state"] == "log1p"
    res = _predict(c)
    _check_library_result(res, c, T)
    # the tied classes hold the same bits; where they win, the smallest of them is the label
    S, first = c["want"]["scores64"], c["tied"][0]
    wins = S[:, first] == S.max(axis=1)
    assert wins.sum() >= 10 and np.all(res["labels"][wins] == first)
    for t in c["tied"][1:]:
        assert np.array_equal(res["scores"][:, t], res["scores"][:, first])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", L.TRANSFORM_T)
def test_transform_confidence_past_one_block_of_classes(T, dtype):
    from spatialcore_amd import _lib
    from spatialcore_amd.annotation import transform_confidence

    S, want, tol = L.transform_case(T, dtype)
    res = _lib.default_context(0).annot_transform(S)
    assert np.array_equal(res["raw"], want["raw"]) and np.array_equal(res["minmax"], want["minmax"])
    for key in ("raw", "zscore", "softmax", "minmax"):
        d = np.abs(res[key] - want[key])
        print(f"T={T} {np.dtype(dtype).name} {key}: largest deviation {d.max():.3g}, tolerance at that cell {tol[key][np.argmax(d)]:.3g}")
        assert np.all(d <= tol[key]), key
        assert np.array_equal(transform_confidence(S, method=key), res[key])
    assert res["zscore"][0] == 0.5 and res["minmax"][0] == 0.0 and res["raw"][0] == 1.25      # the all-equal row: both guards
    assert res["raw"][1] == float(S[1, T - 1]) and res["raw"][2] == float(S[2, 64]) and res["raw"][3] == float(S[3, 64])


@pytest.mark.parametrize("T", L.F32_T)
def test_float32_input_is_widened_exactly(T):
    from spatialcore_amd import _lib

    c64, c32 = L.prediction_case(T), L.prediction_case(T, f32=True)
    # log1p values: the float32 upload gives the restatement on the rounded values, with the rounded values' own model
    _check_library_result(_predict(c32, dtype=np.float32), c32, T)
    # counts are exact in float32: the same bits as the float64 counts run
    a, b = _predict(c64, "counts", "counts", np.float32), _predict(c64, "counts", "counts", np.float64)
    for key in ("scores", "labels") + CONF_KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert np.array_equal(b["labels"], c64["want"]["labels"])
    # the scaler of the training set-up
    ctx = _lib.default_context(0)
    X32 = c32["X"].astype(np.float32)
    labels, s = np.arange(X32.shape[0], dtype=np.int32) % T, np.ones(X32.shape[0])
    got = []
    for X in (X32, X32.astype(np.float64)):
        try:
            got.append(ctx.annot_train_begin(X.indptr, X.indices, X.data, X.shape[1], "log1p", T, labels, s))
        finally:
            ctx.annot_train_end()
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    np.testing.assert_allclose(got[0][0], c32["mean"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(got[0][1], c32["scale"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("T", L.PASSES_T)
def test_training_passes_on_the_ladder(T):
    X, labels = L.passes_case(T)
    _passes_against_numpy(X, labels, T, 1200 + T)


def test_training_passes_with_chunked_columns_at_four_class_blocks():
    X, labels = L.tall_annotation_case()
    first = _passes_against_numpy(X, labels, L.TALL_T, 75)
    again = _passes_against_numpy(X, labels, L.TALL_T, 75)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


def test_two_predictions_at_four_class_blocks_give_identical_bytes():
    c = L.prediction_case(193)
    a, b = _predict(c), _predict(c)
    for key in ("scores", "labels") + CONF_KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key
