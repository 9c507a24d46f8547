"""The inputs of tests/test_gpu_annotation_edges.py without a device: each case is what it says it is, and the restatement
the GPU tests lean on agrees with plain numpy within a quarter of the tolerance its GPU test uses, so that the GPU
tolerances have headroom that comes from the reference alone.

 - ``R.ordered_scores`` against ``R.dense_scores``: at most 0.25e-12 of the terms' size (the GPU training passes: 1e-12);
 - ``R.confidences`` (the epilogue's order) against numpy's own sums: the largest deviation of a case is at most a
   quarter of the case's ``R.ulp_tolerance`` (its largest entry); ``raw`` and ``minmax`` hold no sum and no exp and are
   equal.  The comparison is per case, not per cell, and cannot be per cell: ``R.ulp_tolerance`` measures what one ulp of
   exp moves, which is nothing (tolerance 0, the GPU test then asks for the same bits) at 74 to 122 of 129 z-scores,
   while another summation order moves a value by one or two ulp at up to 9 cells of a case (measured: largest
   deviation 2.2e-16 for zscore and for softmax; case tolerances 6.7e-16 to 3.6e-15).  The device adds in the
   restatement's order, so that cell-wise demand is the right one for the device and the wrong one for numpy's sum."""
import numpy as np
import pytest

import annotation_restated as R
import lane_group_inputs as L

ALL_T = L.SWEEP_T + L.BLOCK_T


def _check_ladder(facts, w, G, zero_gene):
    n = facts["n"]
    assert facts["lengths"] == L.ladder_lengths(w, G) and facts["longest"] == G - 1
    for key, factor in (("over_w", 1), ("over_2w", 2), ("over_3w", 3)):
        assert facts[key] == L.expected_over(w, G, n, factor) and facts[key] >= 2, key
    assert facts["over_3w"] >= 2 * (n // len(L.ladder_pattern(w, G)))          # 3 w + 3 and the full row, every repeat
    assert facts["entries_after_a_full_block"] == [0, 1, 2, 3, 4]             # every scalar tail after a full first fetch
    assert facts["zero_columns"] == [zero_gene] and facts["remainder"] == 1
    assert n >= 2 * facts["rows_per_workgroup"] + 1
    if G == 257:
        assert facts["last_gene_stored"] >= 1 and zero_gene == 0
    if w <= 32:
        assert facts["wavefronts_with_an_empty_row_beside_the_third_block"] >= 1
        assert 2 * facts["wavefronts_with_unequal_trips"] >= facts["wavefronts"]


@pytest.mark.parametrize("T", sorted(set(ALL_T + L.PASSES_T + L.F32_T)))
def test_ladder_has_the_structure_the_gpu_tests_rely_on(T):
    X = L.annotation_counts(T)
    w, G = R.lanes(T), X.shape[1]
    facts = L.ladder_facts(X, w, L.zero_gene_of(T, G))
    print(f"T={T}: {facts}")
    _check_ladder(facts, w, G, L.zero_gene_of(T, G))
    assert w == (64 if T > 32 else {3: 4, 4: 4, 7: 8, 9: 16, 16: 16, 17: 32, 32: 32}[T])
    if T == 129:
        assert G == 257


def test_zero_gene_sits_at_both_ends_over_the_cases():
    ends = {L.zero_gene_of(T, L.annotation_genes(T)) == 0 for T in L.PASSES_T}
    assert ends == {True, False}                                   # column 0 in some training cases, column G - 1 in others


def test_tall_case_has_the_stated_columns():
    X, labels = L.tall_annotation_case()
    facts = L.tall_facts(X, 64, X.shape[1] - 1)
    print(f"tall annotation case: {facts}")
    assert facts["columns"] == [511, 512, 513, 1029] and facts["chunks_of_the_longest"] == 3
    assert (facts["n"], facts["G"]) == (1029, 70) and facts["remainder"] == 1 and facts["cell_chunks"] == 2
    assert facts["zero_columns"] == [69] and labels.shape == (1029,) and labels.max() < L.TALL_T


@pytest.mark.parametrize("T,tie", L.PREDICTIONS)
def test_ordered_scores_against_dense(T, tie):
    c = L.prediction_case(T, tie)
    S = c["want"]["scores64"]
    dense = R.dense_scores(c["X"], c["coef"], c["intercept"], c["mean"], c["scale"])
    reach = np.abs(R.dense_z(c["X"], c["mean"], c["scale"])) @ np.abs(c["coef"]).T + np.abs(c["intercept"])
    rel = float(np.max(np.abs(S - dense) / reach))
    print(f"T={T} tie={tie}: ordered against dense scores, largest deviation {rel:.3g} of the terms' size")
    assert rel <= 0.25e-12
    assert c["empty"].size >= 2 and np.all(S[c["empty"]] == c["want"]["base"])
    # the fp64 sums are visible through the raw confidence only where expit is not saturated: most rows that take a second
    # fetch keep their winning score below 7 (expit' = 9e-4 there, against 1e-11 at 25)
    best = S.max(axis=1)[np.diff(c["X"].indptr) > R.lanes(T)]
    print(f"T={T} tie={tie}: winning scores of the rows past one fetch {best.min():.2f} .. {best.max():.2f}, median {np.median(best):.2f}")
    assert np.mean(np.abs(best) < 7.0) >= 0.5
    # the tie construction: identical bits in the tied classes, which win often enough; the first of them is the label
    tied = c["tied"]
    for t in tied[1:]:
        assert np.array_equal(S[:, t], S[:, tied[0]])
    wins = S[:, tied[0]] == S.max(axis=1)
    assert wins.sum() >= 10 and (~wins).sum() >= 10 and np.all(c["want"]["labels"][wins] == tied[0])
    assert np.all((S == S.max(axis=1)[:, None]).sum(axis=1) == np.where(wins, len(tied), 1))      # no tie but the built one
    assert tied == ([0, T - 1] if T < 65 else sorted({0, 64, T - 1}) if tie == "first" else sorted({64 * ((T - 1) // 64), T - 1}))


def _confidence_headroom(name, F, want, tol):
    plain = L.plain_confidences(F)
    assert np.array_equal(plain["raw"], want["raw"]) and np.array_equal(plain["minmax"], want["minmax"])
    assert np.array_equal(plain["argmax"], want["argmax"])
    for key in ("zscore", "softmax"):
        d = np.abs(plain[key] - want[key])
        over = int((d > 0.25 * tol[key]).sum())
        print(f"{name} {key}: largest deviation {d.max():.3g} ({np.max(d / np.spacing(want[key])):.0f} ulp), the case's tolerance "
              f"{tol[key].max():.3g}; {over} of {d.size} cells above a quarter of their own tolerance, which is 0 at "
              f"{int((tol[key] == 0).sum())} cells")
        assert d.max() <= 0.25 * tol[key].max(), key


@pytest.mark.parametrize("T", ALL_T)
def test_confidences_against_plain_sums_on_the_predicted_rows(T):
    c = L.prediction_case(T)
    F = c["want"]["scores"].astype(np.float64)
    _confidence_headroom(f"T={T} prediction", F, c["want"], c["tol"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", L.TRANSFORM_T)
def test_confidences_against_plain_sums_on_the_transform_matrices(T, dtype):
    S, want, tol = L.transform_case(T, dtype)
    assert S.dtype == dtype and S.shape == (201, T)
    F = S.astype(np.float64)
    assert np.ptp(F[0]) == 0 and want["minmax"][0] == 0.0 and want["zscore"][0] == 0.5         # both guards
    assert want["argmax"][1] == T - 1 and want["argmax"][2] == 64 and want["argmax"][3] == 64   # the first of two maxima
    assert F[3, 64] == F[3, T - 1]
    _confidence_headroom(f"T={T} {np.dtype(dtype).name} matrix", F, want, tol)


@pytest.mark.parametrize("T", L.F32_T)
def test_float32_cases_round_their_values_and_keep_their_counts(T):
    c64, c32 = L.prediction_case(T), L.prediction_case(T, f32=True)
    assert np.array_equal(c32["X"].data, c64["X"].data.astype(np.float32).astype(np.float64))
    assert (c32["X"].data != c64["X"].data).mean() > 0.9                     # the rounding is visible in nearly every value
    C = c64["counts"]
    assert np.array_equal(C.data.astype(np.float32).astype(np.float64), C.data)   # counts are exact in float32
    assert R.lanes(T) == (8 if T == 7 else 64)
