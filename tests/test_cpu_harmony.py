"""spatialcore_amd.integration without a device: the properties of the restated algorithm (tests/harmony_restated.py), its two
textbook counterparts, the quality figures of the recipes, the argument errors of harmony_integrate, the exported surface
and the sanitizer run of the host checks.

The quality figures (harmony_restated.RECIPE_FIGURES) are those of the restatement started from sklearn's KMeans on the unit rows, the start
the device replays; tests/test_gpu_harmony.py takes its thresholds from them, never from the device's output."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import harmony_restated as H
from conftest import make_adata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c[0]: c for c in H.CASES}

def _state(name, rounds=2):
    Z, batch, B, Y, nb, sigma, theta, lamb = H.case_inputs(BY_NAME[name])
    h = H.Harmony(Z, batch, B, Y, nb, sigma, theta, lamb)
    h.cluster(rounds, -1.0)
    return h


# ---- 1. the restated algorithm ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n17", "n1201", "b64", "pair", "theta0"])
def test_rows_of_r_sum_to_one_and_the_tables_hold_its_mass(name):
    h = _state(name)
    np.testing.assert_allclose(h.R.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(h.O.sum(axis=(0, 2)), h.R.sum(axis=0), rtol=1e-13)
    assert h.O.shape == (h.nb, h.K, h.B) and np.all(h.O >= 0)


def test_block_membership_and_the_device_order():
    assert H.n_blocks(17, 0.05) == 17 and H.n_blocks(20, 0.05) == 20 and H.n_blocks(21, 0.05) == 20 and H.n_blocks(10, 1.0) == 1
    batch = np.array([1, 0, 1, 0, 0, 1, 1])
    # 3 blocks: {0, 3, 6}, {1, 4}, {2, 5}; inside a block by batch, then by cell
    np.testing.assert_array_equal(H.device_order(7, 3, batch), [3, 0, 6, 1, 4, 2, 5])


@pytest.mark.parametrize("name", ["n1201", "pair", "b64", "f32", "theta0"])
def test_closed_form_correction_equals_the_dense_textbook_form(name):
    h = _state(name)
    W, Zcorr = H.correct_closed(h.Z, h.R, h._tables()[0], h.batch, h.B, h.lamb)
    Wd, Zd = H.correct_dense(h.Z, h.R, h.batch, h.B, h.lamb)
    assert np.max(np.abs(Zcorr - Zd)) <= 1e-12 * np.max(np.abs(Zd))
    assert np.max(np.abs(W - Wd)) <= 1e-12 * max(np.max(np.abs(Wd)), 1.0)


@pytest.mark.parametrize("name", ["n17", "n21", "n1201", "pair", "sorted"])
def test_block_update_without_subtraction_equals_subtract_and_re_add(name):
    Z, batch, B, Y, nb, sigma, theta, lamb = H.case_inputs(BY_NAME[name])
    h = H.Harmony(Z, batch, B, Y, nb, sigma, theta, lamb)
    h.cluster(1, -1.0)
    start = h.R.copy()
    h.round()                                   # Y, dist and S move first, then the blocks from `start`
    R, O = H.update_subtract(h.S, start, h.batch, h.B, h.nb, h.theta)
    assert np.max(np.abs(R - h.R)) <= 1e-12
    assert np.max(np.abs(O - h._tables()[0])) <= 1e-12 * np.max(O)


def test_row_minimum_shift_changes_nothing_at_sigma_0_1_and_keeps_rows_finite_at_1e_3():
    Z, batch, B, Y, nb, *_ = H.case_inputs(BY_NAME["sigma1e-3"])
    Zc, Yc = H.unit_rows(Z), H.unit_rows(Y)
    _, S = H.soft_assign(Zc, Yc, 0.1)
    _, S0 = H.soft_assign(Zc, Yc, 0.1, shift=False)
    assert np.max(np.abs(S / S.sum(1, keepdims=True) - S0 / S0.sum(1, keepdims=True))) <= 1e-13
    _, S = H.soft_assign(Zc, Yc, 1e-3)
    with np.errstate(invalid="ignore", divide="ignore"):
        _, S0 = H.soft_assign(Zc, Yc, 1e-3, shift=False)
        plain = S0 / S0.sum(1, keepdims=True)
    assert not np.all(np.isfinite(plain))       # the recipe does underflow whole rows without the shift
    R = S / S.sum(1, keepdims=True)
    assert np.all(np.isfinite(R)) and np.all(S.max(axis=1) == 1.0)
    np.testing.assert_allclose(R.sum(axis=1), 1.0, rtol=0, atol=1e-14)


def test_a_cluster_whose_mass_is_in_one_batch_stays_solvable():
    Z, batch, _ = H.mixture((40, 40), 4, 2, 5)
    R = np.zeros((80, 2))
    R[:, 0] = batch == 0                        # cluster 0 only in batch 0, cluster 1 only in batch 1
    R[:, 1] = batch == 1
    O = R.T @ np.eye(2)[batch]
    for lamb in (1.0, 1e-3):
        W, Zcorr = H.correct_closed(Z, R, O, batch, 2, lamb)
        Wd, Zd = H.correct_dense(Z, R, batch, 2, lamb)
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(Zcorr))
        assert np.max(np.abs(Zcorr - Zd)) <= 1e-9 * np.max(np.abs(Zd))     # the dense system's condition grows as 1 / lamb
    # a cluster without any mass corrects nothing
    R[:, 1], R[:, 0] = 0.0, 1.0
    W, Zcorr = H.correct_closed(Z, R, R.T @ np.eye(2)[batch], batch, 2, 1.0)
    assert np.all(W[1] == 0.0) and np.all(np.isfinite(Zcorr))


def test_objective_falls_over_the_rounds_and_the_stop_rule_is_the_window_of_three():
    Z, batch, B, Y, nb, sigma, theta, lamb = H.case_inputs(BY_NAME["n1201"])
    h = H.Harmony(Z, batch, B, Y, nb, sigma, theta, lamb)
    full = h.cluster(20, -1.0)
    assert full.size == 20 and full[-1] < full[0] < h.__class__(Z, batch, B, Y, nb, sigma, theta, lamb).objective
    h = H.Harmony(Z, batch, B, Y, nb, sigma, theta, lamb)
    some = h.cluster(20, 1e-3)
    np.testing.assert_array_equal(some, full[:some.size])
    r = some.size - 1
    assert 4 <= r < 19
    old, new = some[r - 1] + some[r - 2] + some[r - 3], some[r] + some[r - 1] + some[r - 2]
    assert abs(old - new) / abs(old) < 1e-3


# ---- 2. the recipes' quality figures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r[0] for r in H.RECIPES])
def test_recipe_figures_and_chance(name):
    from sklearn.cluster import KMeans

    sizes, K = [(r[1], r[2]) for r in H.RECIPES if r[0] == name][0]
    Z, batch, types = H.recipe(name)
    Y = KMeans(n_clusters=K, n_init=10, max_iter=25, random_state=0).fit(H.unit_rows(Z)).cluster_centers_
    Zcorr, objectives, converged = H.restated_integrate(Z, batch, len(sizes), Y)
    before, after = H.neighbour_shares(Z, batch, types), H.neighbour_shares(Zcorr, batch, types)
    want = H.RECIPE_FIGURES[name]
    chance = float(np.sum((np.array(sizes) / sum(sizes)) ** 2))
    print(f"{name}: same-batch {before[0]:.4f} -> {after[0]:.4f} (chance {chance:.4f}), same-type {before[1]:.4f} -> {after[1]:.4f}, "
          f"{len(objectives)} outer rounds, converged={converged}")
    assert abs(chance - want[2]) < 1e-12
    assert abs(before[0] - want[0]) < 1e-3 and abs(after[0] - want[1]) < 1e-3 and abs(after[1] - want[3]) < 1e-3
    assert abs(after[0] - chance) <= 0.05 and before[0] - chance > 0.4       # the recipe is worth keeping
    assert (len(objectives), converged) == want[4:]


# ---- 3. the public call's arguments --------------------------------------------------------------------------------------------------
def _adata(Z, batch, **obsm):
    ad = make_adata(np.zeros((Z.shape[0], 2)), np.zeros((Z.shape[0], 1)))
    ad.obsm["X_pca"] = Z
    ad.obs["slide"] = batch
    for k, v in obsm.items():
        ad.obsm[k] = v
    return ad


def test_argument_errors_are_raised_before_the_device():
    from spatialcore_amd.integration import harmony_integrate as hi

    Z, batch, _ = H.mixture((30, 30), 5, 2, 3)
    ad = _adata(Z, np.array(["a", "b"])[batch])
    with pytest.raises(ValueError, match="key='nope' is not a column"):
        hi(ad, "nope")
    with pytest.raises(ValueError, match="several keys at once are not supported"):
        hi(ad, ["slide", "slide"])
    with pytest.raises(ValueError, match="has 1 batch"):
        hi(_adata(Z, np.array(["a"] * 60)), "slide")
    with pytest.raises(ValueError, match="batch 'c' .* has 1 cell; every batch needs at least 2"):
        hi(_adata(Z, np.array(["a", "b"] * 29 + ["a", "c"])), "slide")
    with pytest.raises(ValueError, match="has missing values"):
        hi(_adata(Z, np.array([1.0, np.nan] * 30)), "slide")
    for bad in (0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="lamb must be a finite number > 0"):
            hi(ad, "slide", lamb=bad)
        with pytest.raises(ValueError, match="sigma must be a finite number > 0"):
            hi(ad, "slide", sigma=bad)
    for bad in (-0.5, float("nan"), "2", None):
        with pytest.raises(ValueError, match="theta must be a finite number >= 0"):
            hi(ad, "slide", theta=bad)
    for bad in (1, 0, 61, 129, 2.5, True):
        with pytest.raises(ValueError, match="nclust"):
            hi(ad, "slide", nclust=bad)
    for bad in (0, 1.5, 1e-4, -0.05):
        with pytest.raises(ValueError, match="block_size"):
            hi(ad, "slide", block_size=bad)
    for name in ("max_iter_harmony", "max_iter_kmeans", "n_init"):
        with pytest.raises(ValueError, match=f"{name} must be an integer >= 1"):
            hi(ad, "slide", **{name: 0})
    with pytest.raises(ValueError, match="epsilon_cluster must be a number"):
        hi(ad, "slide", epsilon_cluster=float("nan"))
    with pytest.raises(ValueError, match="basis='X_other' is not an entry of adata.obsm"):
        hi(ad, "slide", basis="X_other")
    with pytest.raises(ValueError, match="adjusted_basis must be a non-empty string"):
        hi(ad, "slide", adjusted_basis="")
    with pytest.raises(ValueError, match="has 65 features"):
        hi(_adata(Z, batch, wide=np.ones((60, 65))), "slide", basis="wide")
    with pytest.raises(ValueError, match="must be a 2-D float32 or float64 array"):
        hi(_adata(Z, batch, ints=np.ones((60, 3), dtype=np.int64)), "slide", basis="ints")
    nan = Z.copy()
    nan[59, 4] = np.inf
    with pytest.raises(ValueError, match="contains NaN or infinite values"):
        hi(_adata(nan, batch), "slide")
    zero = Z.copy()
    zero[[3, 17]] = 0.0
    with pytest.raises(ValueError, match=r"has 2 row\(s\) that are all zero"):
        hi(_adata(zero, batch), "slide")
    assert "X_pca_harmony" not in ad.obsm and "harmony" not in ad.uns              # nothing was written


def test_defaults_are_harmonypys():
    import inspect

    from spatialcore_amd.integration import harmony
    from spatialcore_amd.integration import harmony_integrate as hi

    p = inspect.signature(hi).parameters
    want = dict(basis="X_pca", adjusted_basis="X_pca_harmony", theta=2.0, lamb=1.0, sigma=0.1, nclust=None, max_iter_harmony=10,
                max_iter_kmeans=20, epsilon_cluster=1e-5, epsilon_harmony=1e-4, block_size=0.05, n_init=10, random_state=0)
    assert {k: p[k].default for k in want} == want
    assert [harmony.default_nclust(n) for n in (10, 59, 300, 1200, 10**6)] == [2, 2, 10, 40, 100]
    assert harmony.n_blocks(17, 0.05) == 17 and harmony.n_blocks(1201, 0.05) == 20
    Z, _, _ = H.mixture((30, 30), 5, 2, 3)
    assert harmony.unit_rows(Z.astype(np.float32)).tobytes() == H.unit_rows(Z.astype(np.float32)).tobytes()
    for word in ("several keys", "tau", "automatic ``lamb``", "reference_values", "NOT pinned"):
        assert word in hi.__doc__


def test_hvg_and_harmony_share_one_batch_helper():
    from spatialcore_amd import _batches
    from spatialcore_amd.integration import harmony
    from spatialcore_amd.preprocessing import hvg

    assert hvg.batch_groups is _batches.batch_groups is harmony.batch_groups
    ad = _adata(np.ones((5, 2)), np.array(["b", "a", "b", "a", "b"]))
    groups = _batches.batch_groups(ad, "slide")
    assert [g[0] for g in groups] == ["a", "b"] and [g[1].tolist() for g in groups] == [[1, 3], [0, 2, 4]]


# ---- 4. the surface ----------------------------------------------------------------------------------------------------------------
def test_ctypes_surface_and_all():
    import spatialcore_amd
    from spatialcore_amd import _lib, integration

    assert integration.__all__ == ["harmony_integrate"] and callable(integration.harmony_integrate)
    assert "integration" in spatialcore_amd.__all__ and spatialcore_amd.integration is integration
    lib = _lib.load_library()
    for name in ("sc_harmony_begin", "sc_harmony_cluster", "sc_harmony_correct", "sc_harmony_get", "sc_harmony_end"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and hasattr(_lib.Context, name[3:])
    assert len(_lib.SYMBOLS["sc_harmony_begin"]) == 14
    header = open(os.path.join(ROOT, "include", "spatialcore_hip.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define SC_HARMONY_(\w+) (\d+)", header)}
    assert {k.lower(): v for k, v in codes.items()} == {k.lower(): v for k, v in _lib.HARMONY_ARRAYS.items()}
    # the entry points refuse on the host, before any HIP call: no context, no device
    rc = lib.sc_harmony_correct(None)
    assert rc == _lib.SC_ERR_INVALID and b"sc_harmony_correct: null pointer" in lib.sc_last_error()
    obj = ctypes.c_double(0.0)
    z = np.ones((4, 2))
    rc = lib.sc_harmony_begin(None, z.ctypes.data_as(ctypes.c_void_p), _lib.SC_F64, 4, 2, None, 2, None, 2, 2, 0.1, 2.0, 1.0,
                              ctypes.byref(obj))
    assert rc == _lib.SC_ERR_INVALID and b"sc_harmony_begin: null pointer" in lib.sc_last_error()
    makefile = open(os.path.join(ROOT, "spatialcore_amd", "csrc", "Makefile")).read()
    assert "sc_harmony.hip" in makefile.split("SRCS =")[1].split("\n")[0] and "asan_harmony:" in makefile


def test_host_checks_pass_under_the_sanitizers():
    """`make asan_harmony`: tests/harmony_host_checks.cpp (its own main, nothing preloaded) against the AddressSanitizer +
    UBSan objects of the library.  Every call in it is refused before its first HIP call: no device is touched."""
    csrc = os.path.join(ROOT, "spatialcore_amd", "csrc")
    if shutil.which("make") is None or not os.access(csrc, os.W_OK):
        pytest.skip("make is missing or the source tree cannot be written to: the sanitizer objects cannot be built here")
    jobs = str(max(1, min(16, os.cpu_count() or 1)))
    objects = subprocess.run(["make", "-C", csrc, f"-j{jobs}", "asan_build/sc_harmony.o", "asan_build/sc_api.o"],
                             capture_output=True, text=True)
    if objects.returncode != 0:
        pytest.skip("the sanitizer objects cannot be built here: " + objects.stderr[-300:])
    run = subprocess.run(["make", "-C", csrc, f"-j{jobs}", "asan_harmony"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "harmony host checks ok" in run.stdout and "FAIL" not in run.stdout
