"""spatialcore_amd.integration on the device: what is bit-equal to the restatement (tests/harmony_restated.py), every array at
every step within the measured tolerance of it, the edges, the same bytes run to run and under 4 or 24 hardware queues, the
public call, and the quality of the result on the recipes.

Cases (harmony_restated.CASES) are the smallest at which the kernels can go wrong; each names its edge there, against
sc_harmony.hip's slices and tiles of 128 cells, 4 x 4 thread tiles and strided blocks.

Tolerances.  MEASURED_* is the largest |device - restated| / max |restated| per array over every case and every checkpoint of
harmony_restated.walk() (after begin, after 1 and 5 clustering rounds, after the correction, after 3 outer rounds of 5), both
sides started from the same centres with negative epsilons, as scripts/harmony_probe.py --tolerances measured it on an MI355X
(profiles/harmony_1m.json: "tolerances").  The tests assert ten times each and never more than 1e-9.  Every figure is below
1e-10.  The largest, R at sigma = 1e-3, is the last-place difference of dist (1e-16 of values near 1) divided by sigma before
exp, carried through 15 rounds; the same case without that factor 1000 sits at 5e-15.

"sorted" and "interleaved" hold the same cells, batch by batch and in a random order.  Their blocks (cell mod n_blocks) hold
different cells, so their results differ by more than rounding; each is compared with the restatement of its own order."""
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import harmony_restated as H
from conftest import make_adata

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c[0]: c for c in H.CASES}
MEASURED_R = 4.2e-13
MEASURED_Y = 1.8e-14
MEASURED_O = 7.0e-14
MEASURED_W = 9.1e-14
MEASURED_ZCORR = 1.2e-14
MEASURED_OBJECTIVE = 5.8e-14
CAP = 1e-9
TOL = {"R": MEASURED_R, "Y": MEASURED_Y, "O": MEASURED_O, "W": MEASURED_W, "Zcorr": MEASURED_ZCORR, "objective": MEASURED_OBJECTIVE}
TOL = {a: min(10.0 * v, CAP) for a, v in TOL.items()}


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


@functools.lru_cache(maxsize=None)
def _device(name):
    return H.device_walk(_ctx(), BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _restated(name):
    return H.restated_walk(BY_NAME[name])


# ---- 1. bit-equal ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in H.CASES])
def test_unit_rows_block_membership_and_sort_are_bit_equal(name):
    Z, batch, B, Y, nb, sigma, theta, lamb = H.case_inputs(BY_NAME[name])
    ctx = _ctx()
    try:
        ctx.harmony_begin(Z, batch, B, Y, nb, sigma, theta, lamb)
        Zc, order, Yc, O = ctx.harmony_get("Zc"), ctx.harmony_get("order"), ctx.harmony_get("Y"), ctx.harmony_get("O")
        Zcorr, W = ctx.harmony_get("Zcorr"), ctx.harmony_get("W")
    finally:
        ctx.harmony_end()
    assert Zc.tobytes() == H.unit_rows(Z).tobytes()
    assert Yc.tobytes() == H.unit_rows(Y).tobytes()
    np.testing.assert_array_equal(order, H.device_order(Z.shape[0], nb, batch))
    assert Zcorr.tobytes() == Z.astype(np.float64).tobytes() and not W.any()          # before the first correction
    # the membership as the tables show it: a (block, batch) segment without a cell holds no mass, every other one some
    cells = np.zeros((nb, B), dtype=np.int64)
    np.add.at(cells, (np.arange(Z.shape[0]) % nb, batch), 1)
    np.testing.assert_array_equal(O.sum(axis=1) > 0, cells > 0)
    np.testing.assert_allclose(O.sum(axis=1), cells, rtol=1e-13)


# ---- 2. every array at every step, every edge ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in H.CASES])
def test_every_step_is_within_ten_times_the_measured_distance_of_the_restatement(name):
    got, want = _device(name), _restated(name)
    diff = H.relative_differences(got, want)
    for a in H.ARRAYS + ("objective",):
        worst = max((v, cp) for (cp, b), v in diff.items() if b == a)
        print(f"{name} {a}: {worst[0]:.2e} at {worst[1]} (asserted {TOL[a]:.1e})")
    for (cp, a), v in diff.items():
        assert np.all(np.isfinite(got[cp][a])), (cp, a)
        assert v <= TOL[a], (name, cp, a, v)
    for cp in H.CHECKPOINTS:
        np.testing.assert_allclose(got[cp]["R"].sum(axis=1), 1.0, rtol=0, atol=1e-13)
        np.testing.assert_allclose(got[cp]["O"].sum(axis=(0, 2)), got[cp]["R"].sum(axis=0), rtol=1e-12)


def test_no_penalty_still_corrects_and_a_small_sigma_keeps_every_row_finite():
    got = _device("theta0")
    assert np.abs(got["outer3"]["W"]).max() > 1e-3 and np.abs(got["outer3"]["Zcorr"] - got["begin"]["Zcorr"]).max() > 1e-3
    got = _device("sigma1e-3")
    for cp in H.CHECKPOINTS:
        assert all(np.all(np.isfinite(got[cp][a])) for a in H.ARRAYS)
    Z, batch, B, Y, nb, sigma, *_ = H.case_inputs(BY_NAME["sigma1e-3"])
    with np.errstate(invalid="ignore", divide="ignore"):
        _, S0 = H.soft_assign(H.unit_rows(Z), H.unit_rows(Y), sigma, shift=False)
    assert (S0.sum(axis=1) == 0).any()          # without the shift whole rows underflow on this input


def test_the_stop_rule_returns_the_rounds_done():
    Z, batch, B, Y, nb, sigma, theta, lamb = H.case_inputs(BY_NAME["n1201"])
    ctx = _ctx()
    try:
        ctx.harmony_begin(Z, batch, B, Y, nb, sigma, theta, lamb)
        full = ctx.harmony_cluster(20, -1.0)
        ctx.harmony_begin(Z, batch, B, Y, nb, sigma, theta, lamb)
        some = ctx.harmony_cluster(20, 1e-3)
    finally:
        ctx.harmony_end()
    want = H.Harmony(Z, batch, B, Y, nb, sigma, theta, lamb).cluster(20, 1e-3)
    assert full.size == 20 and some.size == want.size < 20
    assert some.tobytes() == full[:some.size].tobytes()
    np.testing.assert_allclose(some, want, rtol=TOL["objective"])


# ---- 3. the same bytes -------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import harmony_restated as H
from spatialcore_amd import _lib
ctx = _lib.default_context(0)
out = {{}}
for case in H.CASES:
    if case[0] in {names!r}:
        w = H.device_walk(ctx, case)
        for cp in H.CHECKPOINTS:
            for a in H.ARRAYS:
                out[case[0] + "/" + cp + "/" + a] = w[cp][a]
            out[case[0] + "/" + cp + "/objective"] = np.float64(w[cp]["objective"])
np.savez(sys.argv[1], **out)
"""


def test_two_calls_and_children_on_4_and_24_hardware_queues_give_the_same_bytes(tmp_path):
    names = ["n1201", "d64-k128", "f32"]
    ctx = _ctx()
    for name in names:
        again = H.device_walk(ctx, BY_NAME[name])
        for cp in H.CHECKPOINTS:
            for a in H.ARRAYS:
                assert again[cp][a].tobytes() == _device(name)[cp][a].tobytes(), (name, cp, a)
            assert again[cp]["objective"] == _device(name)[cp]["objective"]
    script = tmp_path / "harmony_child.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), names=names))
    for queues in ("4", "24"):
        env = dict(os.environ, GPU_MAX_HW_QUEUES=queues)
        path = tmp_path / f"child{queues}.npz"
        run = subprocess.run([sys.executable, str(script), str(path)], env=env, capture_output=True, text=True, timeout=240)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
        child = np.load(path)
        for name in names:
            for cp in H.CHECKPOINTS:
                for a in H.ARRAYS + ("objective",):
                    assert child[f"{name}/{cp}/{a}"].tobytes() == np.asarray(_device(name)[cp][a], dtype=np.float64).tobytes(), (queues, name, cp, a)


# ---- 4. the public call ------------------------------------------------------------------------------------------------------------------
def _adata(Z, batch):
    ad = make_adata(np.zeros((Z.shape[0], 2)), np.zeros((Z.shape[0], 1)))
    ad.obsm["X_pca"] = Z
    ad.obs["slide"] = np.array(["s0", "s1", "s2"])[batch]
    return ad


@functools.lru_cache(maxsize=None)
def _public(name):
    from spatialcore_amd.integration import harmony_integrate

    Z, batch, types = H.recipe(name)
    K = [r[2] for r in H.RECIPES if r[0] == name][0]
    return harmony_integrate(_adata(Z, batch), "slide", nclust=K), Z, batch, types


def test_public_call_writes_the_documented_keys_and_stops_early(caplog):
    from spatialcore_amd.integration import harmony_integrate

    log = logging.getLogger("spatialcore_amd")
    log.addHandler(caplog.handler)
    try:
        Z, batch, _ = H.recipe("three")
        ad = harmony_integrate(_adata(Z.astype(np.float32), batch), "slide", nclust=10)
    finally:
        log.removeHandler(caplog.handler)
    out, info = ad.obsm["X_pca_harmony"], ad.uns["harmony"]
    assert out.dtype == np.float64 and out.shape == Z.shape and np.all(np.isfinite(out))
    assert set(info) == {"params", "nclust", "n_blocks", "batches", "objective_start", "objectives", "n_rounds", "converged"}
    assert info["nclust"] == 10 and info["n_blocks"] == 20 and info["batches"] == {"s0": 400, "s1": 400, "s2": 400}
    assert info["params"]["theta"] == 2.0 and info["params"]["key"] == "slide" and info["params"]["nclust"] == 10
    assert info["converged"] is True and info["n_rounds"] == len(info["objectives"]) < 10       # the objective settled
    assert all(o.dtype == np.float64 and 1 <= o.size <= 20 for o in info["objectives"])
    assert info["objectives"][0][0] < info["objective_start"]
    entry = ad.uns["spatialcore_metadata"]["operations"][-1]
    assert entry["function"] == "harmony_integrate" and entry["parameters"]["n_batches"] == 3
    assert any("Harmony: 1,200 cells x 10 features" in r.getMessage() for r in caplog.records)


def test_neighbors_takes_the_result_as_it_is():
    from spatialcore_amd.neighbors import neighbors

    ad, Z, batch, _ = _public("three")
    neighbors(ad, n_neighbors=15, use_rep="X_pca_harmony")
    assert ad.obsp["connectivities"].shape == (Z.shape[0], Z.shape[0]) and ad.uns["neighbors"]["params"]["use_rep"] == "X_pca_harmony"


def test_public_objectives_equal_the_stepwise_calls_byte_for_byte():
    from spatialcore_amd.integration import harmony

    ad, Z, batch, _ = _public("three")
    info = ad.uns["harmony"]
    ctx = _ctx()
    Y = harmony.kmeans_start(ctx, harmony.unit_rows(Z), 10, 10, 0)
    try:
        start = ctx.harmony_begin(Z, batch, 3, Y, info["n_blocks"], 0.1, 2.0, 1.0)
        objectives = []
        for _ in range(info["n_rounds"]):
            objectives.append(ctx.harmony_cluster(20, 1e-5))
            ctx.harmony_correct()
        Zcorr = ctx.harmony_get("Zcorr")
    finally:
        ctx.harmony_end()
    assert start == info["objective_start"]
    assert [o.tobytes() for o in objectives] == [o.tobytes() for o in info["objectives"]]
    assert Zcorr.tobytes() == ad.obsm["X_pca_harmony"].tobytes()
    old, new = objectives[-2][-1], objectives[-1][-1]
    assert abs(old - new) / abs(old) < 1e-4


# ---- 5. quality: thresholds from the restatement and the start ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r[0] for r in H.RECIPES])
def test_batches_mix_and_types_stay_apart_as_in_the_restatement(name):
    """harmony_restated.RECIPE_FIGURES: the restatement's figures over the 15 exact nearest neighbours, started from sklearn's
    KMeans (tests/test_cpu_harmony.py computes them and checks that they are within 0.05 of chance)."""
    ad, Z, batch, types = _public(name)
    before_want, after_want, chance, type_want, _, _ = H.RECIPE_FIGURES[name]
    before = H.neighbour_shares(Z, batch, types)
    after = H.neighbour_shares(ad.obsm["X_pca_harmony"], batch, types)
    print(f"{name}: same-batch {before[0]:.4f} -> {after[0]:.4f} (restated {after_want:.4f}, chance {chance:.4f}), "
          f"same-type {after[1]:.4f} (restated {type_want:.4f}); {ad.uns['harmony']['n_rounds']} outer rounds")
    assert abs(before[0] - before_want) < 1e-3
    assert abs(after[0] - after_want) <= 0.05
    assert abs(after[1] - type_want) <= 0.005
