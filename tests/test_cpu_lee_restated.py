"""The inputs of the Lee's L edge tests (tests/lee_restated.py), judged without a device."""
import numpy as np

import lee_restated as le


def test_lee_edge_inputs_have_no_near_ties(oracle):
    """Every input of test_lee_rows_and_observed_at_block_and_wave_edges and test_lee_shared_two_x_passes: no |L_perm| of
    a live pair lies within 1e-6 |L| of |L| (the device's sums differ from numpy's by summation order, ~1e-12 relative),
    so the == on the counts tests the kernels and not a tie.  A dead pair is 0 >= 0 exactly, on both sides."""
    total = 0
    for n in le.ROW_SIZES:
        case = le.rows_case(oracle, n)
        assert (case["L"][~case["live"]] == 0).all() and (case["L"][case["live"]] != 0).all()
        total += le.near_ties(case["L"][:, None], case["L_perm"])
    grid = le.grid_case(oracle)
    assert (grid["L"] != 0).all()
    total += le.near_ties(grid["L"][None], grid["L_perm"])
    print(f"near ties of the Lee edge inputs: {total}")
    assert total == 0
