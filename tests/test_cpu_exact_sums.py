"""The oracle's ICP step against the bignum reference of tests/icp_rows_ref.py: the fixed-point sums RNE(clamp(row_i) * clamp(row_j) * 2^32)
formed with exact rationals and unbounded integers, at 80 x 60 -- on an ordinary scene, where the clamp engages, on exact ties of both
signs, and with NaN / +-Inf scattered at the wave boundaries.  tests/test_track_batch_gpu.py checks the kernel against the same numbers."""
import numpy as np
import pytest

import icp_rows_ref as ref
import orc


def orc_sums(inp):
    sums, _ = orc.icp_step(inp["Rcurr"], inp["tcurr"], inp["vc"], inp["nc"], inp["Rprev_inv"], inp["tprev"], orc.Cam(*[float(v) for v in inp["cam"]]),
                           inp["vp"], inp["npv"], inp["dist"], inp["angle"])
    return [int(v) for v in sums[:29]]


@pytest.mark.parametrize("name", list(ref.INPUTS))
def test_oracle_sums_equal_the_bignum_reference(name):
    inp = ref.INPUTS[name]()
    rows, found, sums = ref.reference(inp)
    ref.check_preconditions(name, rows, found)
    assert orc_sums(inp) == sums


@pytest.mark.parametrize("name", list(ref.INPUTS))
def test_oracle_gates_out_nan_and_inf_at_wave_boundaries(name):
    """the poisoned pixels are gated out and nothing else changes: the sums are those of the clean input without the rows of the poisoned
    pixels (and of the pixels that looked one of them up)"""
    clean = ref.INPUTS[name]()
    inp, where = ref.poison(clean)
    rows, found, sums = ref.reference(inp)
    crow, cfound, csums = ref.reference(clean)
    assert sums[28] < csums[28] and csums[28] - sums[28] <= 2 * len(where), (sums[28], csums[28], len(where))
    same = found & cfound
    assert np.array_equal(rows[same], crow[same]) and not (found & ~cfound).any()
    assert np.isfinite(rows[found]).all()
    assert orc_sums(inp) == sums
