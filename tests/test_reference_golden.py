"""The oracle against tests/golden/reference.npz: what the reference's own kernels, executed on the CPU, computed
from the edge inputs of tests/reference_cases.py (raster order; generator: tests/golden/make_reference_golden.py).
Runs everywhere -- the file holds results, so neither the reference checkout nor the executor is needed -- under the
same rules as tests/test_reference_exec.py.  Where the executor is available it must reproduce the file bit for bit.
"""
import os

import numpy as np
import pytest

from tests import reference_cases as rc

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference.npz")
NAMES = sorted(rc.cases())


@pytest.fixture(scope="module")
def recorded():
    return rc.load(np.load(PATH))


def test_file_is_small_and_complete(recorded):
    assert os.path.getsize(PATH) < 1000 * 1000
    assert sorted(recorded) == NAMES
    for name, (case, ref) in recorded.items():
        for k, v in rc.cases()[name].inputs.items():      # the stored inputs are the generator's
            assert np.array_equal(case.inputs[k], v, equal_nan=True), (name, k)
        assert ref, name


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_recorded_reference(name, recorded, oracle):
    case, ref = recorded[name]
    rc.check(name, case, ref, rc.run_oracle(oracle, case, ref))


def test_executor_reproduces_the_file(recorded):
    """Checks something only where the executor is built (it then guards the file against a stale recording);
    elsewhere it passes without a check -- the tests above are the ones that hold everywhere."""
    from oracle.refexec import ref_exec as R
    if not R.available():
        return
    R.set_order("raster")
    try:
        for name, (case, ref) in recorded.items():
            got = rc.run_ref(R, case)
            assert sorted(got) == sorted(ref), name
            for k in ref:
                assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k], equal_nan=ref[k].dtype != bool), (name, k)
    finally:
        R.set_order("blocks")
