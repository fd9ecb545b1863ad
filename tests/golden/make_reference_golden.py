"""Writes tests/golden/reference.npz: the edge inputs of tests/reference_cases.py and what the reference's own
kernels, executed on the CPU (oracle/refexec), compute from them in raster order -- outputs, gradients and the
masks of the elements whose computation read outside a frame.  These are results the reference's programs wrote;
nothing of its text is stored.  Needs the executor (built by `__graft_entry__.build()` when the reference checkout
is present):

    python -m tests.golden.make_reference_golden
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "reference.npz")


def build_arrays():
    from oracle.refexec import ref_exec as R
    from tests import reference_cases as rc
    R.set_order("raster")
    arrays, seen = {}, {}
    for name, case in rc.cases().items():
        arrays.update(rc.flatten(name, case, rc.run_ref(R, case), seen))
    return arrays


def main():
    from oracle.refexec import ref_exec as R
    if not R.available():
        sys.exit("oracle/_ref/libvfi_ref.so is missing: build it first (python -m oracle.refexec.build_ref)")
    arrays = build_arrays()
    np.savez_compressed(PATH, **arrays)
    print("%s: %d arrays, %d bytes" % (PATH, len(arrays), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
