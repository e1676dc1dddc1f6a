#!/usr/bin/env python3
"""Generate tests/golden/golden_poisson.npz by running the REFERENCE's Poisson integration (src/utils/stat_utils.py:142-199) and
its ``standardize_image_center(...).astype(np.uint8)`` (src/utils/frame_utils.py:39-53, as src/visualizer.py:432-433 calls them)
on the seeded cases of tests/_poisson_cases.py.  Runs only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_poisson.py

Stored per case: ``<case>_P`` = poisson_reconstruct(flow[1], flow[0], boundary) (the boundary's dtype; on the rows
``stored_rows(case)`` only, for the cases larger than 64 x 64), ``<case>_absmax`` = max|P| of the whole field and ``<case>_u8`` =
the whole uint8 picture.  The inputs are rebuilt from seeds by ``case_inputs``.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
from _poisson_cases import CASES, case_inputs, stored_rows  # noqa: E402


def main():
    import_reference()   # (stubs cv2, openpiv, ... so that src.utils imports)
    from src.utils.frame_utils import standardize_image_center
    from src.utils.stat_utils import poisson_reconstruct
    out = {}
    for name in CASES:
        flow, boundary = case_inputs(name)
        P = poisson_reconstruct(flow[1], flow[0], boundary)
        assert P.dtype == boundary.dtype
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            u8 = standardize_image_center(P).astype(np.uint8)
        rows = stored_rows(name)
        out[name + "_P"] = P if rows is None else P[rows]
        out[name + "_absmax"] = np.abs(P).max()
        out[name + "_u8"] = u8
        print(f"{name:28s} {P.dtype} max|P| {np.abs(P).max():.6g}")
    path = os.path.join(HERE, "golden_poisson.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
