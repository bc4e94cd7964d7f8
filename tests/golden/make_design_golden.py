"""Generate tests/golden/design_edges.npz: the masks the REAL reference's five f-k designers return at the edge cases of
tests/design_cases.py (odd shapes, one channel, speed-edge ties, band edges that move the column loops), and its fk_filt
on seeded blocks with an odd axis.

Run in the build container, where the reference sources are present:

    python tests/golden/make_design_golden.py

Per case `<name>` and design `<d>` (classic, hybrid, ninf, gs, ninf_gs): `<name>/<d>`, the mask in float64.  For an odd
number of time samples the reference's hybrid_ninf_filter_design returns an [nx, ns - 1] mask (its |H|^2 row is built from
two halves of ns // 2 columns); the fixture records that shape as `<name>/ninf_shape` instead of the mask -- it is why
the package refuses the call.  `fkfilt/<nx>x<ns>`: dsp.fk_filt of tests.design_cases.fkfilt_block((nx, ns)).
The blurred masks are dense float64 and do not compress: the 130 x 600 case is left out when the fixture would pass the
size of the largest one already here, and what remains is written in pieces (tests/golden_npz.py), every file below it.
tests/test_oracle_design_edges.py pins the oracle against this file; nothing that runs on the GPU box reads the reference.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_harness import import_reference  # noqa: E402
from tests import design_cases as dc  # noqa: E402
from tests.golden_npz import _zsize, save  # noqa: E402

LIMIT = 1001143                     # the largest fixture file in tests/golden/ (detect_12x2000.npz)


def dense(m):
    return np.ascontiguousarray(m.todense() if hasattr(m, "todense") else m, dtype=np.float64)


def record(ref, cases):
    out = {"cases": np.array(cases)}
    for case in cases:
        shape = dc.CASES[case][0]
        for design in dc.DESIGNS:
            m = dense(dc.call(ref.dsp, design, case))
            if dc.has_design(case, design):
                assert m.shape == shape, (case, design, m.shape)
                out["%s/%s" % (case, design)] = m
            else:
                out["%s/ninf_shape" % case] = np.array(m.shape)
            print("%-12s %-8s %s" % (case, design, m.shape))
    for shape in dc.FKFILT_SHAPES:
        x = dc.fkfilt_block(shape)
        out["fkfilt/%dx%d" % shape] = np.asarray(ref.dsp.fk_filt(x.copy(), *dc.FKFILT_ARGS), dtype=np.float64)
    return out


def main():
    ref = import_reference()
    path = os.path.join(HERE, "design_edges.npz")
    cases = list(dc.FIXTURE_CASES)
    if _zsize(record(ref, cases)) > LIMIT:      # the 130 x 600 case stays in the oracle comparisons only
        cases.remove("wide")
    files = save(path, record(ref, cases))      # in pieces where one file would still pass the limit
    for f in files:
        print(f, os.path.getsize(f), "bytes")
        assert os.path.getsize(f) <= LIMIT
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
