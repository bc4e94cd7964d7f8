"""How far does the order of summation alone move the localisation result?  Runs the sums-then-solve restatement
(tests/known_answers_loc.solve_lq_sums) on every case of tests/golden/loc.npz in the given channel order and in a few seeded
permutations of it, with the reference's trigonometric rows and with the algebraic rows csrc/loc.hip uses, and prints the
largest difference from the iterates recorded from the reference, per group of cases.  The limits of tests/test_emu_loc.py
and tests/test_loc_gpu.py are 100 x these figures (docs/LAB_NOTEBOOK.md).  CPU only.

    python scripts/measure_loc_limits.py [--perms 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import golden_npz  # noqa: E402
from tests import known_answers_loc as ka  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--perms", type=int, default=3)
    a = ap.parse_args()
    G = golden_npz.load("loc.npz")
    c0 = float(G["c0"])
    worst = {}
    for case in [str(c) for c in G["cases"]]:
        cable, Ti, fix_z = G[str(G[case + "/geom"]) + "/cable_pos"], G[case + "/Ti"], bool(G[case + "/fix_z"])
        nch = len(Ti)
        group = ("fix_z" if fix_z else "free_z", "line" if case.startswith("line") else "bent", nch)
        rng = np.random.default_rng(nch + 17 * fix_z)
        orders = [None] + [rng.permutation(nch) for _ in range(a.perms)]
        for form in ("trig", "algebraic"):
            for order in orders:
                h = ka.solve_lq_sums(Ti, cable, c0, 10, fix_z, form=form, order=order)
                d = np.abs(h - G[case + "/hist"])
                w = worst.setdefault(group, [0.0, 0.0, 0.0])
                w[0] = max(w[0], float(d[:, :2].max()))
                w[1] = max(w[1], float(d[:, 2].max()))
                w[2] = max(w[2], float(d[:, 3].max()))
    print("%-28s %12s %12s %12s" % ("group (10 iterations)", "max |dxy| m", "max |dz| m", "max |dt0| s"))
    tot = {}
    for group in sorted(worst):
        w = worst[group]
        print("%-28s %12.3e %12.3e %12.3e" % ("%s %s %d" % group, w[0], w[1], w[2]))
        t = tot.setdefault(group[0], [0.0, 0.0, 0.0])
        for i in range(3):
            t[i] = max(t[i], w[i])
    for k, t in sorted(tot.items()):
        print("%-28s %12.3e %12.3e %12.3e" % ("ALL " + k, t[0], t[1], t[2]))


if __name__ == "__main__":
    main()
