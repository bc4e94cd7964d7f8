"""Generate tests/golden/loc.npz and tests/golden/reference_signatures_loc.json from the reference's own loc module
(oracle/ref_harness.import_reference; it needs only NumPy).

    python tests/golden/make_loc_golden.py

Cables are synthetic (tests/known_answers_loc.make_cable): "line", a gently curved line of 45 km that descends from -100 m
to -600 m, and "bent", a strongly bent arc with an undulating depth, so that G^T G is well conditioned with free z.  Per
channel count of 5, 400, 3000 and 11 020 the same curve is sampled more densely.

Keys: `cases` (names), `c0`, `<cable>_<nch>/cable_pos`, and per case `<case>/...`:
  geom     name of the case's cable entry          src [x, y, z, t0]        noise (s)        fix_z
  Ti       the arrival times the reference's calc_arrival_times gives for src, plus seeded Gaussian noise
  hist     [10 x 4]: solve_lq(Ti, cable_pos, c0, Nbiter=k, fix_z) for k = 1 .. 10, i.e. the iterate after every iteration
  n20      the same with Nbiter = 20
  var, cov, unc    cal_variance_residuals, calc_covariance_matrix and calc_uncertainty_position at hist[9]
  sub_idx, sub_hist, sub_n20 (some cases): the channels kept when every other pick is dropped, and the reference run on them
and per cable of at most 3000 channels `<cable>_<nch>/helpers_at` = [x, y, z, t0] with `/arrival`, `/distance`, `/radii`,
`/theta`, `/phi`: the five small helpers there.  Only data goes into the fixtures.
"""
import contextlib
import inspect
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_harness import import_reference  # noqa: E402
from tests.golden_npz import save  # noqa: E402
from tests.known_answers_loc import C0, CHANNELS, NOISES, SOURCES, make_cable  # noqa: E402

NAMES = ["calc_arrival_times", "calc_distance_matrix", "calc_radii_matrix", "calc_theta_vector", "calc_phi_vector", "solve_lq",
         "cal_variance_residuals", "calc_covariance_matrix", "calc_uncertainty_position"]


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def run(ref, Ti, cable, fix_z):
    hist = np.array([quiet(ref.solve_lq, Ti.copy(), cable, C0, Nbiter=k, fix_z=fix_z) for k in range(1, 11)])
    n20 = quiet(ref.solve_lq, Ti.copy(), cable, C0, Nbiter=20, fix_z=fix_z)
    return hist, n20


def main():
    ref = import_reference().loc
    sig = {}
    for name in NAMES:
        sig[name] = [[p.name, "<required>" if p.default is inspect._empty else p.default]
                     for p in inspect.signature(getattr(ref, name)).parameters.values()]
    with open(os.path.join(HERE, "reference_signatures_loc.json"), "w") as f:
        json.dump({"loc": sig}, f, indent=1, sort_keys=True)
        f.write("\n")

    rng = np.random.default_rng(20261017)
    out = {"c0": np.array(C0)}
    cases = []
    for kind in ("line", "bent"):
        for nch in CHANNELS:
            geom = "%s_%d" % (kind, nch)
            cable = make_cable(kind, nch)
            out[geom + "/cable_pos"] = cable
            for si, src in enumerate(SOURCES[kind]):
                src = np.asarray(src, dtype=np.float64)
                clean = ref.calc_arrival_times(src[3], cable, src[:3], C0)
                for noise in NOISES:
                    Ti = clean + noise * rng.standard_normal(nch) if noise else clean.copy()
                    for fix_z in (False, True):
                        case = "%s_s%d_n%d_%s" % (geom, si, round(noise * 1000), "fixz" if fix_z else "freez")
                        cases.append(case)
                        hist, n20 = run(ref, Ti, cable, fix_z)
                        n = hist[-1]
                        var = ref.cal_variance_residuals(Ti, ref.calc_arrival_times(n[3], cable, n[:3], C0), fix_z) if nch > 4 else np.nan
                        cov = quiet(ref.calc_covariance_matrix, cable, n, C0, var, fix_z)
                        unc = quiet(ref.calc_uncertainty_position, cable, n, C0, var, fix_z)
                        out.update({case + "/geom": np.array(geom), case + "/src": src, case + "/noise": np.array(noise),
                                    case + "/fix_z": np.array(fix_z), case + "/Ti": Ti, case + "/hist": hist, case + "/n20": n20,
                                    case + "/var": np.array(var), case + "/cov": cov, case + "/unc": unc})
                        if si == 0 and nch >= 400:
                            idx = np.arange(0, nch, 2)
                            sh, s20 = run(ref, Ti[idx], cable[idx], fix_z)
                            out.update({case + "/sub_idx": idx, case + "/sub_hist": sh, case + "/sub_n20": s20})
                        print("%-32s n10 = %s  |n10 - src| = %.3e m, %.3e s; unc %s" % (
                            case, np.array2string(n, precision=4), np.linalg.norm(n[:3] - src[:3]), abs(n[3] - src[3]),
                            np.array2string(unc, precision=3)))
            if nch <= 3000:
                w = np.array([41234.5, 22222.25, -47.5, 3.25])
                out.update({geom + "/helpers_at": w, geom + "/arrival": ref.calc_arrival_times(w[3], cable, w[:3], C0),
                            geom + "/distance": ref.calc_distance_matrix(cable, w[:3]), geom + "/radii": ref.calc_radii_matrix(cable, w),
                            geom + "/theta": ref.calc_theta_vector(cable, w), geom + "/phi": ref.calc_phi_vector(cable, w)})
    out["cases"] = np.array(cases)
    print(save(os.path.join(HERE, "loc.npz"), out))


if __name__ == "__main__":
    main()
