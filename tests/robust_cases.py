"""Cases of the robust weighted relocation (csrc/robust.hip), shared by tests/test_emu_robust.py (C ABI, CPU emulator) and
tests/test_robust_gpu.py (dw.loc.solve_robust_batch on hardware).  The answers are tests/known_answers_robust.py's.

Limits.  The rule of tests/test_emu_loc.py: the restatement is run on a case in channel order and in three seeded
permutations of the channels, and the largest difference of an iterate from the first run is what the summation order alone
does to the answer.  measure_limits() (python -m tests.robust_cases) does that for every parity case; the largest figures were
    x, y, z  1.698e-11 m        t0  1.776e-15 s
and the limits are 100 x those.  Nothing the kernel computes enters them.  The residuals follow: a position within LIM_POS and
an emission time within LIM_T0 move a residual by at most sqrt(3) LIM_POS / c0 + LIM_T0 (LIM_R).

The exact properties need no limit: the scale is 1.4826 x np.median of the |residuals| the kernel itself returns, bit for
bit; the robust weights are the definition's function of those residuals and that scale within a few roundings (Q_RTOL).
"""
import numpy as np

from tests import known_answers_loc as ka
from tests import known_answers_robust as kr

C0 = ka.C0
EPS = np.finfo(np.float64).eps
RESIDENT = 16384                       # robust_limits()[0]; the tests assert that it is
MEASURED_POS, MEASURED_T0 = 1.698e-11, 1.776e-15       # measure_limits(), see above
LIM_POS, LIM_T0 = 100 * MEASURED_POS, 100 * MEASURED_T0
LIM_R = np.sqrt(3.0) * LIM_POS / C0 + LIM_T0
Q_RTOL = 8 * EPS                       # u = |r| / (tuning s), then 1 / u or (1 - u u)^2: four roundings, doubled
LOSSES = ("l2", "huber", "bisquare")


def scene(nch, ncalls, seed, noise=1e-3, moved=0.1, kind="bent"):
    """(cable [nch x 3], Ti [ncalls x nch], sources [ncalls x 4], moved [ncalls x nch] bool): arrival times of the "bent" sources
    with Gaussian noise, a fraction of the channels moved by +-0.05 s (one period of a 20 Hz call)."""
    rng = np.random.default_rng(seed)
    cable = ka.make_cable(kind, nch)
    srcs = np.array([ka.SOURCES[kind][k % len(ka.SOURCES[kind])] for k in range(ncalls)])
    srcs[:, 2] = -60.0
    Ti = np.stack([ka.arrival_times(s[3], cable, s[:3], C0) for s in srcs]) + noise * rng.standard_normal((ncalls, nch))
    mv = np.zeros((ncalls, nch), dtype=bool)
    for k in range(ncalls):
        mv[k, rng.choice(nch, int(round(moved * nch)), replace=False)] = True
    Ti = Ti + np.where(mv, 0.05 * rng.choice([-1.0, 1.0], (ncalls, nch)), 0.0)
    return cable, Ti, srcs, mv


def _weights(form, ncalls, nch, rng):
    """None, [channel] or [ncalls x channel] weights with zeros, negatives and NaNs; the Ti under some of them is garbage."""
    if form == "none":
        return None
    w = 0.2 + rng.random((ncalls, nch) if form == "call" else nch)
    kill = rng.random(w.shape)
    w = np.where(kill < 0.06, 0.0, np.where(kill < 0.12, -1.0, np.where(kill < 0.18, np.nan, w)))
    return w


def make_case(nch, ncalls=1, fix_z=True, loss="huber", scale=None, warmup=0, Nbiter=5, weights="none", half=False, seed=0):
    """A parity case as a dict of the solver's arguments and `id`.  The first guess is 300 m from the source, so that five
    iterations converge at every channel count; half: every second channel is NaN (an odd and an even used count arise from
    nch and from the weights).  The garbage under dead weights is NaN, 1e300 and -1e300."""
    rng = np.random.default_rng(1000 + seed)
    cable, Ti, srcs, _ = scene(nch, ncalls, seed=seed)
    w = _weights(weights, ncalls, nch, rng)
    if half:
        Ti[:, 1::2] = np.nan
    if w is not None:
        dead = ~(np.broadcast_to(w, Ti.shape) > 0)
        Ti = np.where(dead, rng.choice([np.nan, 1e300, -1e300], Ti.shape), Ti)
    fg = srcs + [300.0, -200.0, 0.0, 0.05]
    return dict(id="n%d_c%d_%s_%s_s%s_w%d_it%d_%s%s" % (nch, ncalls, "fixz" if fix_z else "freez", loss, "g" if scale else "m", warmup, Nbiter,
                                                        weights, "_half" if half else ""),
                cable=cable, Ti=Ti, weights=w, loss=loss, scale=scale, warmup=warmup, Nbiter=Nbiter, fix_z=fix_z, first_guess=fg)


def parity_cases():
    """Channel counts at p + 1, around the wave (64), the workgroup (256), several strides (1025) and the LDS-resident limit,
    crossed sparingly with the calls, both fix_z, the three losses, a given scale, the warm-ups, the iteration counts, the three
    weight forms and half the channels unused."""
    L = RESIDENT
    cases = []
    for i, nch in enumerate((4, 5, 63, 64, 65, 255, 256, 257, 1025, L - 1, L, L + 1)):
        fix_z = nch != 5 and i % 2 == 0 or nch == 4
        cases.append(make_case(nch, ncalls=3 if nch in (65, 1025, L + 1) else 1, fix_z=fix_z, loss=LOSSES[1 + i % 2],
                               weights=("none", "chan", "call")[i % 3] if nch > 5 else "none", half=nch in (256, 1025, L), seed=i))
    for k, loss in enumerate(LOSSES):
        cases.append(make_case(257, ncalls=3, fix_z=False, loss=loss, weights="call", seed=20 + k))
        cases.append(make_case(1025, fix_z=True, loss=loss, scale=2e-3, weights="chan", seed=30 + k))
    for k, (warmup, nb) in enumerate(((0, 10), (4, 10), (10, 10), (12, 5), (0, 0), (0, 1), (4, 1), (2, 5))):
        cases.append(make_case(255 + k, ncalls=1 + 2 * (k % 2), fix_z=bool(k % 2), loss=LOSSES[1 + k % 2], warmup=warmup, Nbiter=nb,
                               weights=("call", "none")[k % 2], seed=40 + k))
    cases.append(make_case(L + 1, ncalls=1, fix_z=False, loss="bisquare", weights="call", half=True, seed=60))
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


def restate(case, order=None):
    """The restatement on every call of a case: a list of known_answers_robust.solve_robust_sums' dicts."""
    out = []
    for k in range(case["Ti"].shape[0]):
        w = case["weights"]
        w = w[k] if w is not None and w.ndim == 2 else w
        out.append(kr.solve_robust_sums(case["Ti"][k], case["cable"], C0, weights=w, loss=case["loss"], scale=case["scale"],
                                        Nbiter=case["Nbiter"], warmup=case["warmup"], fix_z=case["fix_z"],
                                        first_guess=case["first_guess"][k], order=order))
    return out


_REF = {}


def reference(case):
    """restate(case), computed once per process and shared; do not modify."""
    if case["id"] not in _REF:
        _REF[case["id"]] = restate(case)
    return _REF[case["id"]]


def check_against_restatement(case, hist, n, scale, q, r, nused, gtg, ssr, wsum, variance=None):
    """The parity assertions, for arrays shaped as the C ABI's ([ncalls x ...]).  gtg and ssr may be None where the caller has
    the variance = ssr / (nused - p) instead (dw.loc.solve_robust_batch's stats)."""
    ref = reference(case)
    p = 3 if case["fix_z"] else 4
    for k, a in enumerate(ref):
        what = (case["id"], k)
        assert nused[k] == a["nused"], what
        both = np.concatenate([hist[k], n[k][None]]) - np.concatenate([a["history"], a["n"][None]])
        dpos, dt0 = float(np.max(np.abs(both[:, :3]))), float(np.max(np.abs(both[:, 3])))
        print(case["id"], "call", k, "largest difference: position %.3e m, t0 %.3e s" % (dpos, dt0))
        assert dpos <= LIM_POS and dt0 <= LIM_T0, (what, dpos, dt0)
        used = ~np.isnan(a["residuals"])
        assert np.array_equal(np.isnan(r[k]), ~used) and np.array_equal(np.isnan(q[k]), ~used), what
        assert np.max(np.abs(r[k][used] - a["residuals"][used])) <= LIM_R, what
        # exact: the scale is the median of the residuals returned, the weights their function
        if case["loss"] == "l2":
            assert np.isnan(scale[k]) and np.all(q[k][used] == 1.0), what
        else:
            s = case["scale"] if case["scale"] else kr.MAD * float(np.median(np.abs(r[k][used])))
            assert scale[k] == s, (what, scale[k], s)
            qq = kr.robust_q(r[k][used], case["loss"], kr.TUNING[case["loss"]], s)
            assert np.all(np.abs(q[k][used] - qq) <= Q_RTOL * qq), what
        # the sums at the returned position, from the returned residuals and weights: recursive summation of nused terms
        w0 = 1.0 if case["weights"] is None else (case["weights"][k] if case["weights"].ndim == 2 else case["weights"])[used]
        w = w0 * q[k][used]
        G = ka.g_rows(case["cable"][used], n[k], C0, case["fix_z"], "algebraic")
        A = (G * w[:, None]).T @ G
        d = np.sqrt(np.diag(A))
        nt = max(int(used.sum()), 1)
        if gtg is not None:
            assert gtg[k].shape == (p, p) and np.array_equal(gtg[k], gtg[k].T), what
            assert np.all(np.abs(gtg[k] - A) <= 4 * nt * EPS * np.outer(d, d)), what
            assert np.isclose(ssr[k], np.sum(w * r[k][used] ** 2), rtol=4 * nt * EPS, atol=0), what
        if variance is not None:
            if nused[k] > p:
                assert np.isclose(variance[k], np.sum(w * r[k][used] ** 2) / (nused[k] - p), rtol=4 * (nt + 1) * EPS, atol=0), what
            else:
                assert np.isnan(variance[k]), what
        assert np.isclose(wsum[k], np.sum(w), rtol=4 * nt * EPS, atol=0), what


def accuracy_scenes():
    """The two scenes of the issue's table: "bent" cable, 1 ms noise, 10 % of the channels moved by +-0.05 s,
    np.random.default_rng(5): (cable, Ti [1 x nch], source [4], moved [nch])."""
    out = []
    for nch, k in ((400, 1), (3000, 2)):
        rng = np.random.default_rng(5)
        cable = ka.make_cable("bent", nch)
        src = np.array(ka.SOURCES["bent"][k])
        Ti = ka.arrival_times(src[3], cable, src[:3], C0) + 1e-3 * rng.standard_normal(nch)
        mv = np.zeros(nch, dtype=bool)
        mv[rng.choice(nch, nch // 10, replace=False)] = True
        Ti = Ti + np.where(mv, 0.05 * rng.choice([-1.0, 1.0], nch), 0.0)
        out.append((cable, Ti[None, :], src, mv))
    return out


def tie_cases():
    """(cable, Ti [1 x nch], first_guess [4]) whose |residuals| at the first guess are half equal, and all equal: the guess is
    the source, and the arrivals are the source's plus or minus exact binary fractions."""
    out = []
    for nch in (64, 1025):
        cable = ka.make_cable("bent", nch)
        src = np.array(ka.SOURCES["bent"][0])
        t = ka.arrival_times(src[3], cable, src[:3], C0)
        rng = np.random.default_rng(nch)
        sign = rng.choice([-1.0, 1.0], nch)
        half = np.where(np.arange(nch) % 2 == 0, 0.25, 0.25 * rng.random(nch))
        out.append((cable, (t + sign * half)[None, :], src))
        out.append((cable, (t + sign * 0.25)[None, :], src))
    return out


def measure_limits(perms=3):
    """The largest difference of an iterate between the restatement in channel order and in seeded permutations, over every
    parity case: (position m, t0 s)."""
    dpos = dt0 = 0.0
    for case in parity_cases():
        base = restate(case)
        for s in range(perms):
            order = np.random.default_rng(7000 + s).permutation(case["Ti"].shape[1])
            for a, b in zip(base, restate(case, order)):
                d = np.concatenate([a["history"], a["n"][None]]) - np.concatenate([b["history"], b["n"][None]])
                if np.all(np.isnan(d)):
                    continue
                dpos, dt0 = max(dpos, float(np.nanmax(np.abs(d[:, :3])))), max(dt0, float(np.nanmax(np.abs(d[:, 3]))))
        print(case["id"], "so far: position %.3e m, t0 %.3e s" % (dpos, dt0), flush=True)
    return dpos, dt0


if __name__ == "__main__":
    print("largest difference under permutation: position %.3e m, t0 %.3e s" % measure_limits())
