"""The cases tests/test_emu_nmf.py (CPU emulator build, host pointers) and tests/test_nmf_gpu.py (gfx950) both run against
tests/known_answers_nmf.py.  A backend supplies two callables:
    kernel(x, head, n_next, mean, maxabs, cs, ms, norms, center, floor, want_max) -> (outs, row maxima or None)
        d4w_nmf_normalise_f32 alone on float32 arrays (cs: the arrays standing in for the correlograms; head may be None)
    public(x, templates, center, floor, head) -> list of arrays
        the whole of detect.compute_nmf_correlograms (row statistics, matrix-core correlator, the normaliser)
"""
import functools

import numpy as np

from tests import known_answers_nmf as kn
from tests.test_emu_rowops import TOL            # the correlator's parity tolerance, relative to a row's largest correlation

MAX_SUPPORT = 7936                               # d4w_nmf_max_support(), asserted by the tests
SUPPORTS = {"1": (1, 2), "2": (2, 135), "pair": (135, 155), "497": (497, 155), "max": (MAX_SUPPORT, 135)}     # (alone, its partner)
NS_FORMS = ("m-1", "m", "m+1", "T-1", "T", "T+1", "2T+3", "4500")


def ns_of(form, m):
    T = kn.TILE
    return {"m-1": m - 1, "m": m, "m+1": m + 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3, "4500": 4500}[form]


def check_kernel_alone(kernel, support, ns_form):
    """Every (center, templates, continuation, rows) combination of one support and one row length; the row maxima of the
    epilogue are asked for on every second combination and must equal the maximum of the rows bit for bit."""
    m0, partner = SUPPORTS[support]
    ns = ns_of(ns_form, max(m0, partner) if ns_form.startswith("m") else m0)
    if ns < 1:
        return 0
    rng = np.random.default_rng(1000 * m0 + ns)
    done = 0
    for nx in (1, 3, 8):
        x = (rng.standard_normal((nx, ns)) * rng.uniform(0.5, 40.0, (nx, 1)) + rng.uniform(-30.0, 30.0, (nx, 1))).astype(np.float32)
        if nx == 8:
            x[3] = 0.0                                       # a dead row
            x[5] += 5000.0                                   # a row that is nearly all offset
        mean, mx = x.astype(np.float64).mean(axis=1), np.abs(x).max(axis=1).astype(np.float32)
        for ms in ((m0,), (m0, partner)):
            mmax = max(ms)
            head = (rng.standard_normal((nx, mmax + 4)) * 3.0 + x[:, :1]).astype(np.float32)      # pitch: 5 more than is read
            cs = [rng.uniform(-1.0, 1.0, (nx, ns)).astype(np.float32) for _ in ms]
            norms = [float(rng.uniform(0.5, 9.0)) for _ in ms]
            for cont in (False, True):
                for center in (True, False):
                    want_max = (done % 2) == 0
                    hd = head if cont else None
                    outs, rmax = kernel(x, hd, mmax - 1 if cont else 0, mean, mx, cs, ms, norms, center, kn.FLOOR, want_max)
                    for t, m in enumerate(ms):
                        ref, bound, compared = kn.nmf(x, cs[t], m, norms[t], center, kn.FLOOR, hd, mean, mx)
                        assert compared.all(), (support, ns, nx, ms, cont, center, float(1.0 - compared.mean()))
                        err = np.abs(outs[t].astype(np.float64) - ref)
                        over = err - bound
                        assert np.all(err <= bound), (support, ns, nx, ms, t, cont, center, float(over.max()), np.unravel_index(np.argmax(over), over.shape))
                        assert np.all(outs[t][ref == 0] == 0)
                        if want_max:
                            assert np.array_equal(rmax[t], outs[t].max(axis=1))
                    done += 1
    return done


# ------------------------------------------------------------------------------------------
# the scene
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_reference(name, center=True, with_head=True):
    """(ref, bound, compared, slack) of the scene for template `name`, computed once and left unchanged."""
    x, head = kn.scene()
    out = kn.nmf_of_template(x, kn.templates()[name], center, kn.FLOOR, head if with_head else None)
    for a in out:
        a.setflags(write=False)
    return out


def check_public_on_scene(public):
    """|got - ref| <= bound + TOL max_k |c_ref(row)| / (|h'| sqrt(V[k])), pair and single, with and without the head."""
    x, head = kn.scene()
    tp = kn.templates()
    for center in (True, False):
        for with_head in (True, False):
            got = public(x, [tp["hf"], tp["lf"]], center, kn.FLOOR, head if with_head else None)
            for name, g in zip(("hf", "lf"), got):
                ref, bound, compared, slack = scene_reference(name, center, with_head)
                assert compared.all()
                err = np.abs(np.asarray(g, dtype=np.float64) - ref)
                lim = bound + TOL * slack
                print("scene %s center=%s head=%s: max err %.3e, max err / limit %.3f" % (name, center, with_head, err.max(),
                                                                                            float(np.max(err / np.where(lim > 0, lim, 1.0)))))
                assert np.all(err <= lim), (name, center, with_head, float((err - lim).max()))
    # one template alone (the one-template correlator, the normaliser's one-template form): the same answer to the same limit
    (one,) = public(x, [tp["lf"]], True, kn.FLOOR, head)
    ref, bound, _, slack = scene_reference("lf", True, True)
    assert np.all(np.abs(np.asarray(one, dtype=np.float64) - ref) <= bound + TOL * slack)


def check_properties(public, pick_times=None, reference_correlogram=None):
    x, head = kn.scene()
    tp = kn.templates()
    hf, lf = public(x, [tp["hf"], tp["lf"]], True, kn.FLOOR, head)
    hf, lf = np.asarray(hf, dtype=np.float64), np.asarray(lf, dtype=np.float64)
    m = {"hf": len(kn.support(tp["hf"])), "lf": len(kn.support(tp["lf"]))}
    assert max(np.abs(hf).max(), np.abs(lf).max()) <= 1.0 + 2.0 ** -20
    # exact zeros: the dead row, the inside of the dropout and of the constant stretch, a one-tap template
    assert np.all(hf[5] == 0) and np.all(lf[5] == 0)
    assert np.all(hf[3, kn.DROPOUT[0]:kn.DROPOUT[1] - m["hf"] + 1] == 0) and np.all(lf[3, kn.DROPOUT[0]:kn.DROPOUT[1] - m["lf"] + 1] == 0)
    assert np.all(hf[6, kn.CONSTANT[0]:kn.CONSTANT[1] - m["hf"] + 1] == 0) and np.all(lf[6, kn.CONSTANT[0]:kn.CONSTANT[1] - m["lf"] + 1] == 0)
    (tap,) = public(x, [np.array([1.0])], True, kn.FLOOR, None)
    assert np.all(np.asarray(tap) == 0)
    # every call row: argmax at the call's lag, >= 0.7 there, < 0.45 farther than m from it (the float64 model: >= 0.77, <= 0.39)
    lags = np.arange(kn.NS)
    for row, (name, at) in kn.CALLS.items():
        r = hf[row] if name == "hf" else lf[row]
        assert int(np.argmax(r)) == at and r[at] >= 0.7, (row, int(np.argmax(r)), float(r[at]))
        assert np.abs(r[np.abs(lags - at) > m[name]]).max() < 0.45, row
    # without local mean removal the offset-plus-ramp row is lost
    _, lf_raw = public(x, [tp["hf"], tp["lf"]], False, kn.FLOOR, head)
    assert abs(float(np.asarray(lf_raw)[2, kn.CALLS[2][1]])) < 0.45
    # the call cut by the end of the file
    hf_cut, _ = public(x, [tp["hf"], tp["lf"]], True, kn.FLOOR, None)
    assert hf[7].max() >= 0.7 and np.asarray(hf_cut)[7].max() < 0.6
    # a block scaled by 1e-9, or (centred) lifted by 1e3: the answer of THAT float32 block to the same limit; and since scaling
    # only rounds every sample once more in float32 (the kind of error the limit is made of), within twice the limit of the
    # unscaled answer
    ref, bound, _, slack = scene_reference("hf")
    for xs, hs, same in (((x.astype(np.float64) * 1e-9).astype(np.float32), (head.astype(np.float64) * 1e-9).astype(np.float32), True),
                         (x + np.float32(1e3), head + np.float32(1e3), False)):
        got = np.asarray(public(xs, [tp["hf"]], True, kn.FLOOR, hs)[0], dtype=np.float64)
        r2, b2, c2, s2 = kn.nmf_of_template(xs, tp["hf"], True, kn.FLOOR, hs)
        assert c2.all()
        assert np.all(np.abs(got - r2) <= b2 + TOL * s2), same
        if same:
            assert np.all(np.abs(got - ref) <= 2.0 * (bound + TOL * slack))
    # the spike row: the reference-style correlogram at 0.45 max finds nothing at the call, nmf >= 0.6 finds it
    if pick_times is not None:
        at = kn.CALLS[4][1]
        corr = reference_correlogram(x[4:5], tp["hf"])
        picks = np.asarray(pick_times(corr, 0.45 * float(np.max(corr)))[0])
        assert not np.any(np.abs(picks - at) <= 2), picks
        picks = np.asarray(pick_times(hf[4:5].astype(np.float32), 0.6)[0])
        assert at in picks, picks
