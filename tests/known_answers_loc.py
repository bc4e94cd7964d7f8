"""float64 NumPy restatements for csrc/loc.hip, and the synthetic cables its tests and fixture share.

solve_lq_sums restates the reference's solve_lq (loc.py:57-128) the way the kernel computes it: the normal equations
G^T G and G^T dt are formed by sums over the channels (in a given channel order) and solved, instead of the reference's
inv(G^T G + lambda I) @ G^T @ dt.  The rows of G come either from the reference's trigonometry or from the algebraic form
(d_x / (R c0), ...) that the kernel uses; both are accepted by the issue this file answers.  Running it with permuted
channel orders against the fixture recorded from the reference measures how far a different summation order alone moves
the result, which is what the limits of tests/test_emu_loc.py and tests/test_loc_gpu.py are derived from.

misfit_grid_f64 restates the misfit grid in two passes (mean, then RMS about it).
"""
import numpy as np

C0 = 1490.0
CHANNELS = (5, 400, 3000, 11020)
NOISES = (0.0, 0.010)
LAMBDA = 1e-5
# [x, y, z, t0]; the default first guess (40000, 23000) lies south of the "line" cable and inside the arc of the "bent" one.
# The last "line" source lies north of the cable: the reference, started south of it, finds its mirror image.
SOURCES = {
    "line": [(38000.0, 21000.0, -60.0, 12.5), (30000.0, 18000.0, -35.0, 7.25), (52000.0, 24500.0, -60.0, 30.0),
             (45000.0, 30000.0, -60.0, 12.5)],
    "bent": [(38000.0, 21000.0, -60.0, 12.5), (43000.0, 27000.0, -35.0, 7.25), (33000.0, 26000.0, -80.0, 30.0)],
}
# the issue's known answers: noise-free, fix_z, depth -60, 20 iterations on the 11 020-channel line cable
KNOWN_SOUTH = [(38000.0, 21000.0), (30000.0, 18000.0), (52000.0, 24500.0)]
KNOWN_NORTH = (45000.0, 30000.0)


def make_cable(kind, nch):
    """[nch x 3] positions.  "line": 45 km, heading east-north-east with a gentle bow, -100 m down to -600 m.
    "bent": two thirds of a circle of 15 km radius around (38000, 23000), depth undulating between -100 m and -600 m."""
    s = np.linspace(0.0, 1.0, nch)
    if kind == "line":
        x = 20000.0 + 45000.0 * s
        y = 23500.0 + 7000.0 * s + 800.0 * np.sin(np.pi * s)
        z = -100.0 - 500.0 * s
    elif kind == "bent":
        a = 0.3 + 4.2 * s
        x = 38000.0 + 15000.0 * np.cos(a)
        y = 23000.0 + 15000.0 * np.sin(a)
        z = -350.0 - 250.0 * np.sin(5.0 * np.pi * s)
    else:
        raise ValueError(kind)
    return np.stack([x, y, z], axis=1)


def arrival_times(t0, cable, pos, c0):
    """loc.py:13-25 written out."""
    return t0 + np.sqrt((cable[:, 0] - pos[0]) ** 2 + (cable[:, 1] - pos[1]) ** 2 + (cable[:, 2] - pos[2]) ** 2) / c0


def g_rows(cable, n, c0, fix_z, form):
    """The rows of G at n.  form "trig": the reference's; "algebraic": d / (R c0) with the reference's rows where r = 0."""
    dx, dy, dz = n[0] - cable[:, 0], n[1] - cable[:, 1], n[2] - cable[:, 2]
    r = np.sqrt(dx ** 2 + dy ** 2)
    if form == "trig":
        th, ph = np.arctan2(np.abs(dz), r), np.arctan2(dy, dx)
        g = [np.cos(th) * np.cos(ph) / c0, np.cos(th) * np.sin(ph) / c0, np.sin(th) / c0]
    else:
        R = np.sqrt(dx ** 2 + dy ** 2 + dz ** 2)
        with np.errstate(all="ignore"):
            inv = 1.0 / (R * c0)
            g = [dx * inv, dy * inv, np.abs(dz) * inv]
        on_axis, on_chan = (r == 0) & (dz != 0), (r == 0) & (dz == 0)
        g[0] = np.where(on_axis, np.cos(np.pi / 2) / c0, np.where(on_chan, 1.0 / c0, g[0]))
        g[1] = np.where(r == 0, 0.0, g[1])
        g[2] = np.where(on_axis, 1.0 / c0, np.where(on_chan, 0.0, g[2]))
    if fix_z:
        g = g[:2]
    return np.stack(g + [np.ones_like(r)], axis=1)


def solve_lq_sums(Ti, cable, c0, Nbiter=10, fix_z=False, first_guess=None, form="trig", order=None):
    """History [Nbiter x 4] of the damped Gauss-Newton iteration with the normal equations formed by sums over the valid
    channels taken in `order` (a permutation of the channel indices; None = as given)."""
    Ti, cable = np.asarray(Ti, dtype=np.float64), np.asarray(cable, dtype=np.float64)
    keep = np.flatnonzero(~np.isnan(Ti)) if order is None else np.asarray(order)[~np.isnan(Ti[np.asarray(order)])]
    Ti, cable = Ti[keep], cable[keep]
    n = np.array([40000.0, 23000.0, -60.0, Ti.min()]) if first_guess is None else np.array(first_guess, dtype=np.float64)
    idx = [0, 1, 3] if fix_z else [0, 1, 2, 3]
    hist = np.empty((Nbiter, 4))
    for j in range(Nbiter):
        G = g_rows(cable, n, c0, fix_z, form)
        dt = Ti - arrival_times(n[3], cable, n[:3], c0)
        p = G.shape[1]
        A = np.array([[np.cumsum(G[:, i] * G[:, k])[-1] for k in range(p)] for i in range(p)])     # sequential sums
        b = np.array([np.cumsum(G[:, i] * dt)[-1] for i in range(p)])
        dn = np.linalg.solve(A + LAMBDA * np.eye(p), b)
        n[idx] += (0.7 if j < 4 else 1.0) * dn
        hist[j] = n
    return hist


def stats_at(Ti, cable, c0, n, fix_z, form="trig"):
    """G^T G (no regularisation), the sum of squared residuals and the pick count at n over the valid channels."""
    Ti, cable = np.asarray(Ti, dtype=np.float64), np.asarray(cable, dtype=np.float64)
    keep = ~np.isnan(Ti)
    G = g_rows(cable[keep], n, c0, fix_z, form)
    dt = Ti[keep] - arrival_times(n[3], cable[keep], n[:3], c0)
    return G.T @ G, float(np.sum(dt ** 2)), int(keep.sum())


def misfit_grid_f64(Ti, cable, c0, xs, ys, z):
    """(rms, t0), each [ny x nx], for one call: e = Ti - distance / c0 over the valid channels, t0 = mean e, rms about it.
    Also returns max |e| and the largest spread max e - min e over the nodes, which the tests' error bounds need."""
    Ti, cable = np.asarray(Ti, dtype=np.float64), np.asarray(cable, dtype=np.float64)
    keep = ~np.isnan(Ti)
    Ti, cable = Ti[keep], cable[keep]
    rms, t0 = np.full((len(ys), len(xs)), np.nan), np.full((len(ys), len(xs)), np.nan)
    emax = spread = 0.0
    if not len(Ti):
        return rms, t0, emax, spread
    for iy, y in enumerate(ys):
        d = np.sqrt((cable[:, 0][None, :] - np.asarray(xs)[:, None]) ** 2 + (cable[:, 1][None, :] - y) ** 2 + (cable[:, 2][None, :] - z) ** 2)
        e = Ti[None, :] - d / c0
        m = e.mean(axis=1)
        t0[iy] = m
        rms[iy] = np.sqrt(np.mean((e - m[:, None]) ** 2, axis=1))
        emax = max(emax, float(np.abs(e).max()))
        spread = max(spread, float((e.max(axis=1) - e.min(axis=1)).max()))
    return rms, t0, emax, spread
