"""Localisation of a call from its per-channel arrival times -- mirror of the reference's `das4whales.loc`.

The nine reference functions keep their names, parameter names and defaults.  The Gauss-Newton solver, the travel times and
the misfit grid run in csrc/loc.hip (float64); `solve_lq_batch`, `misfit_grid` and `first_guess_grid` are the batched forms
the reference does not have; `vote_grid` and `associate_picks` (csrc/assoc.hip) turn the picks of detect.pick_times* into
the [ncalls x channel] arrival times these take; `delay_table`, `stack_grid`, `stack_best`, `arrivals_near` and
`locate_stack` (csrc/stack.hip) get them from the envelopes themselves by a delay-and-sum over the same grid; `beam_delays` and
`beamform` (csrc/beam.hip) close the chain with the waveform of a located call, the strain of all channels advanced by their
travel times from the position and summed; `refine_arrivals` (csrc/align.hip) correlates every channel with that waveform
around the predicted moveout and returns sub-sample arrival times for a second solve; `solve_robust_batch` (csrc/robust.hip) is
that solve, with per-channel weights and a robust loss, and `relocate` the loop beam -> re-pick -> relocate as one call;
`received_levels` (csrc/levels.hip) says how loud a located call is on every channel -- the mean square of the strain in a
window that follows the moveout, the mean square of a noise window before it, the peak --, `levels_db` turns that into a level
and an SNR in dB and `fit_spreading` fits the level against range; `project_calls`, `subtract_calls` and `remove_calls`
(csrc/project.hip) are the transpose of the beam: the call's waveform laid back on every channel along its moveout, fitted
(a signed least-squares amplitude and a correlation coefficient per channel) and subtracted, so that a second pass over the
residual sees the weaker call underneath; `beam_coherence` and `beamform_pws` (csrc/coherence.hip) say whether anything coherent
arrived from a position at all -- the windowed semblance of the beam and the phase coherence of the analytic signal along the
moveout, both in [0, 1] whatever the loudness -- and give the phase-weighted stack.  NumPy in -> NumPy float64 out; a CUDA tensor in -> a float64 tensor on the
same device and stream.  The four small per-channel helpers (distances, radii, angles) are host float64 arithmetic for NumPy input, like the
index arithmetic of the other namespaces; for tensors they stay on the device.

Arrival times that are NaN mean "no pick on this channel": the solver and the grid skip them (the reference has no such
notion -- its np.min(Ti) turns the whole result into NaN).
"""
import ctypes
import math
import sys
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import _device as dev
from . import _lib

LAMBDA_REG = 1e-5                      # loc.py:89 and :185
DEFAULT_FIRST_GUESS = (40000.0, 23000.0, -60.0)      # loc.py:86; the fourth entry is the earliest pick of the call
_MAX_GRID_Z = 65535                    # calls / positions per launch (grid limit of the kernels)


# ------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------
def _f64(x, device=None):
    """Contiguous float64 CUDA tensor holding x."""
    dev.require_gpu()
    if dev.is_tensor(x):
        if not x.is_cuda:
            x = x.to(device or "cuda")
        elif device is not None and x.device != torch.device(device):
            x = x.to(device)
        return x.to(torch.float64).contiguous()
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    return torch.from_numpy(a).to(device or ("cuda:%d" % torch.cuda.current_device()))


# Two rules for the container of a result, different on purpose.  _back serves the functions that mirror the reference and
# their batched forms: a host tensor in gives a host tensor back.  It is the rule of calc_arrival_times, solve_lq,
# calc_covariance_matrix, calc_uncertainty_position, solve_lq_batch, misfit_grid, first_guess_grid and solve_robust_batch
# (relocate returns what its last solve_robust_batch does).  _out serves the later families: any tensor in, on the host or on a
# device, gives a tensor on the device the work ran on, and only NumPy in gives NumPy back.  It is the rule of vote_grid,
# associate_picks, delay_table, stack_grid, stack_best, arrivals_near, locate_stack, beam_delays, beamform, refine_arrivals,
# received_levels, project_calls, subtract_calls, remove_calls, beam_coherence and beamform_pws.  The small arithmetic (the four per-channel helpers,
# levels_db, fit_spreading) stays in the container it was given.
def _back(y, *templates):
    """The device result in the callers' container: a tensor where any input was one (on the host if none was on a device)."""
    ts = [t for t in templates if dev.is_tensor(t)]
    if ts:
        return y if any(t.is_cuda for t in ts) else y.cpu()
    return y.cpu().numpy()


def _out(y, as_tensor):
    return y if as_tensor else y.cpu().numpy()


def _device_of(*xs):
    for x in xs:
        if dev.is_tensor(x) and x.is_cuda:
            return x.device
    return None


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _count(a):
    return int(np.prod(_shape(a)))


def _dtype_name(a):
    return str(a.dtype).split(".")[-1] if hasattr(a, "dtype") else str(np.asarray(a).dtype)


def _pos_finite(**kw):
    for name, v in kw.items():
        if not (math.isfinite(v) and v > 0):
            raise ValueError("%s must be positive and finite, got %r" % (name, v))


def _channels(cable_pos):
    """The one shape check of cable_pos, on the host: the number of channels."""
    cs = _shape(cable_pos)
    if len(cs) != 2 or cs[1] != 3 or cs[0] < 1:
        raise ValueError("cable_pos must be [channel x 3], got %s" % (cs,))
    return cs[0]


def _cable(cable_pos, device):
    _channels(cable_pos)
    return _f64(cable_pos, device)


_SKIP = object()                       # an argument a function does not have (None may be a caller's value)


def _npos(pos, t0=_SKIP):
    """The one check of positions, on the host: pos is [x, y, z] or [n x 3], t0 a scalar or [n].  Returns n."""
    ps = _shape(pos)
    if ps != (3,) and (len(ps) != 2 or ps[1] != 3):
        raise ValueError("pos must be [x, y, z] or [n x 3], got %s" % (ps,))
    n = 1 if len(ps) == 1 else ps[0]
    if t0 is not _SKIP and _count(t0) not in (1, n):
        raise ValueError("t0 must be a scalar or one value per position (%d), got shape %s" % (n, _shape(t0)))
    return n


def _positions(pos, t0, device):
    """pos and t0 after _npos on the device: (p [n x 3], t [n] or None)."""
    p = _f64(pos, device)
    p = p.reshape(1, 3) if p.dim() == 1 else p
    return p, (None if t0 is _SKIP else _f64(t0, device).reshape(-1).expand(p.shape[0]).contiguous())


def _p(t, write=False):
    """The device pointer of t for the C call, NULL for None.  write=True: through dev.out_ptr, which bumps t's version."""
    return None if t is None else (dev.out_ptr(t) if write else dev.ptr(t))


def _whole(v, name, lo, hi=None):
    """v as an int within lo .. hi, checked on the host."""
    try:
        ok = (type(v) is int or (not isinstance(v, bool) and _shape(v) == () and int(v) == v)) and v >= lo and (hi is None or v <= hi)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("%s must be a whole number of at least %d%s, got %r" % (name, lo, "" if hi is None else " and at most %d" % hi, v))
    return int(v)


def _number(v, name):
    """v as a finite float, checked on the host."""
    if isinstance(v, bool) or _shape(v) != () or not np.isfinite(v):
        raise ValueError("%s must be a finite number, got %r" % (name, v))
    return float(v)


def _inplace_view(t, device=None):
    """Whether t is a float32 CUDA tensor [rows x columns] with unit column stride (on `device`, when given): a block that is
    read, and written, where it lies."""
    return (dev.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1
            and (t.stride(0) >= t.shape[1] or t.shape[0] == 1) and (device is None or t.device == torch.device(device)))


def _env_block(env, device):
    """(float32 CUDA tensor [nch x ns] with unit column stride, row pitch in elements).  A column-sliced float32 CUDA view is
    taken as it is; everything else becomes a contiguous float32 copy on the device."""
    if _inplace_view(env, device):
        return env, (env.stride(0) if env.shape[0] > 1 else env.shape[1])
    e = dev.to_device_f32(env, device)
    return e, e.shape[1]


def _check(cable_pos, c0, fs, *, block=_SKIP, name="env", next_block=None, weights=None, xs=_SKIP, ys=_SKIP, pos=_SKIP, t0=_SKIP,
           start=_SKIP, table=_SKIP, limits=None):
    """The arguments the localisation families share, checked against each other on the host: a bad call raises ValueError
    before any device work, with or without a GPU.  Beyond the geometry, for the calls that read a record along a moveout:
    start (an int or [ncalls] ints), table = (delays, kind) with kind "r" (beam_delays(rounded=True), int32) or "kf" (the pair
    (k int32, f float32)) and delays None for tables built from the positions, and limits = (most calls, largest length) of one
    launch.  Returns the object _upload completes, so far with c0, fs, the sizes nch, ns and ns_nb (block, next block), nx, ny
    (grid axes), ncalls (positions), max_calls and max_length (limits) and kind; a function's own checks go between the two."""
    a = SimpleNamespace(c0=float(c0), fs=float(fs), nch=_channels(cable_pos), ns_nb=0, kind=None, tables=())
    _pos_finite(c0=a.c0, fs=a.fs)
    for what, b in ((name, block), ("next_block", next_block)):
        if b is _SKIP or b is None:
            continue
        if getattr(b, "ndim", 0) != 2 or b.shape[0] < 1 or b.shape[1] < 1:
            raise ValueError("%s must be a non-empty 2-D [channel x time] array, got shape %s" % (what, _shape(b)))
        if b.shape[0] != a.nch:
            raise ValueError("%s has %d rows, cable_pos %d channels" % (what, b.shape[0], a.nch))
    if block is not _SKIP:
        a.ns = block.shape[1]
    if next_block is not None:
        a.ns_nb = next_block.shape[1]
    if weights is not None and _count(weights) != a.nch:
        raise ValueError("weights must hold one value per channel (%d), got shape %s" % (a.nch, _shape(weights)))
    if xs is not _SKIP:
        a.nx, a.ny = _count(xs), _count(ys)
        if a.nx < 1 or a.ny < 1:
            raise ValueError("the grid needs at least one node")
    if pos is not _SKIP:
        a.ncalls = _npos(pos, t0)
    if limits is not None:
        a.max_calls, a.max_length = limits
        if a.ncalls > a.max_calls:
            raise ValueError("%d calls are more than the %d one launch takes" % (a.ncalls, a.max_calls))
    if start is not _SKIP:
        ss = _shape(start)
        if ss not in ((), (a.ncalls,)) or _dtype_name(start)[:3] not in ("int", "uin"):
            raise ValueError("start must be an int or [ncalls] = (%d,) ints, got shape %s of %s" % (a.ncalls, ss, _dtype_name(start)))
    if table is not _SKIP:
        delays, a.kind = table
        if delays is not None:
            want = (("r", "int32"),) if a.kind == "r" else (("k", "int32"), ("f", "float32"))
            a.tables = (delays,) if a.kind == "r" else tuple(delays)
            if len(a.tables) != len(want):
                raise ValueError("delays must be the pair (k, f) of beam_delays()")
            for t, (what, dtype) in zip(a.tables, want):
                if _shape(t) != (a.ncalls, a.nch) or _dtype_name(t) != dtype:
                    raise ValueError("delays: %s must be %s [ncalls x channel] = %s, got %s %s"
                                     % (what, dtype, (a.ncalls, a.nch), _dtype_name(t), _shape(t)))
    a.given = (block, cable_pos, xs, ys, pos, t0, weights, next_block, start)
    return a


def _upload(a, like=(), device=None):
    """The arguments of _check on one device: cable [nch x 3], e and pitch (the block; nb and pitch_nb the next one), w [nch] or
    None, gx and gy, p [ncalls x 3] and t [ncalls] or None, s (start as int64 [ncalls]) and the delay tables kr (k or r) and f
    (or None), given or built from p, each where it was asked for.  The device is `device`, or that of the first CUDA tensor
    among the arguments, `like` and the tables, or the current one; as_tensor says whether any of them is a tensor."""
    block, cable_pos, xs, ys, pos, t0, weights, next_block, start = a.given
    given = a.given + tuple(like) + a.tables
    del a.given
    a.as_tensor = any(dev.is_tensor(x) for x in given)
    a.cable = _f64(cable_pos, device if device is not None else _device_of(*given))
    d = a.device = a.cable.device
    if block is not _SKIP:
        a.e, a.pitch = _env_block(block, d)
    a.nb, a.pitch_nb = (None, 0) if next_block is None else _env_block(next_block, d)
    a.w = None
    if weights is not None:
        a.w = dev.to_device_f32(weights if dev.is_tensor(weights) else np.asarray(weights).reshape(1, -1), d).reshape(-1)
    if xs is not _SKIP:
        a.gx, a.gy = _f64(xs, d).reshape(-1), _f64(ys, d).reshape(-1)
    if pos is not _SKIP:
        a.p, a.t = _positions(pos, t0, d)
    if start is not _SKIP:
        s = start.to(d, torch.int64) if dev.is_tensor(start) else torch.from_numpy(np.array(start, dtype=np.int64)).to(d)
        a.s = s.reshape(-1).expand(a.ncalls).contiguous()
    if a.kind is not None:
        a.kr, a.f = _tables(a)
    return a


def _record(a):
    """The record prefix of the C calls that read one: the block with its pitch and sizes, the next block (or NULL) with its."""
    return dev.ptr(a.e), a.pitch, a.nch, a.ns, _p(a.nb), a.pitch_nb, a.ns_nb


def _waveforms(x, name, a):
    """The check of one float32 waveform per call (refine_arrivals' template, the beam of project_calls): their length."""
    xs = _shape(x)
    if not ((len(xs) == 2 and xs[0] == a.ncalls) or (len(xs) == 1 and a.ncalls == 1)) or _dtype_name(x) != "float32":
        raise ValueError("%s must be float32 [ncalls x L] = (%d, L) (or [L] for one call), got %s %s" % (name, a.ncalls, _dtype_name(x), xs))
    if xs[-1] < 1 or xs[-1] > a.max_length:
        raise ValueError("the length %d of %s is outside 1 .. %d" % (xs[-1], name, a.max_length))
    return xs[-1]


def _calls(Ti, nch, device):
    """Ti as [ncalls][nch] on the device; (tensor, whether the caller passed one call as a vector)."""
    t = _f64(Ti, device)
    single = t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1 and nch != 1)
    if single:
        t = t.reshape(1, -1)
    if t.dim() != 2 or t.shape[1] != nch:
        raise ValueError("Ti must hold one arrival time per channel (%d), got %s" % (nch, tuple(t.shape)))
    return t, single


def _first_guess(first_guess, ncalls, device):
    """first_guess ([4] for every call, or [ncalls x 4]) as [ncalls x 4] on the device; None stays None."""
    if first_guess is None:
        return None
    fg = _f64(first_guess, device)
    if fg.dim() == 1:
        fg = fg.reshape(1, -1).expand(ncalls, -1).contiguous()
    if tuple(fg.shape) != (ncalls, 4):
        raise ValueError("first_guess must be [x, y, z, t0] per call (%d x 4), got %s" % (ncalls, tuple(fg.shape)))
    return fg


def _solve(t, cable, c0, Nbiter, fix_z, first_guess):
    """The kernel on [ncalls][nch]: history, n, G^T G, sum of squared residuals, pick count (device tensors)."""
    ncalls, nch = t.shape
    p = 3 if fix_z else 4
    Nbiter = int(Nbiter)
    if Nbiter < 0:
        raise ValueError("Nbiter must not be negative")
    d = t.device
    fg = _first_guess(first_guess, ncalls, d)
    with torch.cuda.device(d):
        hist = torch.empty((ncalls, Nbiter, 4), dtype=torch.float64, device=d)
        n = torch.empty((ncalls, 4), dtype=torch.float64, device=d)
        gtg = torch.empty((ncalls, p, p), dtype=torch.float64, device=d)
        ssr = torch.empty((ncalls,), dtype=torch.float64, device=d)
        npick = torch.empty((ncalls,), dtype=torch.int32, device=d)
        _lib.check(_lib.lib.d4w_loc_solve_f64(dev.ptr(cable), nch, dev.ptr(t), ncalls, float(c0), Nbiter, int(bool(fix_z)),
                                              _p(fg), dev.out_ptr(hist) if Nbiter else None, dev.out_ptr(n), dev.out_ptr(gtg),
                                              dev.out_ptr(ssr), dev.out_ptr(npick), dev.stream_ptr(t)))
    return hist, n, gtg, ssr, npick


def _covariance(gtg, var, quiet=False):
    """loc.py:183-189 on the host for [ncalls][p][p] and [ncalls]: var inv(G^T G), or var inv(G^T G + lambda I) where
    cond(G^T G) exceeds 1 / eps (the reference prints 'Matrix is singular' there)."""
    gtg = np.asarray(gtg, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    p = gtg.shape[-1]
    cov = np.full(gtg.shape, np.nan)
    for k in range(gtg.shape[0]):
        a = gtg[k]
        if not np.all(np.isfinite(a)):
            continue
        with np.errstate(all="ignore"):
            cond = np.linalg.cond(a)
        if not cond <= 1 / sys.float_info.epsilon:
            if not quiet:
                print('Matrix is singular')
            a = a + LAMBDA_REG * np.eye(p)
        cov[k] = var[k] * np.linalg.inv(a)
    return cov


def _stats(gtg, ssr, count, p, count_name, given):
    """The statistics the two batched solvers share, from the kernel's G^T G, sum of squared residuals and channel count per
    call: variance, covariance, uncertainty and the count under the solver's own name, in the callers' container (_back)."""
    cnt = count.cpu().numpy().astype(np.int64)
    with np.errstate(all="ignore"):
        var = np.where(cnt > p, ssr.cpu().numpy() / np.maximum(cnt - p, 1), np.nan)
        cov = _covariance(np.where((cnt > 0)[:, None, None], gtg.cpu().numpy(), np.nan), var, quiet=True)
        unc = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
    stats = {"variance": var, "covariance": cov, "uncertainty": unc, count_name: cnt}
    return {k: _back(torch.from_numpy(np.ascontiguousarray(v)).to(gtg.device), *given) for k, v in stats.items()}


# ------------------------------------------------------------------------------------------
# the reference's functions
# ------------------------------------------------------------------------------------------
def calc_arrival_times(t0, cable_pos, pos, c0):
    """Theoretical arrival times of a call emitted at `t0` from `pos` = [x, y, z] at every channel (loc.py:13-25).  Beyond the
    reference: `pos` = [npos x 3] with `t0` a scalar or [npos] gives [npos x channel] in one launch."""
    nch, npos, single = _channels(cable_pos), _npos(pos, t0), len(_shape(pos)) == 1
    cable = _f64(cable_pos, _device_of(cable_pos, pos, t0))
    p, t = _positions(pos, t0, cable.device)
    out = torch.empty((npos, nch), dtype=torch.float64, device=cable.device)
    with torch.cuda.device(cable.device):
        for a in range(0, npos, _MAX_GRID_Z):
            b = min(npos, a + _MAX_GRID_Z)
            _lib.check(_lib.lib.d4w_loc_arrival_times_f64(dev.ptr(cable), nch, dev.ptr(p[a:b]), dev.ptr(t[a:b]), b - a, float(c0),
                                                          dev.out_ptr(out[a:b]), dev.stream_ptr(cable)))
    out = out[0] if single else out
    return _back(out, cable_pos, pos, t0)


def _host_or_device(cable_pos, whale_pos):
    """(cable, whale, on_device) for the per-channel helpers: NumPy float64 on the host, or float64 tensors on the device."""
    if dev.is_tensor(cable_pos) or dev.is_tensor(whale_pos):
        device = _device_of(cable_pos, whale_pos)
        if device is None:
            c, w = torch.as_tensor(cable_pos, dtype=torch.float64), torch.as_tensor(whale_pos, dtype=torch.float64)
        else:
            c, w = _f64(cable_pos, device), _f64(whale_pos, device)
        return c, w, True
    return np.asarray(cable_pos, dtype=np.float64), np.asarray(whale_pos, dtype=np.float64), False


def calc_distance_matrix(cable_pos, whale_pos):
    """Distance between every channel and the whale (loc.py:28-32)."""
    c, w, t = _host_or_device(cable_pos, whale_pos)
    d2 = ((c - w[:3]) ** 2).sum(1)
    return torch.sqrt(d2) if t else np.sqrt(d2)


def calc_radii_matrix(cable_pos, whale_pos):
    """Horizontal distance between every channel and the whale (loc.py:35-39)."""
    c, w, t = _host_or_device(cable_pos, whale_pos)
    r2 = ((c[:, :2] - w[:2]) ** 2).sum(1)
    return torch.sqrt(r2) if t else np.sqrt(r2)


def calc_theta_vector(cable_pos, whale_pos):
    """Elevation angle between every channel and the whale, atan2(|z_w - z_c|, r) (loc.py:42-47)."""
    c, w, t = _host_or_device(cable_pos, whale_pos)
    r = calc_radii_matrix(c, w)
    return torch.atan2(torch.abs(w[2] - c[:, 2]), r) if t else np.arctan2(np.abs(w[2] - c[:, 2]), r)


def calc_phi_vector(cable_pos, whale_pos):
    """Azimuth from every channel to the whale, atan2(y_w - y_c, x_w - x_c) (loc.py:50-54)."""
    c, w, t = _host_or_device(cable_pos, whale_pos)
    return torch.atan2(w[1] - c[:, 1], w[0] - c[:, 0]) if t else np.arctan2(w[1] - c[:, 1], w[0] - c[:, 0])


def solve_lq(Ti, cable_pos, c0, Nbiter=10, fix_z=False, *, first_guess=None, verbose=True):
    """Least-squares position and emission time [x, y, z, t0] of one call (loc.py:57-128), csrc/loc.hip with one call.

    first_guess: [x, y, z, t0]; None = the reference's [40000, 23000, -60, min(Ti)].  verbose prints the reference's line per
    iteration.  The inputs are not modified."""
    cable = _cable(cable_pos, _device_of(Ti, cable_pos))
    t, _ = _calls(Ti, cable.shape[0], cable.device)
    if t.shape[0] != 1:
        raise ValueError("solve_lq takes one call; solve_lq_batch takes [ncalls x channel]")
    hist, n, _, _, _ = _solve(t, cable, c0, Nbiter, fix_z, first_guess)
    if verbose:
        for j, h in enumerate(hist[0].cpu().numpy()):
            print(f'Iteration {j+1}: x = {h[0]:.4f} m, y = {h[1]:.4f}, z = {h[2]:.4f}, ti = {h[3]:.4f}')
    return _back(n[0], Ti, cable_pos)


def cal_variance_residuals(arrtimes, predic_arrtimes, fix_z=False):
    """Variance of the arrival-time residuals with the reference's 1 / (n - 4), 1 / (n - 3) with fix_z (loc.py:131-153)."""
    residuals = arrtimes - predic_arrtimes
    var = 1 / (len(residuals) - (3 if fix_z else 4)) * (residuals ** 2).sum()
    return var


def calc_covariance_matrix(cable_pos, whale_pos, c0, var, fix_z=False):
    """Covariance of the estimated position (loc.py:156-191): var inv(G^T G) with G at `whale_pos` over every channel of
    `cable_pos` (the kernel's G^T G), regularised as the reference does where cond(G^T G) > 1 / eps."""
    cable = _cable(cable_pos, _device_of(cable_pos, whale_pos))
    w = _f64(whale_pos, cable.device).reshape(-1)
    if w.numel() < 3:
        raise ValueError("whale_pos must be [x, y, z] or [x, y, z, t0]")
    n0 = torch.zeros((1, 4), dtype=torch.float64, device=cable.device)
    n0[0, :3] = w[:3]
    t = torch.zeros((1, cable.shape[0]), dtype=torch.float64, device=cable.device)
    _, _, gtg, _, _ = _solve(t, cable, c0, 0, fix_z, n0)
    v = var.item() if dev.is_tensor(var) else float(var)
    cov = _covariance(gtg.cpu().numpy(), np.array([v]))[0]
    if dev.is_tensor(cable_pos) or dev.is_tensor(whale_pos):
        return _back(torch.from_numpy(cov).to(cable.device), cable_pos, whale_pos)
    return cov


def calc_uncertainty_position(cable_pos, whale_pos, c0, var, fix_z=False):
    """Uncertainties of the estimated position: sqrt of the covariance's diagonal (loc.py:194-217)."""
    cov = calc_covariance_matrix(cable_pos, whale_pos, c0, var, fix_z)
    return torch.sqrt(torch.diagonal(cov)) if dev.is_tensor(cov) else np.sqrt(np.diag(cov))


# ------------------------------------------------------------------------------------------
# beyond the reference: batches and the misfit grid
# ------------------------------------------------------------------------------------------
def solve_lq_batch(Ti, cable_pos, c0, Nbiter=10, fix_z=False, first_guess=None, return_stats=False):
    """solve_lq for [ncalls x channel] arrival times at once, one workgroup per call; NaN = no pick on that channel.

    Returns n [ncalls x 4]; a call without a pick is a NaN row.  first_guess: [4] for every call, [ncalls x 4], or None for
    the reference's.  With return_stats also a dict, per call and evaluated at n over the picked channels:
      history     [ncalls x Nbiter x 4]  the iterate after every iteration
      variance    [ncalls]               sum of squared residuals / (npicks - p), p = 3 with fix_z else 4; NaN where npicks <= p
      covariance  [ncalls x p x p]       variance inv(G^T G), by the reference's rule (regularised where cond > 1 / eps);
                                         computed on the host from the kernel's G^T G
      uncertainty [ncalls x p]           sqrt of the covariance's diagonal
      npicks      [ncalls]               channels that carry a pick"""
    cable = _cable(cable_pos, _device_of(Ti, cable_pos))
    t = _f64(Ti, cable.device)
    if t.dim() != 2 or t.shape[1] != cable.shape[0]:
        raise ValueError("Ti must be [ncalls x channel] with %d channels, got %s" % (cable.shape[0], tuple(t.shape)))
    hist, n, gtg, ssr, npick = _solve(t, cable, c0, Nbiter, fix_z, first_guess)
    if not return_stats:
        return _back(n, Ti, cable_pos)
    stats = _stats(gtg, ssr, npick, 3 if fix_z else 4, "npicks", (Ti, cable_pos))
    stats["history"] = _back(hist, Ti, cable_pos)
    return _back(n, Ti, cable_pos), stats


def _misfit(Ti, cable_pos, c0, xs, ys, z):
    """misfit_grid on the device, shared with first_guess_grid: (gx, gy, whether one call came as a vector, rms, t0 as
    [ncalls x ny x nx])."""
    cable = _cable(cable_pos, _device_of(Ti, cable_pos))
    t, single = _calls(Ti, cable.shape[0], cable.device)
    gx, gy = _f64(xs, cable.device).reshape(-1), _f64(ys, cable.device).reshape(-1)
    ncalls, nch = t.shape
    rms = torch.empty((ncalls, gy.numel(), gx.numel()), dtype=torch.float64, device=cable.device)
    t0 = torch.empty_like(rms)
    with torch.cuda.device(cable.device):
        for a in range(0, max(ncalls, 1), _MAX_GRID_Z):
            b = min(ncalls, a + _MAX_GRID_Z)
            _lib.check(_lib.lib.d4w_loc_misfit_grid_f64(dev.ptr(cable), nch, dev.ptr(t[a:b]), b - a, float(c0), dev.ptr(gx), gx.numel(),
                                                        dev.ptr(gy), gy.numel(), float(z), dev.out_ptr(rms[a:b]),
                                                        dev.out_ptr(t0[a:b]), dev.stream_ptr(cable)))
    return gx, gy, single, rms, t0


def misfit_grid(Ti, cable_pos, c0, xs, ys, z):
    """For every call and every node (xs[ix], ys[iy], z): the best emission time t0 = mean over the picked channels of
    Ti - distance / c0, and the RMS residual once it is removed.  Returns (rms, t0), each [ncalls x ny x nx] ([ny x nx] for
    one call given as a vector).  The minimum of rms is the first guess solve_lq needs (first_guess_grid)."""
    _, _, single, rms, t0 = _misfit(Ti, cable_pos, c0, xs, ys, z)
    if single:
        rms, t0 = rms[0], t0[0]
    return _back(rms, Ti, cable_pos), _back(t0, Ti, cable_pos)


def first_guess_grid(Ti, cable_pos, c0, xs, ys, z):
    """The node of smallest RMS misfit per call as [x, y, z, t0] ([ncalls x 4], or [4] for one call given as a vector), ready to
    pass as `first_guess`.  A call without a pick gives a NaN row."""
    gx, gy, single, rms, t0 = _misfit(Ti, cable_pos, c0, xs, ys, z)
    ncalls = rms.shape[0]
    flat = torch.nan_to_num(rms.reshape(ncalls, -1), nan=float("inf"))
    k = torch.argmin(flat, dim=1)
    out = torch.stack([gx[k % gx.numel()], gy[k // gx.numel()], torch.full_like(gx[k % gx.numel()], float(z)),
                       t0.reshape(ncalls, -1).gather(1, k[:, None])[:, 0]], dim=1)
    out[torch.isnan(out[:, 3])] = float("nan")
    return _back(out[0] if single else out, Ti, cable_pos)


# ------------------------------------------------------------------------------------------
# beyond the reference: association of picks into calls (csrc/assoc.hip)
# ------------------------------------------------------------------------------------------
def _pick_table(picks, nch):
    """The picks as an object of packed [2 x K] int64 ordered by (channel, sample), counts [nch] int32, order (None, or the
    positions in the caller's table of the rows of `packed`) and on_device (a device form came in).  A PickRows stays on the
    device; every other form is a small host table, checked and sorted here and still on the host."""
    from .detect import PickRows, convert_pick_times
    if isinstance(picks, PickRows):
        packed, counts = picks.packed, picks.counts.to(torch.int32)
        if counts.numel() > nch:
            raise ValueError("the picks cover %d channels, cable_pos has %d" % (counts.numel(), nch))
        if counts.numel() < nch:
            counts = torch.cat([counts, counts.new_zeros(nch - counts.numel())])
        return SimpleNamespace(packed=packed.contiguous(), counts=counts.contiguous(), order=None, on_device=True)
    on_device = dev.is_tensor(picks) or (isinstance(picks, tuple) and any(dev.is_tensor(p) for p in picks))
    if isinstance(picks, tuple) and len(picks) == 2:                      # what select_picked_times returns
        picks = [p.cpu().numpy() if dev.is_tensor(p) else np.asarray(p) for p in picks]
        tab = np.stack([np.asarray(p).reshape(-1) for p in picks]) if len(picks[0]) else np.zeros((2, 0))
    elif dev.is_tensor(picks):
        tab = picks.cpu().numpy()
    elif isinstance(picks, np.ndarray) and picks.dtype != object:
        tab = picks
    else:                                                                  # a ragged list of per-channel index arrays
        if len(picks) > nch:
            raise ValueError("the picks cover %d channels, cable_pos has %d" % (len(picks), nch))
        tab = convert_pick_times([p.cpu().numpy() if dev.is_tensor(p) else p for p in picks])
    if tab.ndim != 2 or tab.shape[0] != 2:
        raise ValueError("picks must be a PickRows, a 2 x K table (channel, sample), that pair as a tuple, or a list of "
                         "per-channel index arrays; got an array of shape %s" % (tuple(tab.shape),))
    if tab.size and tab.dtype.kind not in "iu":
        raise ValueError("the pick table must hold integers (channel and sample indices), got %s" % tab.dtype)
    tab = tab.astype(np.int64)
    if tab.shape[1] and (tab[0].min() < 0 or tab[0].max() >= nch):
        raise ValueError("channel indices must lie within 0 .. %d" % (nch - 1))
    order = None
    key = tab[0] * (1 << 40) + tab[1] if tab.shape[1] and np.abs(tab[1]).max() < (1 << 40) else None
    if tab.shape[1] > 1 and (key is None or np.any(np.diff(key) < 0)):
        order = np.lexsort((tab[1], tab[0]))                               # stable: equal picks keep the caller's order
        tab = tab[:, order]
    counts = np.bincount(tab[0], minlength=nch).astype(np.int32)
    return SimpleNamespace(packed=torch.from_numpy(np.ascontiguousarray(tab)), counts=torch.from_numpy(counts), order=order,
                           on_device=on_device)


def _assoc_range(packed, fs, cable, c0, gx, gy, z, dt, t0_range):
    """The bin range as an object of lo, nbins and edges (float64 ndarray).  The default range reads the table's extreme samples
    and the small arrays on the host: lo = min t - Dmax / c0, hi = max t, Dmax = the largest distance between the 8 corners of
    the cable's bounding box and the 4 corners of the grid rectangle at depth z.  Without picks the default takes
    min t = max t = 0."""
    if t0_range is not None:
        lo, hi = (float(v) for v in t0_range)
    else:
        if packed.shape[1]:
            imin, imax = (int(v) for v in torch.stack(torch.aminmax(packed[1])).cpu())
        else:
            imin = imax = 0
        c, x, y = cable.cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy()
        dmax = 0.0
        for cx in (c[:, 0].min(), c[:, 0].max()):
            for cy in (c[:, 1].min(), c[:, 1].max()):
                for cz in (c[:, 2].min(), c[:, 2].max()):
                    for px in (x.min(), x.max()):
                        for py in (y.min(), y.max()):
                            dmax = max(dmax, float(np.sqrt((cx - px) ** 2 + (cy - py) ** 2 + (cz - z) ** 2)))
        lo, hi = imin / fs - dmax / c0, imax / fs
    if not (np.isfinite(lo) and np.isfinite(hi) and hi >= lo):
        raise ValueError("t0_range must be finite with lo <= hi")
    nbins = int(np.ceil((hi - lo) / dt)) + 1
    if nbins < 2:
        raise ValueError("the emission-time range [%g, %g] gives %d bin of %g s; the pair score needs two" % (lo, hi, nbins, dt))
    return SimpleNamespace(lo=lo, nbins=nbins, edges=lo + dt * np.arange(nbins + 1))


def _assoc_setup(picks, fs, cable_pos, c0, xs, ys, z, dt, t0_range):
    """(the shared arguments with z and dt, the pick table on their device, the bin range)."""
    a = _check(cable_pos, c0, fs, xs=xs, ys=ys)
    a.z, a.dt = float(z), float(dt)
    _pos_finite(dt=a.dt)
    t = _pick_table(picks, a.nch)
    _upload(a, device=t.counts.device if t.counts.is_cuda else _device_of(picks))
    a.as_tensor = a.as_tensor or t.on_device
    t.packed, t.counts = t.packed.to(a.device), t.counts.to(a.device)
    return a, t, _assoc_range(t.packed, a.fs, a.cable, a.c0, a.gx, a.gy, a.z, a.dt, t0_range)


def _vote(packed, idx, sign, accumulate, cable, fs, c0, gx, gy, z, lo, dt, nbins, votes, stop):
    K = packed.shape[1]
    _lib.check(_lib.lib.d4w_assoc_vote_i32(dev.ptr(packed) if K else None, K, _p(idx), idx.numel() if idx is not None else 0, sign,
                                           accumulate, dev.ptr(cable), cable.shape[0], fs, c0, dev.ptr(gx), gx.numel(), dev.ptr(gy),
                                           gy.numel(), z, lo, dt, nbins, dev.out_ptr(votes), _p(stop), dev.stream_ptr(cable)))


def vote_grid(picks, fs, cable_pos, c0, xs, ys, z, dt, t0_range=None):
    """Delay-and-vote of picks over the nodes (xs[ix], ys[iy], z): votes[iy, ix, b] counts the picks (channel ch, sample i)
    whose emission time e = i / fs - |cable_pos[ch] - node| / c0 falls into bin b = floor((e - lo) / dt); the picks of one
    call pile up in one bin at the node nearest its source.  Returns (votes [ny x nx x nbins] int32, edges [nbins + 1]
    float64 = lo + dt arange(nbins + 1)).

    picks: a detect.PickRows (stays on the device), a 2 x K integer table (channel, sample) as detect.convert_pick_times
    returns, the tuple detect.select_picked_times returns, or a list of per-channel index arrays.  t0_range = (lo, hi) sets
    the emission times covered; None: lo = earliest pick - Dmax / c0, hi = latest pick, Dmax the largest distance between
    the corners of the cable's bounding box and of the grid.  nbins = ceil((hi - lo) / dt) + 1.  Picks whose bin falls
    outside are not counted.  NumPy in -> NumPy out; a CUDA tensor or PickRows in -> tensors on that device."""
    a, t, r = _assoc_setup(picks, fs, cable_pos, c0, xs, ys, z, dt, t0_range)
    with torch.cuda.device(a.device):
        votes = torch.empty((a.ny, a.nx, r.nbins), dtype=torch.int32, device=a.device)
        _vote(t.packed, None, 1, 0, a.cable, a.fs, a.c0, a.gx, a.gy, a.z, r.lo, a.dt, r.nbins, votes, None)
    return _out(votes, a.as_tensor), (torch.from_numpy(r.edges).to(a.device) if a.as_tensor else r.edges)


def associate_picks(picks, fs, cable_pos, c0, xs, ys, z, dt, min_picks, max_calls=64, t0_range=None, return_votes=False):
    """Group picks into calls by a greedy delay-and-vote over the nodes (xs[ix], ys[iy], z); see vote_grid for `picks`, the
    bins and `t0_range`.  Up to `max_calls` rounds:
      1. the node g* and bin b* of the largest pair score votes[g][b] + votes[g][b + 1] (ties: the smallest flat index
         g (nbins - 1) + b); stop when it is below `min_picks`;
      2. per channel, of its unassigned picks in bins b*, b* + 1 at g*, the one whose emission time is nearest the window
         centre lo + (b* + 1) dt (ties: the earlier row of the table) becomes the call's arrival time on that channel;
      3. the chosen picks' votes are taken off every node.
    Returns (Ti [ncalls x channel] float64 with NaN = no pick, what solve_lq_batch takes; info) with info a dict of
      first_guess [ncalls x 4]  x, y, z of the node and the mean emission time of the chosen picks: solve_lq_batch's first_guess
      node, bin, score, npicks [ncalls] int32: flat node index iy nx + ix, b*, the pair score, channels chosen
      assigned [K] int32       per pick, in the caller's order: the call it went to, 1-based; 0 = none
      edges [nbins + 1]        bin edges of the emission time
      votes [ny x nx x nbins]  with return_votes: the accumulator after the last round = vote_grid of the unassigned picks
    All rounds are enqueued at once; the call synchronises with the host once, for the number of calls found (and, with
    t0_range = None, once before the first round for the extreme pick times)."""
    if int(min_picks) < 1:
        raise ValueError("min_picks must be at least 1")
    if int(max_calls) < 0:
        raise ValueError("max_calls must not be negative")
    min_picks, max_calls = int(min_picks), int(max_calls)
    a, t, r = _assoc_setup(picks, fs, cable_pos, c0, xs, ys, z, dt, t0_range)
    d, nch, nx, ny, nbins, packed, K = a.device, a.nch, a.nx, a.ny, r.nbins, t.packed, t.packed.shape[1]
    lib = _lib.lib
    with torch.cuda.device(d):
        stream = dev.stream_ptr(a.cable)
        votes = torch.empty((ny, nx, nbins), dtype=torch.int32, device=d)
        Ti = torch.empty((max_calls, nch), dtype=torch.float64, device=d)
        fg = torch.empty((max_calls, 4), dtype=torch.float64, device=d)
        rec = torch.zeros((max_calls, 4), dtype=torch.int32, device=d)
        state = torch.zeros(2, dtype=torch.int32, device=d)
        assigned = torch.zeros(K, dtype=torch.int32, device=d)
        chosen = torch.empty(nch, dtype=torch.int32, device=d)
        e_chosen = torch.empty(nch, dtype=torch.float64, device=d)
        off = torch.empty(nch, dtype=torch.int64, device=d)
        summ = torch.empty(2, dtype=torch.int64, device=d)
        ws = torch.empty(lib.d4w_assoc_best_ws_bytes(), dtype=torch.uint8, device=d)

        def vote(idx, sign, accumulate, stop):
            _vote(packed, idx, sign, accumulate, a.cable, a.fs, a.c0, a.gx, a.gy, a.z, r.lo, a.dt, nbins, votes, stop)

        _lib.check(lib.d4w_pick_offsets_i64(dev.ptr(t.counts), nch, dev.out_ptr(off), dev.out_ptr(summ), stream))
        vote(None, 1, 0, None)
        for c in range(max_calls if K else 0):                   # no host synchronisation and no torch kernel in here
            _lib.check(lib.d4w_assoc_best_i32(dev.ptr(votes), nx, ny, nbins, min_picks, c, dev.out_ptr(state), dev.out_ptr(rec),
                                              dev.out_ptr(ws), stream))
            _lib.check(lib.d4w_assoc_select_f64(dev.ptr(packed), K, dev.ptr(off), dev.ptr(a.cable), nch, a.fs, a.c0, dev.ptr(a.gx), nx,
                                                dev.ptr(a.gy), ny, a.z, r.lo, a.dt, nbins, c, dev.ptr(state), dev.out_ptr(rec),
                                                dev.out_ptr(assigned), dev.out_ptr(Ti), dev.out_ptr(chosen), dev.out_ptr(e_chosen),
                                                dev.out_ptr(fg), stream))
            vote(chosen, -1, 1, state)
        ncalls = int(state[1].item()) if K and max_calls else 0  # the call's one host read
        if t.order is not None:
            inv = torch.empty(K, dtype=torch.int64, device=d)
            inv[torch.from_numpy(t.order).to(d)] = torch.arange(K, dtype=torch.int64, device=d)
            assigned = assigned[inv]                             # row j of the caller's table is row inv[j] of the sorted one
    info = {"first_guess": fg[:ncalls], "node": rec[:ncalls, 0].contiguous(), "bin": rec[:ncalls, 1].contiguous(),
            "score": rec[:ncalls, 2].contiguous(), "npicks": rec[:ncalls, 3].contiguous(), "assigned": assigned,
            "edges": torch.from_numpy(r.edges).to(d)}
    if return_votes:
        info["votes"] = votes
    return _out(Ti[:ncalls], a.as_tensor), {k: _out(v, a.as_tensor) for k, v in info.items()}


# ------------------------------------------------------------------------------------------
# beyond the reference: delay-and-sum stack of envelopes on the position grid (csrc/stack.hip)
# ------------------------------------------------------------------------------------------
def _delays(a, z):
    d = torch.empty((a.ny, a.nx, a.nch), dtype=torch.int32, device=a.device)
    _lib.check(_lib.lib.d4w_stack_delays_i32(dev.ptr(a.cable), a.nch, a.c0, a.fs, dev.ptr(a.gx), a.nx, dev.ptr(a.gy), a.ny, z,
                                             dev.out_ptr(d), dev.stream_ptr(a.cable)))
    return d


def delay_table(cable_pos, c0, fs, xs, ys, z):
    """Travel times in samples from every node (xs[ix], ys[iy], z) to every channel, int32 [ny x nx x channel]:
    d = floor(|cable_pos[ch] - node| (1 / c0) fs + 0.5) in float64.  The table stack_grid sums along; it depends on the
    geometry and the rate only, so keep it for the consecutive files of one cable (stack_grid(..., delays=table))."""
    z = float(z)
    a = _upload(_check(cable_pos, c0, fs, xs=xs, ys=ys))
    with torch.cuda.device(a.device):
        d = _delays(a, z)
    return _out(d, a.as_tensor)


def _stack(e, pitch, table, w, nx, ny, k0, k1, normalize, form=0):
    """The kernel on device tensors: (stack [ny x nx x (k1 - k0)], info int32 [2] = form that ran, largest tile spread)."""
    nch, ns = e.shape
    out = torch.empty((ny, nx, k1 - k0), dtype=torch.float32, device=e.device)
    info = torch.empty(2, dtype=torch.int32, device=e.device)
    _lib.check(_lib.lib.d4w_stack_grid_f32(dev.ptr(e), pitch, nch, ns, dev.ptr(table), _p(w), nx, ny, k0, k1, int(bool(normalize)), form,
                                           dev.out_ptr(out), dev.out_ptr(info), dev.stream_ptr(e)))
    return out, info


def _stack_grid(env, fs, cable_pos, c0, xs, ys, z, weights, k_range, normalize, delays=None):
    """stack_grid on the device, shared with locate_stack: (the arguments with z, stack [ny x nx x nt], times as an ndarray)."""
    k0, k1 = (0, None) if k_range is None else (int(k_range[0]), int(k_range[1]))
    if k_range is not None and not k0 < k1:
        raise ValueError("k_range = (k0, k1) must have k0 < k1, got (%d, %d)" % (k0, k1))
    a = _check(cable_pos, c0, fs, block=env, weights=weights, xs=xs, ys=ys)
    a.z = float(z)
    if delays is not None and _shape(delays) != (a.ny, a.nx, a.nch):
        raise ValueError("delays must be [ny x nx x channel] = %s, got %s" % ((a.ny, a.nx, a.nch), _shape(delays)))
    _upload(a, like=(delays,))
    k1 = a.ns if k1 is None else k1
    with torch.cuda.device(a.device):
        if delays is None:
            table = _delays(a, a.z)
        else:
            table = (delays if dev.is_tensor(delays) else torch.from_numpy(np.ascontiguousarray(delays))).to(a.device, torch.int32).contiguous()
        stack, _ = _stack(a.e, a.pitch, table, a.w, a.nx, a.ny, k0, k1, normalize)
    return a, stack, np.arange(k0, k1) / a.fs


def stack_grid(env, fs, cable_pos, c0, xs, ys, z, weights=None, k_range=None, normalize=False, *, delays=None):
    """Delay-and-sum (back-projection) of envelopes over the nodes (xs[ix], ys[iy], z):
        stack[iy, ix, k - k0] = sum over ch of weights[ch] env[ch, k + d[iy, ix, ch]],   d = delay_table(...)
    over the channels with weights[ch] != 0 whose sample k + d lies within the record.  A call emitted at sample k from near a
    node adds up coherently there although it stays under a per-channel pick threshold on every channel.  Returns
    (stack [ny x nx x nt] float32, times [nt] float64 = arange(k0, k1) / fs).

    env: [channel x time] float32, e.g. dsp.envelope of a correlogram; a CUDA float32 view with unit column stride is read in
    place (row pitch).  The stack is taken at env's rate: bring env to the rate wanted with dsp.decimate / dsp.resample_poly
    first.  k_range = (k0, k1): emission samples, half open; default (0, ns); k0 may be negative and k1 may exceed ns.
    weights: float32 [channel], None = ones.  A channel of weight 0 is not read at all (dead channels, the NaN rows of
    zero_rows="nan"); a NaN under a non-zero weight propagates into every element it reaches.  normalize: divide every
    element by the sum of the weights of the channels that contributed to it; an element without contributors is 0.
    delays: the table of delay_table for this cable, grid, c0 and fs (built here when None).
    float32 sums in increasing channel order, one thread per element: run-to-run bit-identical.  NumPy in -> NumPy out; a
    CUDA tensor in -> tensors on that device and stream."""
    a, out, times = _stack_grid(env, fs, cable_pos, c0, xs, ys, z, weights, k_range, normalize, delays)
    return _out(out, a.as_tensor), (torch.from_numpy(times).to(a.device) if a.as_tensor else times)


def _best(s):
    nt = s.shape[-1]
    peak = torch.empty(nt, dtype=torch.float32, device=s.device)
    node = torch.empty(nt, dtype=torch.int32, device=s.device)
    _lib.check(_lib.lib.d4w_stack_best_f32(dev.ptr(s), s.numel() // nt, nt, dev.out_ptr(peak), dev.out_ptr(node), dev.stream_ptr(s)))
    return peak, node


def stack_best(stack):
    """Per column of a stack [ny x nx x nt] (or [nodes x nt]): (peak [nt] float32, node [nt] int32), the largest value over the
    nodes and its flat index iy nx + ix.  Ties go to the smallest index; a NaN never wins; a column of NaNs gives (NaN, -1)."""
    if getattr(stack, "ndim", 0) not in (2, 3) or min(stack.shape) < 1:
        raise ValueError("stack must be a non-empty [ny x nx x nt] or [nodes x nt] array")
    s = dev.to_device_f32(stack, _device_of(stack))
    with torch.cuda.device(s.device):
        peak, node = _best(s)
    as_tensor = dev.is_tensor(stack)
    return _out(peak, as_tensor), _out(node, as_tensor)


def _per_channel(threshold, nch):
    """Whether `threshold` is one value per channel rather than a scalar; checked on the host."""
    per_channel = dev.is_tensor(threshold) or np.ndim(threshold) > 0
    if per_channel and _count(threshold) != nch:
        raise ValueError("threshold must be a scalar or one value per channel (%d), got %d" % (nch, _count(threshold)))
    return per_channel


def _arrivals(a, p, t, h, threshold):
    """arrivals_near on the device, shared with locate_stack: Ti [ncalls x nch] for the calls at p [ncalls x 3], t [ncalls]."""
    ncalls = p.shape[0]
    Ti = torch.empty((ncalls, a.nch), dtype=torch.float64, device=a.device)
    if ncalls:
        thr = _f64(threshold, a.device).reshape(-1) if _per_channel(threshold, a.nch) else None
        _lib.check(_lib.lib.d4w_stack_arrivals_f64(dev.ptr(a.e), a.pitch, a.nch, a.ns, a.fs, dev.ptr(a.cable), a.c0, dev.ptr(p), dev.ptr(t), ncalls,
                                                   h, 0.0 if thr is not None else float(threshold), _p(thr), _p(a.w), dev.out_ptr(Ti),
                                                   dev.stream_ptr(a.cable)))
    return Ti


def arrivals_near(env, fs, cable_pos, c0, pos, t0, halfwidth, threshold, weights=None):
    """Per-channel arrival times of calls whose position and emission time are roughly known (a node and a column of
    stack_grid): for call c at pos[c] = (x, y, z) emitted at t0[c], the sample of the largest env[ch] within `halfwidth`
    samples of round(t0 fs) + the travel time in samples (delay_table's function); the earliest of equal maxima, NaNs skipped.
    Returns Ti [ncalls x channel] float64 = sample / fs, NaN where the window misses the record, weights[ch] = 0, or the
    maximum is below `threshold` (a scalar or one value per channel): the form associate_picks returns and solve_lq_batch
    takes.  pos: [ncalls x 3] (or [3] with a scalar t0: one call, Ti still [1 x channel])."""
    h = _whole(halfwidth, "halfwidth", 0)
    a = _check(cable_pos, c0, fs, block=env, weights=weights, pos=pos, t0=t0)
    if a.ncalls:
        _per_channel(threshold, a.nch)
    _upload(a)
    with torch.cuda.device(a.device):
        Ti = _arrivals(a, a.p, a.t, h, threshold)
    return _out(Ti, a.as_tensor)


def locate_stack(env, fs, cable_pos, c0, xs, ys, z, threshold, halfwidth, pick_threshold, max_calls=64, weights=None, k_range=None,
                 normalize=False, return_stack=False):
    """Calls from the delay-and-sum stack, without a per-channel decision before the sum: stack_grid, stack_best, the
    package's peak picker on the one-row trace of best values (detect.pick_times(peak[None, :], threshold): prominence), the
    `max_calls` largest of its peaks in time order, and arrivals_near at their nodes and times with `pick_threshold`.
    Returns (Ti [ncalls x channel] float64, NaN = no arrival; info) with info a dict of
      first_guess [ncalls x 4]  the node's x, y, z and times[column]: what solve_lq_batch(first_guess=...) takes
      node, column [ncalls] int32, value [ncalls] float32: flat node index iy nx + ix, column of the stack, the peak there
      npicks [ncalls] int32     non-NaN entries of each row of Ti
      times [nt]                emission time of every column
      stack, peak, best_node    with return_stack: the results of stack_grid and stack_best
    Without a call Ti is [0 x channel].  The stack, the best node, the picker and the arrivals are the library's kernels; around
    them the call reads the trace of best values, its nodes and the picker's columns back to the host (three small copies, the
    only synchronisations) to choose the `max_calls` peaks there, uploads their nodes and times, and counts `npicks` with a few
    small torch operations on the [ncalls x channel] result.  See stack_grid for env (bring it to the rate wanted with dsp.decimate /
    dsp.resample_poly first), weights, k_range and normalize, arrivals_near for halfwidth and pick_threshold."""
    from . import detect
    max_calls, h = _whole(max_calls, "max_calls", 0), _whole(halfwidth, "halfwidth", 0)
    a, stack, times = _stack_grid(env, fs, cable_pos, c0, xs, ys, z, weights, k_range, normalize)
    d, nx = a.device, a.nx
    with torch.cuda.device(d):
        peak, best_node = _best(stack)
        cols = detect.pick_times(peak[None, :], threshold).packed[1].cpu().numpy()
        peak_h, node_h = peak.cpu().numpy(), best_node.cpu().numpy()
        cols = cols[node_h[cols] >= 0]
        if len(cols) > max_calls:                                # the largest peaks, the earlier of equals
            cols = cols[np.lexsort((cols, -peak_h[cols].astype(np.float64)))[:max_calls]]
        cols = np.sort(cols)
        nodes = node_h[cols].astype(np.int64)
        fg = np.empty((len(cols), 4))
        fg[:, 0], fg[:, 1] = a.gx.cpu().numpy()[nodes % nx], a.gy.cpu().numpy()[nodes // nx]
        fg[:, 2], fg[:, 3] = a.z, times[cols]
        fg_d = torch.from_numpy(fg).to(d)
        Ti = _arrivals(a, fg_d[:, :3].contiguous(), fg_d[:, 3].contiguous(), h, pick_threshold)
        info = {"first_guess": fg_d, "node": torch.from_numpy(nodes.astype(np.int32)).to(d),
                "column": torch.from_numpy(cols.astype(np.int32)).to(d), "value": torch.from_numpy(peak_h[cols]).to(d),
                "npicks": (~torch.isnan(Ti)).sum(1).to(torch.int32), "times": torch.from_numpy(times).to(d)}
        if return_stack:
            info.update(stack=stack, peak=peak, best_node=best_node)
    return _out(Ti, a.as_tensor), {k: _out(v, a.as_tensor) for k, v in info.items()}


# ------------------------------------------------------------------------------------------
# beyond the reference: delay-and-sum beam of the strain toward located calls (csrc/beam.hip)
# ------------------------------------------------------------------------------------------
def beam_limits():
    """(largest ncalls of a call, largest length, channels per summation segment, samples per workgroup) of the beam kernel."""
    a, b, s, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.d4w_beam_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(s)))
    _lib.check(_lib.lib.d4w_beam_tile(ctypes.byref(t)))
    return a.value, b.value, s.value, t.value


def _beam_delays(a, rounded):
    """r (rounded) or (k, f), each [ncalls x nch], for the positions a.p."""
    shape = (a.ncalls, a.nch)
    r = torch.empty(shape, dtype=torch.int32, device=a.device) if rounded else None
    k = None if rounded else torch.empty(shape, dtype=torch.int32, device=a.device)
    f = None if rounded else torch.empty(shape, dtype=torch.float32, device=a.device)
    if a.ncalls:
        _lib.check(_lib.lib.d4w_beam_delays(dev.ptr(a.cable), a.nch, a.c0, a.fs, dev.ptr(a.p), a.ncalls, _p(k, True), _p(f, True), _p(r, True),
                                            dev.stream_ptr(a.cable)))
    return r if rounded else (k, f)


def beam_delays(cable_pos, c0, fs, pos, rounded=False):
    """Travel times in samples from pos[c] = (x, y, z) to every channel, tau = |cable_pos[ch] - pos[c]| (1 / c0) fs in float64
    (delay_table's expression).  pos: [ncalls x 3] or [3] (one call; the tables are still [1 x channel]).
    rounded=False: (k int32, f float32), both [ncalls x channel], k = floor(tau) and f = float32(tau - k) with 0 <= f < 1 (a
    fraction that rounds to 1.0f is carried into k): what beamform(order=1 or 3, delays=...) takes.
    rounded=True: r int32 [ncalls x channel] = floor(tau + 0.5), delay_table's value at an arbitrary position (capped at 2^30, where
    a NaN lands as well): what beamform(order=0, delays=...) takes.
    The tables depend on the geometry, the rate and the positions only.  NumPy in -> NumPy out; a CUDA tensor in -> tensors on that
    device and stream."""
    a = _upload(_check(cable_pos, c0, fs, pos=pos, limits=beam_limits()[:2]))
    with torch.cuda.device(a.device):
        d = _beam_delays(a, bool(rounded))
    return _out(d, a.as_tensor) if rounded else (_out(d[0], a.as_tensor), _out(d[1], a.as_tensor))


def _given_table(t, device):
    t = t if dev.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.to(device).contiguous()


def _tables(a):
    """(k or r, f or None) on the device: the given tables, or beam_delays' for the positions a.p."""
    if a.tables:
        t = [_given_table(t, a.device) for t in a.tables]
        return t[0], (t[1] if a.kind == "kf" else None)
    with torch.cuda.device(a.device):                        # the one launch of _upload: given tables need no device context
        return (_beam_delays(a, True), None) if a.kind == "r" else _beam_delays(a, False)


def _order(order):
    """(order as an int, the kind of delay table it reads along)."""
    if isinstance(order, bool) or order not in (0, 1, 3):
        raise ValueError("order must be 0, 1 or 3, got %r" % (order,))
    return int(order), ("r" if order == 0 else "kf")


def _beam(a, nt, order, normalize):
    """The kernel on device tensors: beam [ncalls x nt] float32; no launch without a call."""
    out = torch.empty((a.ncalls, nt), dtype=torch.float32, device=a.device)
    if not a.ncalls:
        return out
    nbytes = ctypes.c_size_t()
    _lib.check(_lib.lib.d4w_beam_ws_bytes(a.nch, a.ncalls, nt, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=a.device) if nbytes.value else None
    _lib.check(_lib.lib.d4w_beamform_f32(*_record(a), dev.ptr(a.kr), _p(a.f), _p(a.w), dev.ptr(a.s), a.ncalls, nt, order, int(bool(normalize)),
                                         dev.out_ptr(out), _p(ws, True), dev.stream_ptr(a.e)))
    return out


def beamform(trace, fs, cable_pos, c0, pos, start=0, length=None, order=1, weights=None, normalize=False, next_block=None, *, delays=None):
    """Delay-and-sum beam of the strain toward located calls: the waveform of call c as the whole array hears it, every channel
    advanced by its travel time from pos[c] = (x, y, z) and summed (about sqrt(channels) above the noise of one channel),
        beam[c, j] = sum over ch, increasing, of weights[ch] v(ch, start[c] + j + delay[c, ch]),        0 <= j < length
    Returns (beam [ncalls x length] float32, times [ncalls x length] float64 = (start[c] + j) / fs).

    trace: [channel x time] strain; a CUDA float32 view with unit column stride is read in place (row pitch), anything else becomes
    a float32 copy on the device.  pos: [ncalls x 3] or [3], e.g. the first three columns of solve_lq_batch's result.
    start: the first emission sample, an int or [ncalls] ints, e.g. round(t0 fs); may be negative.  length: samples of the beam,
    shared by the calls; default the samples of trace.
    order: 0 = the nearest sample, v = x[ch, n + r], r = beam_delays(rounded=True) (one fmaf per term: a stack_grid term);
    1 = linear, q = n + k, v = (1 - f) x[q] + f x[q + 1] with (k, f) = beam_delays(); 3 = four-point Lagrange on x[q - 1 .. q + 2].
    A term contributes only if all of its taps lie inside the record; everything else adds nothing.
    weights: float32 [channel], None = ones; a channel of weight 0 is not read at all (a NaN row under weight 0 changes nothing), a
    NaN under a non-zero weight propagates.  normalize: divide every element by the sum of the weights of the channels that
    contributed to it; an element without contributors is 0.
    next_block: the next file of the same cable, [channel x ns2], same rules as trace: sample ns + i of a row is next_block[ch, i]
    and the record is ns + ns2 long.  A call emitted in the last seconds of a file reaches the far channels in the next one; without
    next_block those channels drop out of the beam.
    delays: what beam_delays returns for this order (r for 0, (k, f) otherwise), built here when None.
    float32 sums in increasing channel order in fixed segments of beam_limits()[2] channels, the segment partials added in
    increasing order: run-to-run bit-identical, independent of the other calls of the batch and of a power-of-two scaling of trace.
    NumPy in -> NumPy out; a CUDA tensor in -> tensors on that device and stream."""
    order, kind = _order(order)
    a = _check(cable_pos, c0, fs, pos=pos, block=trace, name="trace", next_block=next_block, weights=weights, start=start,
               table=(delays, kind), limits=beam_limits()[:2])
    nt = _whole(a.ns if length is None else length, "length", 1, a.max_length)
    d = _upload(a).device
    with torch.cuda.device(d):
        out = _beam(a, nt, order, normalize)
        # a tensor divisor: a true division (by a Python number torch multiplies with the reciprocal instead)
        times = (a.s.to(torch.float64)[:, None] + torch.arange(nt, dtype=torch.float64, device=d)[None, :]) \
            / torch.full((), a.fs, dtype=torch.float64, device=d)
    return _out(out, a.as_tensor), _out(times, a.as_tensor)


# ------------------------------------------------------------------------------------------
# beyond the reference: arrival times refined by correlating every channel with the beam (csrc/align.hip)
# ------------------------------------------------------------------------------------------
def align_limits():
    """(largest number of calls, largest template length, largest max_lag, channels per workgroup) of the alignment kernel."""
    a, b, m, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.d4w_align_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(m), ctypes.byref(w)))
    return a.value, b.value, m.value, w.value


def refine_arrivals(trace, fs, cable_pos, c0, pos, template, start, max_lag, min_coef=0.0, weights=None, next_block=None, subsample=True,
                    return_all=False, *, delays=None):
    """Arrival times of located calls refined against their own waveform: every channel is correlated with the call's template
    (its beam) over the lags -max_lag .. max_lag around the predicted moveout, and the lag of the largest correlation
    coefficient, moved by a parabola through its two neighbours, becomes the arrival.  With n0 = start[c] + r[c, ch],
    r = beam_delays(rounded=True):
        rho[m] = sum_j template[c, j] trace[ch, n0 + m + j] / sqrt(sum_j template[c, j]^2  sum_j trace[ch, n0 + m + j]^2)
    in float32 for the lags whose L samples all lie inside the record (NaN otherwise; 0 where either energy is 0); m* the lag of
    the largest non-NaN rho (the smallest of equals), coef = rho[m*]; delta = 0.5 (a - c) / (a - 2 b + c) from
    a, b, c = rho[m* - 1 .. m* + 1] in float64, clipped to +-0.5, where both neighbours exist, are not NaN and the denominator is
    negative (else 0; always 0 with subsample=False); Ti[c, ch] = (n0 + m* + delta) / fs.
    Returns (Ti [ncalls x channel] float64, coef [ncalls x channel] float32); Ti is NaN where weights[ch] = 0, where no lag fits the
    record or every rho is NaN, or where coef < min_coef: the form associate_picks and arrivals_near return and solve_lq_batch
    takes, consistent with t0 = start[c] / fs when sample 0 of the template is emission sample start[c] (a beam's is).  With
    return_all also lag [ncalls x channel] int32 (m*; 0 where there is no lag to report) and rho [ncalls x channel x (2 max_lag + 1)]
    float32, the table the pick was read from.

    The adaptive-stacking loop this closes:
        Ti, info = locate_stack(env, fs, cable_pos, c0, xs, ys, z, threshold, halfwidth, pick_threshold)
        n = solve_lq_batch(Ti, cable_pos, c0, fix_z=True, first_guess=info["first_guess"])
        start = round(n[:, 3] fs) - lead
        beam, _ = beamform(trace, fs, cable_pos, c0, n[:, :3], start=start, length=L, order=3)
        Ti2, coef = refine_arrivals(trace, fs, cable_pos, c0, n[:, :3], beam, start, max_lag=4)
        n2 = solve_lq_batch(Ti2, cable_pos, c0, fix_z=True, first_guess=n)
    The last three lines, with coef as the second solve's weights and a robust loss against the channels that skipped a cycle,
    are one call: relocate(trace, fs, cable_pos, c0, n, length=L, max_lag=4, lead=lead) (solve_robust_batch).
    max_lag must stay under half the dominant period of a narrow-band call, or the largest coefficient skips a cycle: on the
    64-channel scene of a 20 Hz burst at 200 Hz (period 10 samples) the arrival-time error about its mean is 0.19 samples with
    max_lag = 4 and 3.4 with max_lag = 10, against 7.9 for envelope-maximum picks (a float64 prototype).

    trace, weights, next_block, start, pos: as for beamform (a CUDA float32 view with unit column stride is read in place; a
    channel of weight 0 is never read, and its Ti, coef and rho are NaN).  template: float32 [ncalls x L], or [L] for one call.
    delays: beam_delays(rounded=True) for these positions, built here when None.  Limits: align_limits().
    The sums are float32 in an order that depends on L alone: run-to-run bit-identical, independent of the other calls of the
    batch, and rho keeps its bits under a power-of-two scaling of trace or template.  NumPy in -> NumPy out; any tensor in ->
    tensors on that device and stream."""
    limits = align_limits()
    a = _check(cable_pos, c0, fs, pos=pos, block=trace, name="trace", next_block=next_block, weights=weights, start=start,
               table=(delays, "r"), limits=limits[:2])
    L, M, min_coef = _waveforms(template, "template", a), _whole(max_lag, "max_lag", 0, limits[2]), _number(min_coef, "min_coef")
    d = _upload(a, like=(template,)).device
    with torch.cuda.device(d):
        Ti = torch.empty((a.ncalls, a.nch), dtype=torch.float64, device=d)
        coef = torch.empty((a.ncalls, a.nch), dtype=torch.float32, device=d)
        lag = torch.empty((a.ncalls, a.nch), dtype=torch.int32, device=d) if return_all else None
        rho = torch.empty((a.ncalls, a.nch, 2 * M + 1), dtype=torch.float32, device=d) if return_all else None
        if a.ncalls:
            t = _given_table(template, d).reshape(a.ncalls, L)
            _lib.check(_lib.lib.d4w_align_f32(*_record(a), dev.ptr(t), L, dev.ptr(a.kr), dev.ptr(a.s), a.ncalls, M, _p(a.w), a.fs, min_coef,
                                              int(bool(subsample)), dev.out_ptr(Ti), dev.out_ptr(coef), _p(lag, True), _p(rho, True),
                                              dev.stream_ptr(a.e)))
    out = (Ti, coef) + ((lag, rho) if return_all else ())
    return tuple(_out(y, a.as_tensor) for y in out)


# ------------------------------------------------------------------------------------------
# beyond the reference: robust weighted relocation (csrc/robust.hip) and the adaptive-stacking loop as one call
# ------------------------------------------------------------------------------------------
_LOSSES = {"l2": (0, 1.0), "huber": (1, 1.345), "bisquare": (2, 4.685)}      # name -> (code of the C ABI, default tuning)
_MAX_NBITER = 100000


def robust_limits():
    """(channels of a call whose |residuals| stay in LDS for the median -- above it they go through a global workspace --,
    bits one pass of the radix select resolves) of the robust solver."""
    a, b = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.d4w_loc_robust_limits(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def _robust_check(Ti, cable_pos, c0, weights, loss, tuning, scale, Nbiter, warmup, first_guess):
    """Every check of solve_robust_batch on the host, before any device work: (nch, ncalls, loss code, tuning, scale or 0.0,
    Nbiter, warmup, whether the weights are per call)."""
    nch = _channels(cable_pos)
    _pos_finite(c0=float(c0))
    ts = _shape(Ti)
    if len(ts) != 2 or ts[1] != nch:
        raise ValueError("Ti must be [ncalls x channel] with %d channels, got %s" % (nch, ts))
    ncalls = ts[0]
    if not isinstance(loss, str) or loss not in _LOSSES:
        raise ValueError("loss must be one of %s, got %r" % (sorted(_LOSSES), loss))
    code, default = _LOSSES[loss]
    for name, v in (("tuning", tuning), ("scale", scale)):
        if v is None:
            continue
        if isinstance(v, bool) or _shape(v) != () or dev.is_tensor(v):
            raise ValueError("%s must be None or a positive finite number, got %r" % (name, v))
        _pos_finite(**{name: float(v)})
    per_call = False
    if weights is not None:
        ws = _shape(weights)
        if ws not in ((nch,), (ncalls, nch)):
            raise ValueError("weights must be [channel] = (%d,) or [ncalls x channel] = %s, got %s" % (nch, (ncalls, nch), ws))
        per_call = len(ws) == 2
    if first_guess is not None and _shape(first_guess) not in ((4,), (ncalls, 4)):
        raise ValueError("first_guess must be [x, y, z, t0] or one per call (%d x 4), got %s" % (ncalls, _shape(first_guess)))
    return (nch, ncalls, code, float(default if tuning is None else tuning), 0.0 if scale is None else float(scale),
            _whole(Nbiter, "Nbiter", 0, _MAX_NBITER), _whole(warmup, "warmup", 0, 2 ** 31 - 1), per_call)


def solve_robust_batch(Ti, cable_pos, c0, weights=None, loss="huber", tuning=None, scale=None, Nbiter=10, warmup=4, fix_z=False,
                       first_guess=None, return_stats=False):
    """solve_lq_batch with per-channel weights and a robust loss, by iteratively reweighted least squares inside the same
    damped Gauss-Newton (csrc/robust.hip, one workgroup per call): the second solve for the arrivals and coefficients of
    refine_arrivals, where a minority of channels is wrong by a whole period, or carries the pick of another call.

    Ti, cable_pos, c0, Nbiter, fix_z, first_guess: as in solve_lq_batch.  weights: None, [channel] or [ncalls x channel]
    (float64), e.g. coef ** 2.  Channel ch of call c is USED iff Ti[c, ch] is not NaN and weights[c, ch] > 0: a NaN, zero or
    negative weight means "not used", and the Ti and the cable row of an unused channel may hold anything.
    loss: "l2", "huber" (tuning 1.345) or "bisquare" (4.685); tuning: the loss's constant in units of the scale.
    scale: the residuals' standard deviation in seconds; None estimates it per call and iteration as 1.4826 x the exact median
    of |r| over the used channels.  warmup: iterations of plain weighted least squares before the robust weights start (the
    first guess may be kilometres off, and the median residual with it).
    Iteration j at n: r = Ti - (n[3] + R / c0); q = 1 for "l2", for j < warmup and where the scale s is not > 0 (a noise-free
    call); otherwise with u = |r| / (tuning s): huber q = 1 (u <= 1), 1 / u; bisquare q = (1 - u^2)^2 (u < 1), 0.
    w = weights q; dn = (sum w g g^T + 1e-5 I)^-1 sum w g r; n += 0.7 dn for j < 4, dn after.

    Returns n [ncalls x 4]; a call without a used channel is a NaN row.  With return_stats also a dict, per call, from one
    more pass at n with q formed as for j >= warmup:
      history        [ncalls x Nbiter x 4]  the iterate after every iteration
      scale          [ncalls]               s; NaN where no q was formed ("l2", no used channel)
      robust_weights [ncalls x channel]     q; NaN on unused channels
      residuals      [ncalls x channel]     r; NaN on unused channels
      nused          [ncalls]               used channels
      weight_sum     [ncalls]               sum of w
      variance       [ncalls]               sum w r^2 / (nused - p), p = 3 with fix_z else 4; NaN where nused <= p
      covariance     [ncalls x p x p]       variance inv(G^T W G), solve_lq_batch's rule (regularised where cond > 1 / eps), on the host
      uncertainty    [ncalls x p]           sqrt of the covariance's diagonal
    Every sum has a fixed order and the median is exact integer work: run-to-run bit-identical and independent of the other
    calls of the batch.  With loss="l2" and weights=None, n and history equal solve_lq_batch's bit for bit.  Limits:
    robust_limits().  A bad argument raises ValueError on the host before any device work.  Containers as solve_lq_batch."""
    nch, ncalls, code, tuning, scale, Nbiter, warmup, per_call = _robust_check(Ti, cable_pos, c0, weights, loss, tuning, scale, Nbiter,
                                                                               warmup, first_guess)
    given = (Ti, cable_pos, weights, first_guess)
    cable = _cable(cable_pos, _device_of(*given))
    d = cable.device
    t = _f64(Ti, d)
    w = _f64(weights, d) if weights is not None else None
    fg = _first_guess(first_guess, ncalls, d)
    p = 3 if fix_z else 4
    lib = _lib.lib
    with torch.cuda.device(d):
        hist = torch.empty((ncalls, Nbiter, 4), dtype=torch.float64, device=d)
        n = torch.empty((ncalls, 4), dtype=torch.float64, device=d)
        gtg = torch.empty((ncalls, p, p), dtype=torch.float64, device=d)
        ssr, wsum, sc = (torch.empty((ncalls,), dtype=torch.float64, device=d) for _ in range(3))
        nused = torch.empty((ncalls,), dtype=torch.int32, device=d)
        q = torch.empty((ncalls, nch), dtype=torch.float64, device=d) if return_stats else None
        r = torch.empty((ncalls, nch), dtype=torch.float64, device=d) if return_stats else None
        nbytes = ctypes.c_size_t()
        _lib.check(lib.d4w_loc_robust_ws_bytes(nch, ncalls, ctypes.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=d) if nbytes.value else None
        if ncalls:                               # (an empty tensor has no pointer to hand over)
            _lib.check(lib.d4w_loc_robust_f64(dev.ptr(cable), nch, dev.ptr(t), ncalls, _p(w), int(per_call), float(c0), Nbiter, warmup,
                                              int(bool(fix_z)), code, tuning, scale, _p(fg), dev.out_ptr(hist) if Nbiter else None,
                                              dev.out_ptr(n), dev.out_ptr(gtg), dev.out_ptr(ssr), dev.out_ptr(wsum), dev.out_ptr(nused),
                                              dev.out_ptr(sc), _p(q, True), _p(r, True), _p(ws, True), dev.stream_ptr(t)))
    if not return_stats:
        return _back(n, *given)
    stats = _stats(gtg, ssr, nused, p, "nused", given)
    stats.update({k: _back(v, *given) for k, v in (("history", hist), ("scale", sc), ("robust_weights", q), ("residuals", r),
                                                    ("weight_sum", wsum))})
    return _back(n, *given), stats


def relocate(trace, fs, cable_pos, c0, n, length, max_lag, lead=0, rounds=1, order=3, loss="huber", tuning=None, coef_power=2.0,
             min_coef=0.0, Nbiter=10, fix_z=True, weights=None, next_block=None, return_stats=False):
    """The adaptive-stacking loop of refine_arrivals' docstring as one call: located calls n [ncalls x 4] = [x, y, z, t0]
    (solve_lq_batch's result) are beamformed, every channel is re-picked against the beam, and the position is solved again
    with the correlation coefficients as weights and a robust loss.  A composition of the package's own calls on the callers'
    device and stream; per round
        start = round(n[:, 3] fs) - lead                                                     (int64, half to even)
        beam, _ = beamform(trace, fs, cable_pos, c0, n[:, :3], start, length, order, weights, next_block=next_block)
        Ti, coef = refine_arrivals(trace, fs, cable_pos, c0, n[:, :3], beam, start, max_lag, min_coef, weights, next_block)
        n = solve_robust_batch(Ti, cable_pos, c0, weights=max(coef, 0) ** coef_power, loss=loss, tuning=tuning, Nbiter=Nbiter,
                               warmup=0, fix_z=fix_z, first_guess=n)
    in float64 for the weights.  coef_power = 0 means unit weights on the channels that have an arrival.  warmup is 0: n is a
    located call, not the default guess.  lead: samples of the beam before the emission sample, so that the template holds
    the call's onset; length: samples of the beam (the call's length + 2 lead).  max_lag: see refine_arrivals -- under half the
    dominant period; the robust loss takes the edge off a cycle skip on a minority of channels, it does not repair a majority.
    weights: float32 [channel] for the beam and the alignment (dead channels: 0).  A NaN row of n (a call without a pick) stays
    a NaN row.  Returns n [ncalls x 4]; with return_stats also a dict of the last round's solver stats (solve_robust_batch)
    and its Ti, coef and beam.  A CUDA float32 trace is read in place every round; a NumPy trace is uploaded by every call."""
    rounds = _whole(rounds, "rounds", 1)
    lead = _whole(lead, "lead", 0)
    if _number(coef_power, "coef_power") < 0:
        raise ValueError("coef_power must not be negative, got %r" % (coef_power,))
    if _shape(n)[1:] != (4,) or len(_shape(n)) != 2:
        raise ValueError("n must be [ncalls x 4] = [x, y, z, t0] per call, got %s" % (_shape(n),))
    if not isinstance(loss, str) or loss not in _LOSSES:
        raise ValueError("loss must be one of %s, got %r" % (sorted(_LOSSES), loss))
    stats = Ti = coef = beam = None
    for _ in range(rounds):
        if dev.is_tensor(n):
            start = torch.nan_to_num(torch.round(n[:, 3].to(torch.float64) * fs), nan=0.0).to(torch.int64) - lead
            pos = n[:, :3]
        else:
            n = np.asarray(n, dtype=np.float64)
            start = np.nan_to_num(np.round(n[:, 3] * fs), nan=0.0).astype(np.int64) - lead
            pos = n[:, :3]
        beam, _t = beamform(trace, fs, cable_pos, c0, pos, start=start, length=length, order=order, weights=weights, next_block=next_block)
        Ti, coef = refine_arrivals(trace, fs, cable_pos, c0, pos, beam, start, max_lag, min_coef=min_coef, weights=weights,
                                   next_block=next_block)
        if dev.is_tensor(coef):
            w = torch.clamp(coef.to(torch.float64), min=0.0) ** float(coef_power)
        else:
            w = np.maximum(coef.astype(np.float64), 0.0) ** float(coef_power)
        out = solve_robust_batch(Ti, cable_pos, c0, weights=w, loss=loss, tuning=tuning, Nbiter=Nbiter, warmup=0, fix_z=fix_z,
                                 first_guess=n, return_stats=return_stats)
        n, stats = out if return_stats else (out, None)
    if not return_stats:
        return n
    stats.update(Ti=Ti, coef=coef, beam=beam)
    return n, stats


# ------------------------------------------------------------------------------------------
# beyond the reference: received level and SNR of located calls per channel (csrc/levels.hip), and a spreading-loss fit
# ------------------------------------------------------------------------------------------
def level_limits():
    """(largest number of calls, largest length -- of the signal window, and of noise_length + gap --, channels per workgroup)
    of the level kernel."""
    a, b, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.d4w_level_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(w)))
    return a.value, b.value, w.value


def _level_check(a, length, noise_length, gap):
    """The arguments only received_levels has, on the host before any device work: (L, N, gap)."""
    L, N = _whole(length, "length", 1, a.max_length), _whole(noise_length, "noise_length", 0, a.max_length)
    gap = _whole(gap, "gap", 0, a.max_length)
    if N + gap > a.max_length:
        raise ValueError("noise_length + gap = %d is more than the %d one launch takes" % (N + gap, a.max_length))
    return L, N, gap


def received_levels(trace, fs, cable_pos, c0, pos, start, length, noise_length=0, gap=0, weights=None, next_block=None, *, delays=None):
    """How loud located calls are on every channel: the mean square of the strain in a window that follows the call's travel
    time, the mean square in a noise window just before the call arrives, and the largest sample of the signal window.  With
    n0 = start[c] + r[c, ch], r = beam_delays(rounded=True):
        signal[c, ch] = mean of trace[ch, n0 + j]^2                      over 0 <= j < length
        noise[c, ch]  = mean of trace[ch, n0 - gap - noise_length + j]^2 over 0 <= j < noise_length
        peak[c, ch]   = max of |trace[ch, n0 + j]|                       over 0 <= j < length       (exact)
    Returns (signal, noise, peak), float32 [ncalls x channel].  A window gives a value only if it lies wholly inside the record,
    NaN otherwise; noise_length = 0 means no noise window (noise is all NaN).  A NaN sample makes its window's mean square NaN,
    and peak is NaN wherever signal is.  levels_db turns the pair into a level and an SNR in dB, fit_spreading fits the
    level against range.

    trace, weights, next_block, start, pos: as for beamform and refine_arrivals (a CUDA float32 view with unit column stride is
    read in place; start an int or [ncalls] ints, e.g. round(t0 fs) - lead; next_block continues the record).  weights is a
    mask here: a channel of weight 0 is never read and its three values are NaN, a non-zero weight scales nothing.
    length, noise_length, gap: whole numbers of samples, length >= 1, the others >= 0.  gap keeps the noise window clear of
    the call's onset.  delays: beam_delays(rounded=True) for these positions, built here when None.  Limits: level_limits().
    To level a band, band-limit trace first (dsp.bp_filt).
    The sums are float32 in an order that depends on the window length alone (64 interleaved chains, added pairwise): run-to-run
    bit-identical, independent of the other calls of the batch, of the alignment of a window and of where next_block begins;
    a scaling of trace by 2^k scales signal and noise by 4^k and peak by 2^k exactly.  A bad argument raises ValueError on the
    host before any device work.  NumPy in -> NumPy out; any tensor in -> tensors on that device and stream."""
    a = _check(cable_pos, c0, fs, pos=pos, block=trace, name="trace", next_block=next_block, weights=weights, start=start,
               table=(delays, "r"), limits=level_limits()[:2])
    L, N, gap = _level_check(a, length, noise_length, gap)
    d = _upload(a).device
    with torch.cuda.device(d):
        signal, noise, peak = (torch.empty((a.ncalls, a.nch), dtype=torch.float32, device=d) for _ in range(3))
        if a.ncalls:
            _lib.check(_lib.lib.d4w_level_f32(*_record(a), dev.ptr(a.kr), dev.ptr(a.s), a.ncalls, L, gap, N, _p(a.w), dev.out_ptr(signal),
                                              dev.out_ptr(noise), dev.out_ptr(peak), dev.stream_ptr(a.e)))
    return tuple(_out(y, a.as_tensor) for y in (signal, noise, peak))


def levels_db(signal, noise=None):
    """received_levels' mean squares in decibels, float64: level_db = 10 log10(signal), and with noise given
    (level_db, snr_db) with snr_db = 10 log10(signal / noise).  IEEE results without warnings: signal 0 gives -inf, noise 0
    gives +inf, 0 / 0 and every NaN give NaN.  On strain the level is relative (dB re 1 strain^2), not a pressure level.
    Small arithmetic on the container it was given: NumPy in -> NumPy out; a tensor in -> tensors on its device."""
    d = _device_of(signal, noise)
    if d is not None:
        s = (signal if dev.is_tensor(signal) else torch.from_numpy(np.asarray(signal))).to(d, torch.float64)
        level = 10.0 * torch.log10(s)
        if noise is None:
            return level
        q = (noise if dev.is_tensor(noise) else torch.from_numpy(np.asarray(noise))).to(d, torch.float64)
        return level, 10.0 * torch.log10(s / q)
    # on the host a tensor goes through the NumPy expressions as well: one result for one input, whatever the container
    back = (lambda v: torch.from_numpy(v)) if dev.is_tensor(signal) or dev.is_tensor(noise) else (lambda v: v)
    s = np.asarray(signal.numpy() if dev.is_tensor(signal) else signal, dtype=np.float64)
    with np.errstate(all="ignore"):
        level = np.asarray(10.0 * np.log10(s))
        if noise is None:
            return back(level)
        q = np.asarray(noise.numpy() if dev.is_tensor(noise) else noise, dtype=np.float64)
        return back(level), back(np.asarray(10.0 * np.log10(s / q)))


def fit_spreading(level_db, cable_pos, pos, snr_db=None, min_snr_db=None):
    """A spreading law through the levels of every call, by ordinary least squares per call:
        level_db[c, ch] = SL[c] - k[c] 10 log10(range[c, ch] / 1 m),        range = |cable_pos[ch] - pos[c]|
    over the channels whose level is finite and, when both snr_db and min_snr_db are given, whose snr_db >= min_snr_db.
    Returns (SL [ncalls] float64, k [ncalls] float64, used [ncalls] int32 = the channels of the fit); SL and k are NaN where
    fewer than two channels remain or all their ranges are equal.  k = 2 for an amplitude that falls as 1 / r (spherical
    spreading), 1 for cylindrical.  On strain SL is a relative level -- the level_db the law gives at 1 m -- and not a source
    level in dB re 1 uPa: nothing here calibrates strain to pressure.
    level_db: [ncalls x channel] (or [channel] for one call), what levels_db returns; pos: [ncalls x 3] or [3].
    Float64, closed form (the two sums of a straight-line fit about the means); small arithmetic on the container level_db
    came in, not a kernel: NumPy in -> NumPy out; a tensor in -> tensors on its device."""
    nch = _channels(cable_pos)
    ncalls = _npos(pos)
    ls = _shape(level_db)
    if ls not in ((ncalls, nch),) + (((nch,),) if ncalls == 1 else ()):
        raise ValueError("level_db must be [ncalls x channel] = %s, got %s" % ((ncalls, nch), ls))
    if snr_db is not None and _shape(snr_db) != ls:
        raise ValueError("snr_db must have level_db's shape %s, got %s" % (ls, _shape(snr_db)))
    if min_snr_db is not None and (isinstance(min_snr_db, bool) or _shape(min_snr_db) != () or np.isnan(min_snr_db)):
        raise ValueError("min_snr_db must be None or a number, got %r" % (min_snr_db,))
    as_tensor = dev.is_tensor(level_db)
    d = level_db.device if as_tensor else "cpu"

    def t64(v):
        v = v if dev.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64)))
        return v.to(d, torch.float64)

    y = t64(level_db).reshape(ncalls, nch)
    p = t64(pos).reshape(ncalls, 3)
    diff = t64(cable_pos)[None, :, :] - p[:, None, :]
    u = 10.0 * torch.log10(torch.sqrt((diff * diff).sum(-1)))
    ok = torch.isfinite(y) & torch.isfinite(u)
    if snr_db is not None and min_snr_db is not None:
        ok &= t64(snr_db).reshape(ncalls, nch) >= float(min_snr_db)
    used = ok.sum(1)
    n = used.to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64, device=y.device)
    um = torch.where(ok, u, zero).sum(1) / n
    ym = torch.where(ok, y, zero).sum(1) / n
    du = torch.where(ok, u - um[:, None], zero)
    suu = (du * du).sum(1)
    suy = (du * torch.where(ok, y - ym[:, None], zero)).sum(1)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=y.device)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=y.device)
    fit = (used >= 2) & (torch.where(ok, u, -inf).amax(1) > torch.where(ok, u, inf).amin(1))      # two channels, two ranges
    k = torch.where(fit, -suy / suu, nan)
    SL = torch.where(fit, ym + k * um, nan)
    used = used.to(torch.int32)
    if as_tensor:
        return SL, k, used
    return SL.numpy(), k.numpy(), used.numpy()


# ------------------------------------------------------------------------------------------
# beyond the reference: the transpose of the beam -- located calls projected onto the channels and subtracted (csrc/project.hip)
# ------------------------------------------------------------------------------------------
def project_limits():
    """(largest number of calls, largest beam length, channels per workgroup of the fit) of the projection kernels."""
    a, b, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.d4w_project_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(w)))
    return a.value, b.value, w.value


def _project_check(a, beam, amp=_SKIP):
    """The arguments only project_calls and subtract_calls have against the shared ones, on the host before any device work:
    the beam's length."""
    if amp is not _SKIP:
        if _shape(amp) not in ((a.ncalls, a.nch),) + (((a.nch,),) if a.ncalls == 1 else ()) or _dtype_name(amp) != "float32":
            raise ValueError("amp must be float32 [ncalls x channel] = %s, got %s %s" % ((a.ncalls, a.nch), _dtype_name(amp), _shape(amp)))
    return _waveforms(beam, "beam", a)


def _check_inplace(inplace, trace, next_block):
    """inplace=True writes into the callers' blocks: they must be what the kernels take as it is, on one device."""
    if inplace and not (_inplace_view(trace) and (next_block is None or _inplace_view(next_block, trace.device))):
        raise ValueError("inplace=True needs trace (and next_block) as CUDA float32 tensors with unit column stride on one device")
    return bool(inplace)


def _project(a, b, order):
    """The fit on device tensors: (amp, coef) float32 [ncalls x nch]; no launch without a call."""
    amp, coef = (torch.empty((a.ncalls, a.nch), dtype=torch.float32, device=a.device) for _ in range(2))
    if a.ncalls:
        _lib.check(_lib.lib.d4w_project_f32(*_record(a), dev.ptr(a.kr), _p(a.f), dev.ptr(b), b.shape[1], dev.ptr(a.s), a.ncalls, order, _p(a.w),
                                            dev.out_ptr(amp), dev.out_ptr(coef), dev.stream_ptr(a.e)))
    return amp, coef


def _subtract(a, b, amp, order, inplace, trace, next_block):
    """The subtraction on device tensors, and its result in the callers' container: the residual, or (residual, residual_next)
    with a next block; in place these are trace and next_block themselves.  Without a call it still launches, with null call
    pointers: out of place the copy has to be written."""
    if inplace:
        y, yn, py, pyn = a.e, a.nb, a.pitch, a.pitch_nb
    else:
        y = torch.empty((a.nch, a.ns), dtype=torch.float32, device=a.device)
        yn = torch.empty((a.nch, a.ns_nb), dtype=torch.float32, device=a.device) if a.nb is not None else None
        py, pyn = a.ns, a.ns_nb
    kr, f, b_, s, amp = (_p(t) if a.ncalls else None for t in (a.kr, a.f, b, a.s, amp))
    _lib.check(_lib.lib.d4w_project_subtract_f32(*_record(a), kr, f, b_, b.shape[1], s, amp, a.ncalls, order, dev.out_ptr(y), py, _p(yn, True),
                                                 pyn, dev.stream_ptr(a.e)))
    if inplace:
        return trace if next_block is None else (trace, next_block)
    return _out(y, a.as_tensor) if yn is None else (_out(y, a.as_tensor), _out(yn, a.as_tensor))


def project_calls(trace, fs, cable_pos, c0, pos, beam, start, order=1, weights=None, next_block=None, *, delays=None):
    """The waveform of located calls projected back onto every channel: the transpose of beamform.  The image of call c on
    channel ch is its beam laid along the call's moveout with the beam's own interpolation taps,
        g[c, ch](n) = sum_m l_m beam[c, n - q0 - m],        q0 = start[c] + delay[c, ch],  beam = 0 outside 0 <= j < L
    (l_m: beamform's coefficients of that order with weight 1; support of L + order samples), and the fit over that support is
        amp[c, ch]  = sum trace g / sum g g                       the least-squares amplitude of the image on the channel
        coef[c, ch] = sum trace g / sqrt(sum g g  sum trace^2)    the correlation coefficient, refine_arrivals' form
    Returns (amp, coef), float32 [ncalls x channel].  amp is signed and coherent -- far less biased by noise than
    received_levels' mean square -- and is what subtract_calls takes; amp is 0 where the image is all zero, coef is 0 where
    either energy is.  NaN in both where the support does not lie wholly inside the record, where a sample of the window is
    NaN, and where weights[ch] = 0 (the channel is never read; a non-zero weight scales nothing: weights is a mask).
    Every fit is against trace as given, independent of the other calls: overlapping calls are not fitted jointly.

    beam: float32 [ncalls x L] (or [L] for one call), e.g. beamform(..., normalize=True)[0] with the same pos, start and order.
    A normalized beam holds 1 / channels of every channel's own noise, so amp and coef of a channel are biased up by about
    (noise energy of the channel) / (channels x energy of the beam) -- negligible on a long cable, visible on a few channels.
    trace, weights, next_block, start, pos, order, delays: as for beamform (a CUDA float32 view with unit column stride is
    read in place; delays is beam_delays' r for order 0 and (k, f) otherwise, built here when None).  Limits: project_limits().
    The sums are float32 in an order that depends on L + order alone (64 interleaved chains, added pairwise): run-to-run
    bit-identical, independent of the batch and of where next_block begins; a scaling of a channel by 2^k scales amp by 2^k
    exactly and keeps coef's bits.  A bad argument raises ValueError on the host before any device work.
    NumPy in -> NumPy out; any tensor in -> tensors on that device and stream."""
    order, kind = _order(order)
    a = _check(cable_pos, c0, fs, pos=pos, block=trace, name="trace", next_block=next_block, weights=weights, start=start,
               table=(delays, kind), limits=project_limits()[:2])
    L = _project_check(a, beam)
    _upload(a, like=(beam,))
    with torch.cuda.device(a.device):
        out = _project(a, _given_table(beam, a.device).reshape(a.ncalls, L), order)
    return tuple(_out(y, a.as_tensor) for y in out)


def subtract_calls(trace, fs, cable_pos, c0, pos, beam, start, amp, order=1, next_block=None, inplace=False, *, delays=None):
    """Located calls taken out of the block, the CLEAN step of array processing:
        residual = trace, then for c = 0, 1, ... in increasing order: residual[ch, n] -= amp[c, ch] g[c, ch](n)
    over the support of the image g (project_calls), one fmaf per sample and call, wherever amp[c, ch] is finite and
    non-zero and the support lies wholly inside the record.  A NaN or zero amp subtracts nothing: mask amp to choose the
    channels (remove_calls does, by coef).  Returns the residual [channel x time] float32, or (residual, residual_next) when
    next_block is given (the part of the record past the seam).  A second pass of locate_stack / beamform / refine_arrivals
    over the residual sees the weaker call the first one hid, and the residual under a call is the noise estimate there.

    inplace=False: new arrays; every sample is written (a copy where no call reaches).  inplace=True: trace (and next_block)
    must be CUDA float32 tensors with unit column stride -- views into larger buffers are fine --; they are written into and
    returned, only the samples under a support are touched, and the result has the same bits as out of place.
    beam, start, order, delays: as for project_calls; amp: float32 [ncalls x channel] (or [channel] for one call).
    A gather without atomics: run-to-run bit-identical.  A bad argument raises ValueError on the host before any device work.
    NumPy in -> NumPy out; any tensor in -> tensors on that device and stream."""
    order, kind = _order(order)
    a = _check(cable_pos, c0, fs, pos=pos, block=trace, name="trace", next_block=next_block, start=start, table=(delays, kind),
               limits=project_limits()[:2])
    L, inplace = _project_check(a, beam, amp), _check_inplace(inplace, trace, next_block)
    _upload(a, like=(beam, amp))
    with torch.cuda.device(a.device):
        return _subtract(a, _given_table(beam, a.device).reshape(a.ncalls, L), _given_table(amp, a.device).reshape(a.ncalls, a.nch), order,
                         inplace, trace, next_block)


def remove_calls(trace, fs, cable_pos, c0, pos, start, length, order=1, min_coef=0.0, weights=None, next_block=None, inplace=False,
                 return_parts=False):
    """Beam, fit and subtract located calls in one call, with one delay table for the three steps:
        beam = beamform(trace, ..., start, length, order, weights, normalize=True)
        amp, coef = project_calls(trace, ..., beam, start, order, weights)
        amp[coef < min_coef] = NaN                     (min_coef=None masks nothing)
        residual = subtract_calls(trace, ..., beam, start, amp, order, inplace=inplace)
    Returns the residual (or (residual, residual_next) with next_block), followed by (beam, amp, coef) when return_parts.
    The default min_coef = 0 leaves alone the channels where the call's image correlates negatively with the record.
    Every call is fitted against trace as given and the calls are subtracted in increasing order; two calls that overlap in
    time on a channel are not fitted jointly, so the louder one belongs first and a second remove_calls over the residual
    refines the weaker.  The beam holds 1 / channels of every channel's own noise (see project_calls), which this
    subtracts along with the call.  Arguments as for beamform and subtract_calls; length is the beam's, in samples."""
    order, kind = _order(order)
    min_coef = None if min_coef is None else _number(min_coef, "min_coef")
    a = _check(cable_pos, c0, fs, pos=pos, block=trace, name="trace", next_block=next_block, weights=weights, start=start,
               table=(None, kind), limits=tuple(map(min, beam_limits()[:2], project_limits()[:2])))      # the beam's and the fit's
    L, inplace = _whole(length, "length", 1, a.max_length), _check_inplace(inplace, trace, next_block)
    _upload(a)
    with torch.cuda.device(a.device):
        beam = _beam(a, L, order, True)
        amp, coef = _project(a, beam, order)
        if min_coef is not None:
            amp = torch.where(coef < min_coef, torch.full((), float("nan"), dtype=torch.float32, device=a.device), amp)
        res = _subtract(a, beam, amp, order, inplace, trace, next_block)
    if not return_parts:
        return res
    parts = tuple(_out(t, a.as_tensor) for t in (beam, amp, coef))
    return (res,) + parts if next_block is None else res + parts


# ------------------------------------------------------------------------------------------
# beyond the reference: coherence of located calls along their moveout -- semblance, phase-weighted stack (csrc/coherence.hip)
# ------------------------------------------------------------------------------------------
Coherence = namedtuple("Coherence", ["beam", "semblance", "phase", "wsum", "times", "peak", "peak_index"])


def coherence_limits():
    """(largest number of calls, largest length, largest half_window, channels per summation segment) of the coherence kernels."""
    a, b, h, s = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.d4w_coherence_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(h), ctypes.byref(s)))
    return a.value, b.value, h.value, s.value


def _coherence_check(a, trace, next_block, weights, length, half_window, imag, next_imag, peak_range, max_half):
    """The arguments only beam_coherence has, on the host before any device work: (nt, H, (lo, hi))."""
    nt = _whole(a.ns if length is None else length, "length", 1, a.max_length)
    H = _whole(half_window, "half_window", 0, max_half)
    if weights is not None and not (dev.is_tensor(weights) and weights.is_cuda):
        w = np.asarray(weights.numpy() if dev.is_tensor(weights) else weights, dtype=np.float64)
        if not (np.all(np.isfinite(w)) and np.all(w >= 0)):
            raise ValueError("weights must be finite and >= 0")
    if imag is None or imag is False:
        if next_imag is not None:
            raise ValueError("next_imag without imag")
    elif imag is True:
        if next_imag is not None:
            raise ValueError("imag=True forms the imaginary part of next_block here: next_imag must be None")
    else:
        for what, b, like, other in (("imag", imag, trace, "trace"), ("next_imag", next_imag, next_block, "next_block")):
            if (b is None) != (like is None):
                raise ValueError("next_imag is given if and only if next_block is")
            if b is not None and (getattr(b, "ndim", 0) != 2 or _shape(b) != _shape(like)):
                raise ValueError("%s must have the shape %s of %s, got %s" % (what, _shape(like), other, _shape(b)))
    lo, hi = (0, nt) if peak_range is None else (peak_range if _shape(peak_range) == (2,) else (None, None))
    if lo is None:
        raise ValueError("peak_range must be None or (lo, hi), got %r" % (peak_range,))
    lo = _whole(lo, "peak_range[0]", 0, nt - 1)
    return nt, H, (lo, _whole(hi, "peak_range[1]", lo + 1, nt))


def _coherence(a, nt, order, H, im, pitch_im, imn, pitch_imn, rng):
    """The kernels on device tensors: (beam, semblance, phase or None, wsum) float32 [ncalls x nt], peak float32 and peak_index
    int32 [ncalls]; no launch without a call."""
    d = a.device
    beam, semb, wsum = (torch.empty((a.ncalls, nt), dtype=torch.float32, device=d) for _ in range(3))
    phase = torch.empty((a.ncalls, nt), dtype=torch.float32, device=d) if im is not None else None
    peak = torch.empty((a.ncalls,), dtype=torch.float32, device=d)
    index = torch.empty((a.ncalls,), dtype=torch.int32, device=d)
    if a.ncalls:
        nbytes = ctypes.c_size_t()
        _lib.check(_lib.lib.d4w_coherence_ws_bytes(a.nch, a.ncalls, nt, int(im is not None), ctypes.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=d)
        _lib.check(_lib.lib.d4w_coherence_f32(*_record(a), _p(im), pitch_im, _p(imn), pitch_imn, dev.ptr(a.kr), _p(a.f), _p(a.w), dev.ptr(a.s),
                                              a.ncalls, nt, order, H, dev.out_ptr(beam), dev.out_ptr(semb), _p(phase, True), dev.out_ptr(wsum),
                                              dev.out_ptr(ws), dev.stream_ptr(a.e)))
        _lib.check(_lib.lib.d4w_coherence_peak_f32(dev.ptr(semb), a.ncalls, nt, rng[0], rng[1], dev.out_ptr(peak), dev.out_ptr(index),
                                                   dev.stream_ptr(a.e)))
    return beam, semb, phase, wsum, peak, index


def beam_coherence(trace, fs, cable_pos, c0, pos, start=0, length=None, half_window=0, order=1, weights=None, next_block=None, imag=None,
                   next_imag=None, peak_range=None, *, delays=None):
    """Whether anything coherent arrived from the positions a solver returned: the windowed semblance of the beam along each
    call's moveout (Neidell-Taner) and, with the imaginary part of the analytic signal, the phase coherence across the channels.
    Both are amplitude-free numbers in [0, 1]: one threshold holds for every cable, file and sea state.  With w = weights[ch],
    v(ch, j) the sample beamform reads for (c, ch, j) at this order and h(ch, j) the same interpolation of imag, over the
    channels that contribute (weight not 0, every tap inside the record), in increasing order:
        b[c, j] = sum w v          e[c, j] = sum w v^2          W[c, j] = sum w
        pr = sum w v / a           pi = sum w h / a             a = sqrt(v^2 + h^2); a term with a = 0 adds nothing to pr, pi
        semblance[c, j] = sum_tau b^2 / sum_tau (W e),  tau over [j - half_window, j + half_window] clipped to [0, length); 0 where
                          the denominator is 0
        phase[c, j]     = sqrt(pr^2 + pi^2) / W; 0 where W is 0
    Returns the named tuple Coherence(beam, semblance, phase, wsum, times, peak, peak_index): beam = b, bit for bit
    beamform(normalize=False) of the same arguments; semblance, phase (None without imag) and wsum = W, all float32
    [ncalls x length]; times float64 as beamform's; peak float32 [ncalls] = the largest semblance of each call over the columns
    peak_range = (lo, hi), default the whole length, and peak_index int32 [ncalls] the first column that attains it.  The gate
    after locate_stack, associate_picks or relocate is  keep = result.peak >= thr.

    trace, pos, start, length, order, weights, next_block, delays: as for beamform; weights must be finite and >= 0.
    half_window: H >= 0 samples, at most coherence_limits()[2]; the window should hold a period or more of the call.
    imag: None (no phase), an array of trace's shape holding imag(hilbert(trace)) -- with next_block given, next_imag holds the
    next block's in the same way --, or True: formed here with dsp.hilbert_imag, block by block.  A per-file Hilbert transform
    is inexact for a few samples at the seam between trace and next_block; a caller who needs it exact passes blocks cut from
    a transform of the joined record.  CUDA float32 views with unit column stride are read in place with their row pitch.
    float32 sums in increasing channel order in fixed segments of coherence_limits()[3] channels, window sums in increasing tau:
    run-to-run bit-identical, independent of the other calls of the batch, and semblance keeps its bits under a power-of-two
    scaling of trace.  Non-finite samples under a non-zero weight leave the elements they touch unspecified.  A bad argument
    raises ValueError on the host before any device work (negative or non-finite weights in a CUDA tensor: before any launch).
    NumPy in -> NumPy out; a CUDA tensor in -> tensors on that device and stream."""
    a, ys = _coherence_run(trace, fs, cable_pos, c0, pos, start, length, half_window, order, weights, next_block, imag, next_imag, peak_range,
                           delays)
    return Coherence(*(None if y is None else _out(y, a.as_tensor) for y in ys))


def _coherence_run(trace, fs, cable_pos, c0, pos, start, length, half_window, order, weights, next_block, imag, next_imag, peak_range, delays):
    """beam_coherence on device tensors: (the checked arguments, (beam, semblance, phase or None, wsum, times, peak, peak_index))."""
    order, kind = _order(order)
    limits = coherence_limits()
    a = _check(cable_pos, c0, fs, pos=pos, block=trace, name="trace", next_block=next_block, weights=weights, start=start,
               table=(delays, kind), limits=limits[:2])
    nt, H, rng = _coherence_check(a, trace, next_block, weights, length, half_window, imag, next_imag, peak_range, limits[2])
    given = imag is not None and imag is not True and imag is not False
    d = _upload(a, like=(imag, next_imag) if given else ()).device
    with torch.cuda.device(d):
        im, pitch_im, imn, pitch_imn = None, 0, None, 0
        if given:
            im, pitch_im = _env_block(imag, d)
            if next_imag is not None:
                imn, pitch_imn = _env_block(next_imag, d)
        elif imag is True:
            from . import dsp
            im, pitch_im = _env_block(dsp.hilbert_imag(a.e), d)
            if a.nb is not None:
                imn, pitch_imn = _env_block(dsp.hilbert_imag(a.nb), d)
        beam, semb, phase, wsum, peak, index = _coherence(a, nt, order, H, im, pitch_im, imn, pitch_imn, rng)
        times = (a.s.to(torch.float64)[:, None] + torch.arange(nt, dtype=torch.float64, device=d)[None, :]) \
            / torch.full((), a.fs, dtype=torch.float64, device=d)
    return a, (beam, semb, phase, wsum, times, peak, index)


def beamform_pws(trace, fs, cable_pos, c0, pos, start=0, length=None, power=2.0, order=1, weights=None, next_block=None, imag=True,
                 next_imag=None, *, delays=None):
    """Phase-weighted stack toward located calls: the normalized beam times the phase coherence of beam_coherence to the power
    `power`,  (beam / wsum) * phase ** power  (0 where wsum is 0).  Stretches of the beam on which the channels do not agree in
    phase are suppressed and coherent signals keep their waveform: signal-to-noise beyond the sqrt(channels) of a linear sum.
    Returns (pws [ncalls x length] float32, times [ncalls x length] float64).  power >= 0; with power = 0 it is
    beamform(normalize=True).  imag: True (formed here with dsp.hilbert_imag, block by block) or the imaginary block(s), as
    for beam_coherence, whose other arguments, rules and containers apply."""
    power = _number(power, "power")
    if power < 0:
        raise ValueError("power must be >= 0, got %r" % (power,))
    if imag is None or imag is False:
        raise ValueError("beamform_pws needs the analytic signal: imag must be True or the imaginary block")
    a, (beam, _, phase, wsum, times, _, _) = _coherence_run(trace, fs, cable_pos, c0, pos, start, length, 0, order, weights, next_block, imag,
                                                            next_imag, None, delays)
    with torch.cuda.device(a.device):
        live = wsum != 0
        out = torch.where(live, beam / torch.where(live, wsum, torch.ones_like(wsum)), torch.zeros_like(beam)) \
            * phase ** torch.full((), power, dtype=torch.float32, device=a.device)
    return _out(out, a.as_tensor), _out(times, a.as_tensor)
