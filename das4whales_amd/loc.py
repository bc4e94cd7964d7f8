"""Localisation of a call from its per-channel arrival times -- mirror of the reference's `das4whales.loc`.

The nine reference functions keep their names, parameter names and defaults.  The Gauss-Newton solver, the travel times and
the misfit grid run in csrc/loc.hip (float64); `solve_lq_batch`, `misfit_grid` and `first_guess_grid` are the batched forms
the reference does not have.  NumPy in -> NumPy float64 out; a CUDA tensor in -> a float64 tensor on the same device and
stream.  The four small per-channel helpers (distances, radii, angles) are host float64 arithmetic for NumPy input, like the
index arithmetic of the other namespaces; for tensors they stay on the device.

Arrival times that are NaN mean "no pick on this channel": the solver and the grid skip them (the reference has no such
notion -- its np.min(Ti) turns the whole result into NaN).
"""
import sys

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


def _back(y, *templates):
    """The device result in the callers' container: a tensor where any input was one (on the host if none was on a device)."""
    ts = [t for t in templates if dev.is_tensor(t)]
    if ts:
        return y if any(t.is_cuda for t in ts) else y.cpu()
    return y.cpu().numpy()


def _device_of(*xs):
    for x in xs:
        if dev.is_tensor(x) and x.is_cuda:
            return x.device
    return None


def _cable(cable_pos, device):
    c = _f64(cable_pos, device)
    if c.dim() != 2 or c.shape[1] != 3 or c.shape[0] < 1:
        raise ValueError("cable_pos must be [channel x 3], got %s" % (tuple(c.shape),))
    return c


def _calls(Ti, nch, device):
    """Ti as [ncalls][nch] on the device; (tensor, whether the caller passed one call as a vector)."""
    t = _f64(Ti, device)
    single = t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1 and nch != 1)
    if single:
        t = t.reshape(1, -1)
    if t.dim() != 2 or t.shape[1] != nch:
        raise ValueError("Ti must hold one arrival time per channel (%d), got %s" % (nch, tuple(t.shape)))
    return t, single


def _solve(t, cable, c0, Nbiter, fix_z, first_guess):
    """The kernel on [ncalls][nch]: history, n, G^T G, sum of squared residuals, pick count (device tensors)."""
    ncalls, nch = t.shape
    p = 3 if fix_z else 4
    Nbiter = int(Nbiter)
    if Nbiter < 0:
        raise ValueError("Nbiter must not be negative")
    d = t.device
    fg = None
    if first_guess is not None:
        fg = _f64(first_guess, d)
        if fg.dim() == 1:
            fg = fg.reshape(1, -1).expand(ncalls, -1).contiguous()
        if tuple(fg.shape) != (ncalls, 4):
            raise ValueError("first_guess must be [x, y, z, t0] per call (%d x 4), got %s" % (ncalls, tuple(fg.shape)))
    with torch.cuda.device(d):
        hist = torch.empty((ncalls, Nbiter, 4), dtype=torch.float64, device=d)
        n = torch.empty((ncalls, 4), dtype=torch.float64, device=d)
        gtg = torch.empty((ncalls, p, p), dtype=torch.float64, device=d)
        ssr = torch.empty((ncalls,), dtype=torch.float64, device=d)
        npick = torch.empty((ncalls,), dtype=torch.int32, device=d)
        _lib.check(_lib.lib.d4w_loc_solve_f64(dev.ptr(cable), nch, dev.ptr(t), ncalls, float(c0), Nbiter, int(bool(fix_z)),
                                              dev.ptr(fg) if fg is not None else None, dev.out_ptr(hist) if Nbiter else None,
                                              dev.out_ptr(n), dev.out_ptr(gtg), dev.out_ptr(ssr), dev.out_ptr(npick),
                                              dev.stream_ptr(t)))
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


# ------------------------------------------------------------------------------------------
# the reference's functions
# ------------------------------------------------------------------------------------------
def calc_arrival_times(t0, cable_pos, pos, c0):
    """Theoretical arrival times of a call emitted at `t0` from `pos` = [x, y, z] at every channel (loc.py:13-25).  Beyond the
    reference: `pos` = [npos x 3] with `t0` a scalar or [npos] gives [npos x channel] in one launch."""
    device = _device_of(cable_pos, pos, t0)
    cable = _cable(cable_pos, device)
    p = _f64(pos, cable.device)
    single = p.dim() == 1
    p = p.reshape(1, -1) if single else p
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("pos must be [x, y, z] or [npos x 3], got %s" % (tuple(p.shape),))
    npos, nch = p.shape[0], cable.shape[0]
    t = _f64(t0, cable.device).reshape(-1)
    if t.numel() == 1:
        t = t.expand(npos).contiguous()
    if t.numel() != npos:
        raise ValueError("t0 must be a scalar or one value per position")
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
    p = 3 if fix_z else 4
    cnt = npick.cpu().numpy().astype(np.int64)
    with np.errstate(all="ignore"):
        var = np.where(cnt > p, ssr.cpu().numpy() / np.maximum(cnt - p, 1), np.nan)
        cov = _covariance(np.where((cnt > 0)[:, None, None], gtg.cpu().numpy(), np.nan), var, quiet=True)
        unc = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
    stats = {"variance": var, "covariance": cov, "uncertainty": unc, "npicks": cnt}
    stats = {k: _back(torch.from_numpy(np.ascontiguousarray(v)).to(t.device), Ti, cable_pos) for k, v in stats.items()}
    stats["history"] = _back(hist, Ti, cable_pos)
    return _back(n, Ti, cable_pos), stats


def misfit_grid(Ti, cable_pos, c0, xs, ys, z):
    """For every call and every node (xs[ix], ys[iy], z): the best emission time t0 = mean over the picked channels of
    Ti - distance / c0, and the RMS residual once it is removed.  Returns (rms, t0), each [ncalls x ny x nx] ([ny x nx] for
    one call given as a vector).  The minimum of rms is the first guess solve_lq needs (first_guess_grid)."""
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
    if single:
        rms, t0 = rms[0], t0[0]
    return _back(rms, Ti, cable_pos), _back(t0, Ti, cable_pos)


def first_guess_grid(Ti, cable_pos, c0, xs, ys, z):
    """The node of smallest RMS misfit per call as [x, y, z, t0] ([ncalls x 4], or [4] for one call given as a vector), ready to
    pass as `first_guess`.  A call without a pick gives a NaN row."""
    cable = _cable(cable_pos, _device_of(Ti, cable_pos))
    t, single = _calls(Ti, cable.shape[0], cable.device)
    gx, gy = _f64(xs, cable.device).reshape(-1), _f64(ys, cable.device).reshape(-1)
    rms, t0 = misfit_grid(t, cable, c0, gx, gy, z)
    ncalls = t.shape[0]
    flat = torch.nan_to_num(rms.reshape(ncalls, -1), nan=float("inf"))
    k = torch.argmin(flat, dim=1)
    out = torch.stack([gx[k % gx.numel()], gy[k // gx.numel()], torch.full_like(gx[k % gx.numel()], float(z)),
                       t0.reshape(ncalls, -1).gather(1, k[:, None])[:, 0]], dim=1)
    out[torch.isnan(out[:, 3])] = float("nan")
    return _back(out[0] if single else out, Ti, cable_pos)
