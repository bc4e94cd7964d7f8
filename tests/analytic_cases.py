"""Inputs, float64 references and bars shared by the analytic-signal mode tests (tests/test_analytic_modes_gpu.py on the
GPU, tests/test_emu_spectral.py on the CPU emulator).

The reference is always scipy.signal.hilbert in float64 on the float32 samples the kernel saw (oracle hilbert), and for the
normalised modes np.var in float64 of those same samples.  No figure in here comes from the code under test."""
import numpy as np

from oracle import d4w_oracle as orc

TOL = 1e-5
FS = 200.0
GUARD = 64


def tone_rows(nrows, ns, fs=FS, carriers=None):
    """AM-FM tones, one carrier per row: (1 + 0.3 cos(2 pi 0.7 t + r)) cos(2 pi f_r t + 2 sin(2 pi 0.5 t) + 0.4 r),
    f_r = 12 + 9 r Hz unless given.  The envelope stays within 0.7 .. 1.3 and the instantaneous frequency within 1 Hz of
    f_r, so a row written to (or read from) another row's place is 9 Hz off."""
    t = np.arange(ns)[None, :] / fs
    r = np.arange(nrows)[:, None].astype(np.float64)
    f = (12.0 + 9.0 * r) if carriers is None else np.asarray(carriers, dtype=np.float64)[:, None]
    return (1.0 + 0.3 * np.cos(2 * np.pi * 0.7 * t + r)) * np.cos(2 * np.pi * f * t + 2.0 * np.sin(2 * np.pi * 0.5 * t) + 0.4 * r)


def tone_block(nx, ns, seed, fs=FS):
    """[nx, ns] float32: rows 0 .. nx - 2 the tones, the last row white noise."""
    x = np.empty((nx, ns), dtype=np.float64)
    x[:nx - 1] = tone_rows(nx - 1, ns, fs)
    x[nx - 1] = np.random.default_rng(seed).standard_normal(ns)
    return np.ascontiguousarray(x, dtype=np.float32)


def spread_tones(nx, ns, fs=FS):
    """[nx, ns] float32 tone rows with the carriers 10, 20 .. 60 Hz by r % 6."""
    return np.ascontiguousarray(tone_rows(nx, ns, fs, carriers=10.0 + 10.0 * (np.arange(nx) % 6)), dtype=np.float32)


def reference(x32):
    """(z, var): the float64 analytic signal and population variance of the float32 samples."""
    x = np.asarray(x32, dtype=np.float64)
    return orc.hilbert(x), np.var(x, axis=1)


def check_mode(mode, y, z, var):
    """Modes 0, 1, 2, 4 against the float64 reference at the project's bar; returns the measured figure (relative to the
    bar's own scale) so that callers can print it."""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == z.shape, (y.shape, z.shape)
    assert np.all(np.isfinite(y) | (mode == 2)), "mode %d: non-finite output" % mode
    if mode == 2:                                            # on linear power ratios: the quantity under the log
        lin, ref = 10.0 ** (y / 10), np.abs(z) ** 2 / var[:, None]
        err = float(np.max(np.abs(lin - ref)) / np.max(ref))
    else:
        ref = np.abs(z) if mode == 0 else z.imag if mode == 1 else np.abs(z) / np.sqrt(var)[:, None]
        err = float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))
    assert err <= TOL, "mode %d: max|y - ref| / max|ref| = %.3e > %.0e" % (mode, err, TOL)
    return err


def ifreq_weights(z):
    """w[r, i] = min(|z_i|, |z_i+1|) / max|z_r|: the angle of z[i+1] conj(z[i]) is conditioned like 1 / |z|."""
    a = np.abs(z)
    return np.minimum(a[:, 1:], a[:, :-1]) / np.max(a, axis=1, keepdims=True)


def check_ifreq(y, z, fs, tones, need_share=0.9):
    """Mode 3, [nx, ns - 1], against diff(unwrap(angle z)) fs / 2 pi modulo fs.  Every sample of every row: d w < TOL fs / 2.
    Rows listed in `tones`: at least `need_share` of the row has w >= 0.2 (asserted from the reference alone; None: not
    asserted), there d < 5 TOL fs / 2 unweighted, and the row medians agree to 0.1 Hz.  Returns (max d w, max d on
    w >= 0.2, max median difference, smallest share)."""
    y = np.asarray(y, dtype=np.float64)
    nx, ns = z.shape
    assert y.shape == (nx, ns - 1), (y.shape, (nx, ns - 1))
    assert np.all(np.isfinite(y))
    ref = np.diff(np.unwrap(np.angle(z), axis=1), axis=1) / (2.0 * np.pi) * fs
    d = np.abs(y - ref)
    d = np.minimum(d, np.abs(d - fs))                       # a +-pi phase step may take either sign
    w = ifreq_weights(z)
    dw = float(np.max(d * w))
    assert dw < TOL * fs / 2, "mode 3: max d w = %.3e Hz (row %d) >= %.1e" % (dw, int(np.argmax(np.max(d * w, axis=1))), TOL * fs / 2)
    dmax, dmed, share = 0.0, 0.0, 1.0
    for r in tones:
        good = w[r] >= 0.2
        share = min(share, float(np.mean(good)))
        if need_share is not None:
            assert np.mean(good) >= need_share, "row %d: only %.1f %% of the reference has w >= 0.2" % (r, 100 * np.mean(good))
        dmax = max(dmax, float(np.max(d[r][good])))
        assert np.max(d[r][good]) < 5 * TOL * fs / 2, "row %d: max d = %.3e Hz on w >= 0.2" % (r, np.max(d[r][good]))
        dmed = max(dmed, abs(float(np.median(y[r]) - np.median(ref[r]))))
        assert abs(np.median(y[r]) - np.median(ref[r])) < 0.1, "row %d: medians %.3f / %.3f Hz" % (r, np.median(y[r]), np.median(ref[r]))
    return dw, dmax, dmed, share


def run_long_modes(torch, lib, dev, x_noise, x_tones, fs=FS):
    """The five modes through d4w_analytic_long_f32 the way dsp._analytic calls it (workspace from
    d4w_analytic_long_ws_bytes, the tensor's stream; var of modes 2 and 4 from d4w_row_var_f32): noise rows for modes
    0, 1, 2, 4, tone rows for mode 3.  Every output lies in front of GUARD + nx floats that must come back untouched (mode 3
    writes rows of ns - 1).  Returns five float32 host arrays."""
    from das4whales_amd._lib import check
    out = []
    xn = torch.from_numpy(x_noise).cuda()
    xt = torch.from_numpy(x_tones).cuda()
    nx, ns = xn.shape
    with torch.cuda.device(xn.device):
        var = torch.empty(nx, dtype=torch.float32, device=xn.device)
        check(lib.d4w_row_var_f32(dev.ptr(xn), nx, ns, dev.ptr(var), dev.stream_ptr(xn)))
        ws = torch.empty(int(lib.d4w_analytic_long_ws_bytes(nx, ns)), dtype=torch.uint8, device=xn.device)
        for mode in range(5):
            x = xt if mode == 3 else xn
            nout = ns - 1 if mode == 3 else ns
            buf = torch.full((nx * nout + GUARD + nx,), float("nan"), dtype=torch.float32, device=xn.device)
            y = buf[:nx * nout].view(nx, nout)
            check(lib.d4w_analytic_long_f32(dev.ptr(x), dev.ptr(y), nx, ns, mode, dev.ptr(var) if mode in (2, 4) else None,
                                            float(fs), dev.ptr(ws), dev.stream_ptr(x)))
            assert bool(torch.isnan(buf[nx * nout:]).all()), "mode %d wrote past its %d x %d output" % (mode, nx, nout)
            out.append(y.cpu().numpy())
    return out
