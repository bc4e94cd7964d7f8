"""detect -- MI355X-native mirror of das4whales.detect (reference: src/das4whales/detect.py).

Templates are generated on the host in float64 (a few hundred samples); correlations run in the
HIP library (include/d4w.h: d4w_row_stats_f32 / d4w_row_stats_prefix_f32 for the normalisation; d4w_xcorr_mm_tail_f32,
d4w_xcorr_fft_cont_f32 or d4w_xcorr_lens_f32 for the correlation; d4w_xcorr_dc_tail_rows_f32 where the zero-padded templates'
tail takes a second pass -- _matched_filter chooses)."""
import numpy as np
import torch

import collections.abc

from . import _device as dev
from . import dsp
from ._lib import lib, check
from .dsp import _cache_lock


# ---------------------------------------------------------------------------------------------
# templates (host)
# ---------------------------------------------------------------------------------------------
def gen_linear_chirp(fmin, fmax, duration, sampling_rate):
    """Linear down-sweep fmax -> fmin -- reference detect.py:20-41
    (scipy.signal.chirp(t, f0=fmax, f1=fmin, t1=duration, 'linear') restated)."""
    t = np.arange(0, duration, 1 / sampling_rate)
    return np.cos(2 * np.pi * (fmax * t + 0.5 * (fmin - fmax) / duration * t * t))


def gen_hyperbolic_chirp(fmin, fmax, duration, sampling_rate):
    """Hyperbolic down-sweep fmax -> fmin -- reference detect.py:44-65."""
    t = np.arange(0, duration, 1 / sampling_rate)
    f0, f1 = fmax, fmin
    if f0 == f1:
        return np.cos(2 * np.pi * f0 * t)
    sing = -f1 * duration / (f0 - f1)
    return np.cos(2 * np.pi * (-sing * f0) * np.log(np.abs(1 - t / sing)))


def gen_template_fincall(time, fs, fmin=15., fmax=25., duration=1., window=True):
    """Hann-windowed hyperbolic chirp zero-padded to len(time) -- reference detect.py:68-93."""
    chirp_signal = gen_hyperbolic_chirp(fmin, fmax, duration, fs)
    template = np.zeros(np.shape(time))
    if window:
        template[:len(chirp_signal)] = chirp_signal * np.hanning(len(chirp_signal))
    else:
        template[:len(chirp_signal)] = chirp_signal
    return template


# ---------------------------------------------------------------------------------------------
# matched filter
# ---------------------------------------------------------------------------------------------
def _support(v):
    nz = np.nonzero(v)[0]
    return int(nz[-1]) + 1 if len(nz) else 1


def _taps_tensor(taps_list, device):
    lt = max(4, -(-max(len(t) for t in taps_list) // 4) * 4)
    taps = np.zeros((len(taps_list), lt), dtype=np.float32)
    for i, t in enumerate(taps_list):
        taps[i, :len(t)] = t
    return torch.from_numpy(taps).to(device), lt


_xf_tables = {}     # (templates, device, stream) -> [taps tensor, lt, workspace, tables built]


def _xf_prepared(grp, device, ws=True):
    """Device taps + the overlap-save workspace of a template group, kept per (templates, device, stream): the second
    call with the same templates on the same stream finds the template spectra already in the workspace (taps = NULL
    in d4w_xcorr_fft_cont_f32) and uploads nothing.  ws=False (the matrix-core form): the taps only."""
    key = (tuple(np.asarray(t, dtype=np.float64).tobytes() for t in grp), str(device),
           int(torch.cuda.current_stream(device).cuda_stream))
    with _cache_lock:
        ent = _xf_tables.get(key)
        if ent is None:
            if len(_xf_tables) > 32:
                _xf_tables.clear()
            taps, lt = _taps_tensor(grp, device)
            ent = _xf_tables[key] = [taps, lt, None, False]
        if ws and ent[2] is None:
            ent[2] = torch.empty(int(lib.d4w_xcorr_fft_ws_bytes()), dtype=torch.uint8, device=device)
    return ent


# das4whales_amd.set_strict_reference(True): the reference's side effects and degenerate values where this package's defaults
# differ: tapering=True tapers the caller's array (dsp.py:744-745), an all-zero row correlates to NaN (detect.py:157)
STRICT_REFERENCE = False

_row_stats_memo = {}        # (data_ptr, shape, device) -> (weakref to the tensor, its version, (mean, maxabs))


def _row_stats_cached(x, prefix=False):
    """(mean, max|.|) of the rows of a CUDA tensor, remembered while the SAME tensor (identity and version counter) is asked
    again: the reference's scripts call compute_cross_correlogram once per template on one block
    (scripts/main_mfdetect.py:79-80), which would read it twice just for the normalisation.  prefix=True: (mean, max|.|,
    prefix maxima) from one launch (d4w_row_stats_prefix_f32; what _matched_filter decides the tail per row on)."""
    import weakref
    nx, ns = x.shape
    # per stream: statistics formed on one stream are not ordered before a kernel of another
    key = (x.data_ptr(), nx, ns, str(x.device), int(torch.cuda.current_stream(x.device).cuda_stream), bool(prefix))
    with _cache_lock:
        ent = _row_stats_memo.get(key)
        if ent is not None and ent[0]() is x and ent[1] == x._version:
            return ent[2]
    with torch.cuda.device(x.device):
        mean = torch.empty(nx, dtype=torch.float64, device=x.device)      # float64 (hi + lo for the kernels): d4w.h
        mx = torch.empty(nx, dtype=torch.float32, device=x.device)
        if prefix:
            pm = torch.empty(nx, dtype=torch.float32, device=x.device)
            check(lib.d4w_row_stats_prefix_f32(dev.ptr(x), nx, ns, dev.ptr(mean), dev.ptr(mx), dev.ptr(pm), dev.stream_ptr(x)))
            res = (mean, mx, pm)
        else:
            check(lib.d4w_row_stats_f32(dev.ptr(x), nx, ns, dev.ptr(mean), dev.ptr(mx), dev.stream_ptr(x)))
            res = (mean, mx)
    with _cache_lock:
        if len(_row_stats_memo) > 8:
            _row_stats_memo.clear()
        _row_stats_memo[key] = (weakref.ref(x), x._version, res)
    return res


def _remember_row_stats(x, stats):
    """Deposits (float64 row means, float32 row maxima) somebody else formed for the CUDA tensor x as it is now -- the f-k
    filter's last pass leaves them in its epilogue (dsp._fk_apply) -- so that the matched filter that follows does not read
    the block again for its normalisation (detect.py:157).  Dropped like any memo entry when x is written to."""
    import weakref
    nx, ns = x.shape
    key = (x.data_ptr(), nx, ns, str(x.device), int(torch.cuda.current_stream(x.device).cuda_stream), False)
    with _cache_lock:
        if len(_row_stats_memo) > 8:
            _row_stats_memo.clear()
        _row_stats_memo[key] = (weakref.ref(x), x._version, tuple(stats[:2]))


def _xcorr_method(taps_list, ns, method):
    """The kernel a correlation runs on: "mm" (banded-Toeplitz product on the matrix cores: two templates of <= 177 samples in
    one launch, one template of <= 497 per launch, longer ones in 496-tap sections up to d4w_xcorr_mm_max_support(); the
    default), "fft" (overlap-save, supports <= 161, rows >= 1024 samples) or "direct" (any support).  D4W_XCORR_METHOD
    overrides "auto" (measurements, A/B tests)."""
    import os
    import warnings
    explicit = method != "auto"
    if method == "auto":
        method = os.environ.get("D4W_XCORR_METHOD", "auto")
    if method not in ("auto", "mm", "fft", "direct"):
        raise ValueError("method must be 'auto', 'mm', 'fft' or 'direct', not %r" % (method,))
    longest = max(len(t) for t in taps_list)
    mm_ok = longest <= int(lib.d4w_xcorr_mm_max_support())
    fft_ok = ns >= 1024 and longest <= int(lib.d4w_xcorr_fft_max_support())
    if method == "mm" and not mm_ok:
        if explicit:
            raise ValueError("the matrix-core correlation takes supports <= %d samples" % int(lib.d4w_xcorr_mm_max_support()))
        warnings.warn("D4W_XCORR_METHOD=mm does not apply to a support of %d samples: choosing the form as 'auto' does" % longest)
        method = "auto"
    if method == "fft" and not fft_ok:
        # an override the shape does not admit falls back like 'auto' instead of surfacing as EINVAL from the C side
        warnings.warn("the overlap-save FFT correlation needs rows >= 1024 samples and supports <= %d (got %d, %d): "
                      "choosing the form as 'auto' does" % (int(lib.d4w_xcorr_fft_max_support()), ns, longest))
        method = "auto"
    if method == "mm" or (method == "auto" and mm_ok):
        return "mm"
    if method == "fft" or (method == "auto" and fft_ok):
        return "fft"
    return "direct"


def _tails_in_kernel(taps_list, coefs, ns, how):
    """Whether the zero-padded templates' constant tails (detect.py:158) can be added inside the matrix-core correlator
    (d4w_xcorr_mm_tail_f32: exact on every row, no second pass): the matrix-core form, supports of at most
    d4w_xcorr_mm_tail_max_support() samples (one launch per template) and shorter than the rows.
    D4W_XCORR_TAIL=pass keeps the two-pass form of rounds 1-5 (A/B measurements)."""
    import os
    if how != "mm" or not any(c != 0.0 for c in coefs) or os.environ.get("D4W_XCORR_TAIL", "kernel") == "pass":
        return False
    longest = max(len(t) for t in taps_list)
    return longest <= int(lib.d4w_xcorr_mm_tail_max_support()) and longest < ns


def _xcorr_device(x, taps_list, normalize, method="auto", stats=None, cont=None, row_max=None, tails=None):
    """x: float32 CUDA [nx, ns]; taps_list: 1..n host float64 vectors -> list of CUDA tensors.
    tails: optional list of the templates' DC-tail coefficients (_tail_coef) to be added inside the matrix-core kernel
    (the caller has checked _tails_in_kernel; needs normalize=True).
    method: "mm" (matrix cores), "fft" (overlap-save), "direct", or "auto" (_xcorr_method).
    stats: optional (mean, maxabs) CUDA tensors of the rows, e.g. from FkPlan.apply_stats.
    cont: optional (tensor [nx, >= n], n): the record continues -- the last lags read the first n samples of these rows
    instead of zeros (stream.FileStream); the matrix-core form, or exactly two templates on the FFT form.
    row_max: optional list that receives one CUDA tensor [nx] per template, max over the lags of every row, from the
    matrix-core kernel's epilogue (d4w_xcorr_mm_rowmax_f32); other forms leave it empty."""
    nx, ns = x.shape
    outs = []
    how = _xcorr_method(taps_list, ns, method)
    if tails is not None:
        if how != "mm" or not normalize or len(tails) != len(taps_list):
            raise ValueError("in-kernel template tails need the matrix-core form, normalize=True and one coefficient per template")
    if cont is not None:
        nxt, n_next = cont
        if not (how in ("mm", "fft") and (how == "mm" or len(taps_list) == 2) and nxt.is_cuda and nxt.dtype == torch.float32
                and nxt.stride(1) == 1 and nxt.shape[0] == nx and nxt.shape[1] >= n_next):
            raise ValueError("a continuation needs the matrix-core form (or two templates on the FFT form) and float32 CUDA rows")
    with torch.cuda.device(x.device):
        mean = mx = None
        if normalize and stats is not None:
            mean, mx = stats
            if (mean.dtype != torch.float64 or mx.dtype != torch.float32 or mean.numel() < nx or mx.numel() < nx
                    or not mean.is_contiguous() or not mx.is_contiguous()):
                raise ValueError("stats = (float64 row means, float32 row maxima), one contiguous value per row (d4w_row_stats_f32)")
        elif normalize:
            mean, mx = _row_stats_cached(x)
        for i in range(0, len(taps_list), 2):                      # two templates per read of x
            grp = taps_list[i:i + 2]
            # the correlograms of a fused pair sit back to back in one allocation: a consumer that treats both alike (envelope
            # picks at one threshold) can take them as ONE [2 nx, ns] block (stacked_pair below) -- one launch per operator
            pair = torch.empty((len(grp),) + tuple(x.shape), dtype=x.dtype, device=x.device)
            ys = [pair[k] for k in range(len(grp))]
            if how == "mm":
                taps, lt, _, _ = _xf_prepared(grp, x.device, ws=False)
                rm = [torch.empty(nx, dtype=torch.float32, device=x.device) for _ in grp] if row_max is not None else None
                tc = [float(c) for c in tails[i:i + 2]] if tails is not None else [0.0]
                check(lib.d4w_xcorr_mm_tail_f32(dev.ptr(x), nx, ns,
                                                dev.ptr(cont[0]) if cont is not None else None,
                                                int(cont[0].stride(0)) if cont is not None else 0,
                                                int(cont[1]) if cont is not None else 0,
                                                dev.ptr(mean) if normalize else None, dev.ptr(mx) if normalize else None,
                                                dev.ptr(taps), len(grp), lt, len(grp[0]), len(grp[-1]), tc[0], tc[-1] if len(grp) > 1 else 0.0,
                                                dev.ptr(ys[0]), dev.ptr(ys[1]) if len(ys) > 1 else None,
                                                dev.ptr(rm[0]) if rm else None, dev.ptr(rm[1]) if rm and len(rm) > 1 else None,
                                                dev.stream_ptr(x)))
                outs.extend(ys)
                if rm:
                    row_max.extend(rm)
                continue
            if how == "fft":
                ent = _xf_prepared(grp, x.device)
                taps, lt, ws, built = ent
                check(lib.d4w_xcorr_fft_cont_f32(dev.ptr(x), nx, ns,
                                                 dev.ptr(cont[0]) if cont is not None else None,
                                                 int(cont[0].stride(0)) if cont is not None else 0,
                                                 int(cont[1]) if cont is not None else 0,
                                                 dev.ptr(mean) if normalize else None,
                                                 dev.ptr(mx) if normalize else None, None if built else dev.ptr(taps), len(grp), lt,
                                                 len(grp[0]), len(grp[-1]),
                                                 dev.ptr(ys[0]), dev.ptr(ys[1]) if len(ys) > 1 else None,
                                                 dev.ptr(ws), dev.stream_ptr(x)))
                ent[3] = True
                outs.extend(ys)
                continue
            taps, lt = _taps_tensor(grp, x.device)
            check(lib.d4w_xcorr_lens_f32(dev.ptr(x), nx, ns, dev.ptr(mean) if normalize else None,
                                         dev.ptr(mx) if normalize else None, dev.ptr(taps), len(grp), lt,
                                         len(grp[0]), len(grp[-1]),
                                         dev.ptr(ys[0]), dev.ptr(ys[1]) if len(ys) > 1 else None,
                                         dev.stream_ptr(x)))
            outs.extend(ys)
    return outs


def stacked_pair(c0, c1):
    """The two correlograms of one fused correlator launch as ONE [2 nx, ns] tensor (no copy) when they sit back to back in one
    allocation (what _xcorr_device produces for a template pair), else None.  Rows 0 .. nx-1 are c0's, nx .. 2 nx-1 are c1's."""
    b0, b1 = getattr(c0, "_base", None), getattr(c1, "_base", None)
    if (b0 is None or b0 is not b1 or b0.dim() != 3 or b0.shape[0] != 2 or not b0.is_contiguous() or c0.shape != c1.shape
            or c0.data_ptr() != b0.data_ptr() or c1.data_ptr() != b0.data_ptr() + c0.numel() * c0.element_size()):
        return None
    return b0.view(2 * c0.shape[0], c0.shape[1])


def correlogram_max(c, row_max=None, on_device=False):
    """np.max(corr_m) of a correlogram as a Python float (scripts/main_mfdetect.py:82: the detection threshold is half the
    largest correlation): from the per-row maxima the matrix-core correlator left in its epilogue when they are given
    (stream.FileStream results carry them: one 2-value reduction over nx numbers), else one read of the block -- the
    library's own reduction either way, one 8-byte copy to the host.  on_device=True: the value stays on the device (a
    1-element float32 CUDA tensor, no copy, no wait) for `Threshold(0.45, value)` below."""
    src = row_max if row_max is not None else dev.to_device_f32(c)
    mm = torch.empty(2, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        check(lib.d4w_minmax_f32(dev.ptr(src), int(src.numel()), dev.ptr(mm), dev.stream_ptr(src)))
    return mm[1:2] if on_device else float(mm.cpu()[1])


class Threshold:
    """A pick threshold formed on the device: scale x value[0] (value: a 1-element float32 CUDA tensor, e.g.
    correlogram_max(c, on_device=True)) -- the reference's `0.45 * np.max(corr_m)` (scripts/main_mfdetect.py:82,95) without the
    host waiting for the maximum; the product is formed in float64 like the host's.  A NaN value (the maximum of a block
    with a dead channel, detect._nan_dead_rows) or a NaN scale gives a NaN bar, and a NaN bar yields no pick in any row, as
    scipy.signal.find_peaks(x, prominence=nan) does -- the same holds of a NaN passed as a plain number.  A +inf bar yields no
    pick either, even in a row that holds +inf (SciPy keeps such a sample: DESIGN.md).  Accepted wherever pick_times /
    pick_times_env take a threshold."""

    def __init__(self, scale, value):
        if not (dev.is_tensor(value) and value.is_cuda and value.dtype == torch.float32 and value.numel() == 1):
            raise ValueError("value must be a 1-element float32 CUDA tensor")
        self.scale, self.value = float(scale), value

    def __float__(self):
        return self.scale * float(self.value.cpu().reshape(-1)[0])


class ChannelThreshold:
    """One pick threshold per channel, formed on the device: scale x values[c] (values: a float32 CUDA [nx] tensor) -- "k times
    this channel's noise floor", e.g. ChannelThreshold(8.0, dsp.channel_noise(x).env_quantiles[:, 0]) with the per-channel
    median envelope of scripts/main_bathynoise.py:139,183.  No host wait; the product is formed in float64 like Threshold's.
    As in SciPy a NaN or +inf bar yields no pick in its row, a zero or negative bar every strict local maximum.  Accepted
    wherever pick_times / pick_times_env take a threshold."""

    def __init__(self, scale, values):
        if not (dev.is_tensor(values) and values.is_cuda and values.dtype == torch.float32 and values.dim() == 1 and values.numel() >= 1):
            raise ValueError("values must be a float32 CUDA tensor with one value per channel")
        self.scale, self.values = float(scale), values.contiguous()


def _per_channel(threshold, nx):
    """Host-side reading of a picker's threshold: None for the one-bar forms (a number, a Threshold), else the per-channel bars
    as a ChannelThreshold or a float32 ndarray of nx values.  A wrong count raises ValueError -- before any device work."""
    if isinstance(threshold, Threshold):
        return None
    if isinstance(threshold, ChannelThreshold):
        n, bars = int(threshold.values.numel()), threshold
    elif dev.is_tensor(threshold):
        if threshold.dim() == 0 or (threshold.numel() == 1 and nx != 1):
            return None                                              # float(threshold), as ever
        if not (threshold.is_cuda and threshold.dtype == torch.float32):
            raise ValueError("a per-channel threshold tensor must be a float32 CUDA tensor (or pass a NumPy array / list)")
        n, bars = (int(threshold.numel()) if threshold.dim() == 1 else -1), ChannelThreshold(1.0, threshold.reshape(-1))
    else:
        if np.ndim(threshold) == 0 or (np.size(threshold) == 1 and nx != 1):
            return None
        bars = np.asarray(threshold, dtype=np.float32)
        n = int(bars.size) if bars.ndim == 1 else -1
    if n != nx:
        raise ValueError("a per-channel threshold needs one value for each of the %d channels (got %s)"
                         % (nx, "%d" % n if n >= 0 else "an array that is not 1-D"))
    return bars


def xcorr_continuation_ok(taps_list, ns, how=None):
    """Whether _xcorr_device(..., cont=...) applies: the matrix-core form, or two templates that run the fused overlap-save kernel.
    how: _xcorr_method(taps_list, ns, "auto") when the caller has resolved it already."""
    import os
    if how is None:
        how = _xcorr_method(taps_list, ns, "auto")
    if how == "mm":
        return True
    return (how == "fft" and len(taps_list) == 2
            and os.environ.get("D4W_XF_FUSED", "1") == "1" and os.environ.get("D4W_XF_TPAIR", "0") == "0")


def _host_vec(v):
    if dev.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype=np.float64).ravel()


def shift_xcorr(x, y):
    """Positive-lag cross-correlation c[k] = sum_n x[n+k] y[n] -- reference detect.py:96-112."""
    yv = _host_vec(y)
    x1 = x if dev.is_tensor(x) else np.asarray(x)
    if x1.ndim != 1:
        raise ValueError("shift_xcorr expects 1-D inputs")
    xd = dev.to_device_f32(x1.reshape(1, -1))
    c = _xcorr_device(xd, [yv[:_support(yv)]], normalize=False)[0][0]
    return dev.like_input(c, x)


def shift_nxcorr(x, y):
    """shift_xcorr / (std(x) std(y) len(x)) -- reference detect.py:115-137 (population std)."""
    xv, yv = _host_vec(x), _host_vec(y)
    c = shift_xcorr(x, y)
    return c / (np.std(xv) * np.std(yv) * len(xv))


_tpl_memo = {}      # digest of a template's bytes -> (normalised support, tail coefficient)


def _template_parts(template):
    """(normalised support, tail coefficient) of a template, remembered by the CONTENT of the vector (a 64-bit digest of its
    bytes: 0.1 ms for a 120 000-sample template against 0.8 ms for the mean / max / support sweeps -- the reference's scripts call
    compute_cross_correlogram once per template and block with the same two vectors, scripts/main_mfdetect.py:79-80)."""
    t = _host_vec(template)
    try:
        import xxhash
        key = (t.shape[0], xxhash.xxh3_64_intdigest(t.tobytes()))
    except Exception:                                    # noqa: BLE001  (no xxhash: a slower digest, same behaviour)
        import hashlib
        key = (t.shape[0], hashlib.blake2b(t.tobytes(), digest_size=8).digest())
    with _cache_lock:
        hit = _tpl_memo.get(key)
    if hit is not None:
        return hit
    a = np.max(np.abs(t))
    if a == 0:
        raise ValueError("template is all zeros")
    sup = _support(t)
    taps = ((t - t.mean()) / a)[:sup]
    taps.setflags(write=False)
    coef = 0.0 if sup >= len(t) else float(t.mean() / a)
    with _cache_lock:
        if len(_tpl_memo) > 64:
            _tpl_memo.clear()
        _tpl_memo[key] = (taps, coef)
    return taps, coef


def _normalised_support(template):
    """detect.py:158: (template - mean) / max|template| over the zero-padded length; returns the
    non-zero support of the ORIGINAL template (the constant -mean/max tail on the padded part is
    handled by _tail_coef and _matched_filter)."""
    return _template_parts(template)[0]


def _tail_coef(template):
    """mean(template) / max|template| over the zero-padded length: minus the constant that detect.py:158
    leaves on the padded part (0 when the template fills its whole length)."""
    return _template_parts(template)[1]


# The DC tail of a zero-padded template (detect.py:158) is |coef| g times a PREFIX SUM of the de-meaned row: 3-5e-6 of the
# correlogram's maximum for the fin-whale templates on white 60-s rows, 3e-8 on band-passed rows, 1e-3 on rows that drift --
# a property of the data, so the decision is taken per row on the data (round 5; rounds 1-4 predicted it from the template
# assuming white rows and let drifting rows pass with 2-9e-4): a row is left without the term only when the term cannot
# exceed TAIL_EPS of that row's own largest correlation (d4w_row_prefix_max_f32 bounds it, the correlator's epilogue gives
# the row maximum), every other row receives it.
TAIL_EPS = 1e-6


def _tail_form(taps, coefs, ns, exact_tail=None):
    """(how, form): the correlator a block of ns-sample rows runs on (_xcorr_method) and how its zero-padded templates' DC
    tails (detect.py:158) are added -- None (no non-zero coefficient, or exact_tail=False), "kernel" (inside the matrix-core
    correlator, _tails_in_kernel), "rows" (second pass, decided per row by TAIL_EPS: exact_tail=None on the matrix-core
    form, the one that leaves row maxima) or "all" (second pass, every row).  The ONE place where the form is chosen."""
    how = _xcorr_method(taps, ns, "auto")                   # decided once (an override that does not apply warns once)
    if exact_tail is False or not any(c != 0.0 for c in coefs):
        return how, None
    if _tails_in_kernel(taps, coefs, ns, how):
        # round 6: the term is formed inside the correlator (prefix sums in its sample-conversion phase) -- exact on every row,
        # one pass over the block, no per-row decision
        return how, "kernel"
    return how, "rows" if exact_tail is None and how == "mm" else "all"


def _needs_prefix_max(taps, coefs, ns):
    """Whether _matched_filter(..., exact_tail=None) will read the rows' prefix maxima at this shape: who forms the row
    statistics ahead of it (dsp._fk_apply_stats(..., prefix=)) forms them only then."""
    return _tail_form(taps, coefs, ns)[1] == "rows"


def _matched_filter(x, taps, coefs, exact_tail=None, stats=None, next_head=None, want_row_max=False):
    """Peak-normalised correlograms of the rows of x (float32 CUDA [nx, ns]) with the templates' supports `taps`, the DC tails
    of their zero-padded originals (coefs: _tail_coef; exact_tail as in compute_cross_correlograms) included
    -> (correlograms, row maxima or None).
    stats: (mean, maxabs[, prefix maxima]) of x as dsp._fk_apply_stats leaves them; what is missing comes from
    _row_stats_cached.  next_head: [nx, >= longest support - 1] rows that continue x (stream.FileStream): the last lags
    read them in place where a continuation applies (xcorr_continuation_ok), else [x | head] is correlated and cropped;
    normalisation and tails stay those of x.  want_row_max: also return max over the lags per template and row where the
    matrix-core correlator leaves it; without it that epilogue runs only for the per-row tail decision."""
    nx, ns = x.shape
    how, form = _tail_form(taps, coefs, ns, exact_tail)
    n_next = max(len(t) for t in taps) - 1 if next_head is not None else 0
    cont, src = None, x
    if n_next > 0:
        if next_head.is_cuda and next_head.dtype == torch.float32 and next_head.stride(1) == 1 and xcorr_continuation_ok(taps, ns, how):
            cont = (next_head, n_next)
        else:
            # the padding must enter de-meaned like the block's own samples (the kernel subtracts the mean from every
            # sample it reads); the epilogues do not apply to the widened rows
            src = dsp._concat_cols([x, next_head[:, :n_next]])
            if form is not None:
                form = "all"
    if stats is None or (form == "rows" and len(stats) < 3):
        stats = _row_stats_cached(x, prefix=form == "rows")
    rmax = [] if src is x and (want_row_max or form == "rows") else None
    outs = _xcorr_device(src, taps, normalize=True, method=how, stats=stats[:2], cont=cont, row_max=rmax,
                         tails=coefs if form == "kernel" else None)
    if src is not x:
        outs = [dsp._copy_cols(c[:, :ns], torch.empty_like(x)) for c in outs]
    if form in ("rows", "all"):
        # a row is left without the term only where it cannot exceed TAIL_EPS of the row's own largest correlation ("rows");
        # the kernel forms the row maxima of the rows it changes again
        by_row = form == "rows"
        with torch.cuda.device(x.device):
            for k, (o, tp, c) in enumerate(zip(outs, taps, coefs)):
                if c != 0.0:
                    check(lib.d4w_xcorr_dc_tail_rows_f32(dev.ptr(x), nx, ns, dev.ptr(stats[0]), dev.ptr(stats[1]), float(c), len(tp),
                                                         dev.out_ptr(o), dev.ptr(stats[2]) if by_row else None,
                                                         dev.out_ptr(rmax[k]) if rmax else None,
                                                         TAIL_EPS if by_row else 0.0, dev.stream_ptr(x)))
    return outs, rmax or None


def _nan_dead_rows(xd, outs):
    """zero_rows="nan": an all-zero row (a dead channel) is 0 / 0 in the reference's normalisation (detect.py:157) and its
    correlogram NaN; the kernels give zeros.  One masked fill per correlogram, only when asked for."""
    dead = _row_stats_cached(xd)[1] == 0
    for o in outs:
        o[dead] = float("nan")


def compute_cross_correlograms(data, templates, exact_tail=None, zero_rows=None):
    """Several templates against one block (detect.compute_cross_correlogram for each) -- what
    scripts/main_mfdetect.py:79-80 does with two separate calls.  exact_tail: True / False forces /
    skips the DC-tail term of the zero-padded template (detect.py:158) on every row; None (default) decides per row
    on the data and leaves out only what cannot exceed TAIL_EPS of the row's largest correlation (_matched_filter).
    zero_rows: "zeros" (default) / "nan" -- what an all-zero row gives; "nan" is the reference's 0 / 0
    (default "nan" under das4whales_amd.set_strict_reference(True))."""
    if zero_rows is None:
        zero_rows = "nan" if STRICT_REFERENCE else "zeros"
    if zero_rows not in ("zeros", "nan"):
        raise ValueError('zero_rows must be "zeros" or "nan"')
    xd, outs = _correlograms(data, templates, exact_tail)
    if zero_rows == "nan":
        _nan_dead_rows(xd, outs)
    return [dev.like_input(o, data) for o in outs]


def _correlograms(data, templates, exact_tail):
    if getattr(data, "ndim", 0) != 2:
        raise ValueError("data must be a 2-D [channel x time] array")
    xd = dev.to_device_f32(data)
    # no row maxima asked for: the in-kernel tail runs the kernel instance without that epilogue
    outs, _ = _matched_filter(xd, [_normalised_support(t) for t in templates], [_tail_coef(t) for t in templates], exact_tail=exact_tail)
    return xd, outs


def compute_cross_correlogram(data, template, exact_tail=None, zero_rows=None):
    """Peak-normalised matched filter, every row against `template` -- reference detect.py:140-166.

    Rows: (x - mean) / max|x| (max of the un-de-meaned row, detect.py:157).  Output is floating
    point (the reference's np.empty_like would truncate integer input); an all-zero row gives
    zeros where the reference divides by zero -- zero_rows="nan" gives the reference's NaN row."""
    return compute_cross_correlograms(data, [template], exact_tail=exact_tail, zero_rows=zero_rows)[0]


# ---------------------------------------------------------------------------------------------
# window-normalised matched filter (no reference counterpart; DESIGN.md 3.3a, csrc/nmf.hip)
# ---------------------------------------------------------------------------------------------
def _nmf_parts(template):
    """(h', |h'|) of a template for the window-normalised matched filter: the support as _normalised_support cuts it, de-meaned
    over the SUPPORT (the zero-padded length and its DC tail have no place here) and scaled by 1 / max|h| (the scale cancels);
    the norm is that of the float32 taps the correlator receives."""
    t = _host_vec(template)
    h = t[:_support(t)]
    a = np.max(np.abs(h))
    if a == 0:
        raise ValueError("template is all zeros")
    if len(h) > int(lib.d4w_nmf_max_support()):
        raise ValueError("the window-normalised matched filter takes supports <= %d samples (got %d)"
                         % (int(lib.d4w_nmf_max_support()), len(h)))
    hp = (h - h.mean()) / a
    return hp, float(np.sqrt(np.sum(hp.astype(np.float32).astype(np.float64) ** 2)))


def _nmf_device(x, taps, norms, center=True, floor=1e-6, stats=None, next_head=None, want_row_max=False):
    """Window-normalised correlograms of the rows of x (float32 CUDA [nx, ns]) -> (list, row maxima or None): the numerator from
    _matched_filter (taps = the de-meaned supports, no tail), then d4w_nmf_normalise_f32 in place, one launch per template pair
    (x read once for both).  stats / next_head as _matched_filter (next_head: any container, see _nmf_head)."""
    nx, ns = x.shape
    next_head = _nmf_head(next_head, nx, max(len(t) for t in taps), x.device)
    if stats is None:
        stats = _row_stats_cached(x)                     # (the statistics the f-k filter deposited, when it ran last)
    outs, _ = _matched_filter(x, taps, [0.0] * len(taps), stats=stats, next_head=next_head)
    rmax = [] if want_row_max else None
    with torch.cuda.device(x.device):
        for i in range(0, len(taps), 2):
            ms = [len(t) for t in taps[i:i + 2]]
            ys, nn = outs[i:i + 2], norms[i:i + 2]
            n_next = max(len(t) for t in taps) - 1 if next_head is not None else 0
            rm = [torch.empty(nx, dtype=torch.float32, device=x.device) for _ in ys] if want_row_max else None
            check(lib.d4w_nmf_normalise_f32(dev.ptr(x), nx, ns, dev.ptr(next_head) if n_next > 0 else None,
                                            int(next_head.stride(0)) if n_next > 0 else 0, n_next, dev.ptr(stats[0]), dev.ptr(stats[1]),
                                            len(ys), ms[0], ms[-1], nn[0], nn[-1], int(bool(center)), float(floor),
                                            dev.out_ptr(ys[0]), dev.out_ptr(ys[1]) if len(ys) > 1 else None,
                                            dev.ptr(rm[0]) if rm else None, dev.ptr(rm[1]) if rm and len(rm) > 1 else None,
                                            dev.stream_ptr(x)))
            if rm:
                rmax.extend(rm)
    return outs, rmax


def _nmf_head(next_head, nx, longest, device):
    """The continuation rows as the kernels read them in place: float32 CUDA [nx, >= longest - 1], unit stride along time."""
    if next_head is None:
        return None
    if getattr(next_head, "ndim", 0) != 2 or next_head.shape[0] != nx or next_head.shape[1] < longest - 1:
        raise ValueError("next_head must be [%d x >= %d] (the rows' continuation, longest support - 1 samples)" % (nx, longest - 1))
    if not (dev.is_tensor(next_head) and next_head.is_cuda and next_head.dtype == torch.float32 and next_head.stride(1) == 1
            and next_head.device == device):
        next_head = dev.to_device_f32(next_head[:, :max(longest - 1, 1)], device)
    return next_head


def compute_nmf_correlograms(data, templates, center=True, floor=1e-6, next_head=None):
    """Window-normalised matched filter of every row against several templates -> a list of [channel x time] correlation
    COEFFICIENTS in [-1, 1], in the caller's container: lag k is the correlation of the template's support h (m samples,
    de-meaned over the support) with the m samples under it, divided by |h'| and by the energy of THOSE samples --
        nmf[k] = sum_n x'[k + n] h'[n] / (|h'| sqrt(V[k])),   V = S2 - S1^2 / m (center=True: the Pearson coefficient) or S2,
    -- instead of by the row's loudest sample (compute_cross_correlogram, detect.py:157): a spike on a channel no longer buries
    that channel's calls, a loud channel no longer sets everybody's threshold, and 0.6 means the same in every file.
    floor: windows whose RMS is below floor x the row's max|x| give 0 (dropouts, constant stretches; a one-tap template gives
    zeros).  next_head: [channel x >= longest support - 1] samples that continue the rows (the next file's head): the last
    lags see them instead of zeros; they are normalised like the row's own samples.  Zeros behind the row count as data.
    pick_times / pick_times_env take the result as it is; the two correlograms of a pair sit back to back (stacked_pair)."""
    if getattr(data, "ndim", 0) != 2:
        raise ValueError("data must be a 2-D [channel x time] array")
    if not (np.isfinite(floor) and floor >= 0):
        raise ValueError("floor must be finite and >= 0")
    parts = [_nmf_parts(t) for t in templates]
    if not parts:
        return []
    xd = dev.to_device_f32(data)
    outs, _ = _nmf_device(xd, [h for h, _ in parts], [n for _, n in parts], center, floor, next_head=next_head)
    return [dev.like_input(o, data) for o in outs]


def compute_nmf_correlogram(data, template, center=True, floor=1e-6, next_head=None):
    """compute_nmf_correlograms for one template."""
    return compute_nmf_correlograms(data, [template], center=center, floor=floor, next_head=next_head)[0]


# ---------------------------------------------------------------------------------------------
# local slant-stack semblance (no reference counterpart; DESIGN.md 3.3b, csrc/semblance.hip)
# ---------------------------------------------------------------------------------------------
def semblance_limits():
    """The largest half aperture M, number of trial slownesses, half window H and |delay| in samples local_semblance takes."""
    import ctypes
    v = [ctypes.c_int() for _ in range(4)]
    check(lib.d4w_semblance_limits(*[ctypes.byref(c) for c in v]))
    return {"half_aperture": v[0].value, "slownesses": v[1].value, "half_window": v[2].value, "abs_delay": v[3].value}


def slowness_delays(slowness, dx, fs, half_aperture):
    """Delay table of plane arrivals for local_semblance: float64 [np, 2M + 1] with d[j, m] = m * slowness[j] * dx * fs samples,
    m = -M .. M.  slowness: signed apparent slownesses in s/m (positive: the arrival is later at higher channel numbers);
    dx: spacing of the selected channels in metres; fs: sampling rate in Hz; half_aperture: M."""
    s = _host_vec(slowness)
    M = int(half_aperture)
    if s.size < 1 or not np.all(np.isfinite(s)):
        raise ValueError("slowness must be a non-empty 1-D list of finite values (s/m)")
    if M != half_aperture or M < 1:
        raise ValueError("half_aperture must be an integer >= 1")
    if not (np.isfinite(dx) and dx > 0 and np.isfinite(fs) and fs > 0):
        raise ValueError("dx and fs must be finite and > 0")
    m = np.arange(-M, M + 1, dtype=np.float64)
    return m[None, :] * s[:, None] * float(dx) * float(fs)


def _split_delays(delays):
    """k = floor(d), f = float32(d - k); a fraction that rounds to 1.0f is carried into k (include/d4w.h)."""
    k = np.floor(delays)
    f = (delays - k).astype(np.float32)
    carry = f >= np.float32(1.0)
    return np.where(carry, k + 1, k), np.where(carry, np.float32(0.0), f).astype(np.float32)


def local_semblance(data, delays, half_window, weights=None, return_all=False):
    """Local slant-stack semblance of a [channel x time] block -> (coh, idx), or (coh, idx, cube) with return_all=True: for every
    channel c and sample t the coherence in [0, 1] of the 2M + 1 neighbouring channels along each of np trial moveouts, the
    largest of them (coh, float32) and the smallest trial that attains it (idx, uint8); cube is every trial's S, float32
    [np, channel, time].  The measure does not depend on amplitude: one threshold serves every channel and file.
        delays: float64 [np, 2M + 1] in samples, slowness_delays(...) or any table whose centre column is 0 (curved moveouts
            are allowed); d is split into k = floor(d) and a float32 fraction f.
        X(c, u) = data[c, u] inside the record, 0 outside; a neighbour c + m outside the block or of weight 0 is absent.
        xi = v0 + f (v1 - v0), v0 = X(c + m, tau + k), v1 = X(c + m, tau + k + 1);  b = sum_m w xi, e = sum_m w xi^2, W = sum_m w
        S_j[c, t] = sum_tau b^2 / (W sum_tau e) over tau in [t - H, t + H] inside the record; 0 where W sum e = 0
    half_window: H >= 0.  weights: [2M + 1] >= 0 with a centre > 0 (default ones).  float32 throughout; window sums only add
    their terms (no running sums), so two runs agree bit for bit.  Non-finite samples give an unspecified result.
    With the slowness list s that made the table: s[idx] is the apparent slowness (its sign: which side of a call's apex;
    the sign change: the closest point of approach), 1 / s[idx] the apparent speed.  Works on strain, on f-k filtered strain
    and on matched-filter correlograms alike.  Results come in the caller's container (NumPy array or CUDA tensor).
    Limits (semblance_limits()): M <= 16, np <= 64, H <= 64, |delay| <= 64 samples; beyond them ValueError."""
    if getattr(data, "ndim", 0) != 2 or data.shape[0] < 1 or data.shape[1] < 1:
        raise ValueError("data must be a 2-D [channel x time] array of at least one channel and one sample")
    lim = semblance_limits()
    d = np.asarray(delays.detach().cpu().numpy() if dev.is_tensor(delays) else delays, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] < 3 or d.shape[1] % 2 == 0:
        raise ValueError("delays must be a 2-D [np x 2M + 1] table with M >= 1")
    npj, n = d.shape
    M = (n - 1) // 2
    if M > lim["half_aperture"]:
        raise ValueError("half aperture %d exceeds the limit of %d channels" % (M, lim["half_aperture"]))
    if npj > lim["slownesses"]:
        raise ValueError("%d trial slownesses exceed the limit of %d" % (npj, lim["slownesses"]))
    if not np.all(np.isfinite(d)) or np.max(np.abs(d)) > lim["abs_delay"]:
        raise ValueError("delays must be finite and within +-%d samples" % lim["abs_delay"])
    if np.any(d[:, M] != 0):
        raise ValueError("the centre column of delays must be 0")
    H = int(half_window)
    if H != half_window or H < 0 or H > lim["half_window"]:
        raise ValueError("half_window must be an integer in 0..%d" % lim["half_window"])
    w = np.ones(n, dtype=np.float32) if weights is None else np.asarray(_host_vec(weights), dtype=np.float32)
    if w.shape != (n,):
        raise ValueError("weights must have 2M + 1 = %d entries" % n)
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("weights must be finite and >= 0")
    if not w[M] > 0:
        raise ValueError("the centre weight must be > 0")
    k, f = _split_delays(d)
    k = np.ascontiguousarray(k, dtype=np.int32)
    f = np.ascontiguousarray(f, dtype=np.float32)
    w = np.ascontiguousarray(w)
    if dev.is_tensor(data) and data.is_cuda and data.dtype == torch.float32 and data.stride(1) == 1 and data.stride(0) >= data.shape[1]:
        xd = data                                        # a column-sliced view is read in place (row pitch)
    else:
        xd = dev.to_device_f32(data)
    nx, ns = xd.shape
    coh = torch.empty((nx, ns), dtype=torch.float32, device=xd.device)
    idx = torch.empty((nx, ns), dtype=torch.uint8, device=xd.device)
    cube = torch.empty((npj, nx, ns), dtype=torch.float32, device=xd.device) if return_all else None
    with torch.cuda.device(xd.device):
        check(lib.d4w_semblance_f32(dev.ptr(xd), int(xd.stride(0)), nx, ns, k.ctypes.data, f.ctypes.data, npj, M, w.ctypes.data, H,
                                    dev.out_ptr(coh), dev.out_ptr(idx), dev.out_ptr(cube) if return_all else None, dev.stream_ptr(xd)))
    if dev.is_tensor(data):
        outs = [o if data.is_cuda else o.to(data.device) for o in ((coh, idx, cube) if return_all else (coh, idx))]
    else:
        outs = [dev.like_input(coh, data), idx.cpu().numpy()]
        if return_all:
            outs.append(dev.like_input(cube, data))
    return tuple(outs)


# ---------------------------------------------------------------------------------------------
# peak picking (d4w_find_peaks_f32; the envelope of the *_env variants is d4w_analytic_f32)
# ---------------------------------------------------------------------------------------------
class PickRows(collections.abc.Sequence):
    """The picks of every channel: a read-only Sequence that behaves like the list of per-channel int64 index arrays the
    reference returns (detect.py:169-274: len(), indexing, slicing, iteration, `in`, reversed(), in channel order), backed
    by ONE packed 2 x K table on the device (`packed`: row 0 = channel, row 1 = time index = detect.convert_pick_times'
    output) and `counts`.  Nothing is copied to the host until a row (or the table) is asked for; the first access copies
    the whole table once.  Deviation from the reference: it is not a `list` instance -- code that needs one (isinstance
    checks, `+`, append, np.asarray(..., dtype=object)) calls .tolist()."""

    def tolist(self):
        """A plain Python list of per-channel int64 ndarrays, exactly the reference's return type."""
        return list(self)

    def __add__(self, other):
        return self.tolist() + list(other)

    def __radd__(self, other):
        return list(other) + self.tolist()

    def __eq__(self, other):
        try:
            return len(self) == len(other) and all(np.array_equal(a, b) for a, b in zip(self, other))
        except TypeError:
            return NotImplemented

    __hash__ = None

    def __init__(self, packed, counts, resolve=None):
        """resolve: a callable returning the packed table, run on first use (pick_times*(..., lazy=True): the picker has
        been launched, the one host synchronisation of the call -- the table's size -- waits until somebody looks)."""
        self._packed, self.counts, self._resolve = packed, counts, resolve
        self._host = None

    @property
    def packed(self):
        if self._packed is None:
            self._packed = self._resolve()
            self._resolve = None
        return self._packed

    def _rows(self):
        if self._host is None:
            cnt = self.counts.cpu().numpy().astype(np.int64)
            self._host = (self.packed[1].cpu().numpy(), np.concatenate(([0], np.cumsum(cnt))))
        return self._host

    def __len__(self):
        return int(self.counts.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        flat, off = self._rows()
        i = int(i)
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError("channel index out of range")
        return flat[off[i]:off[i + 1]]

    def __iter__(self):
        flat, off = self._rows()
        return (flat[off[i]:off[i + 1]] for i in range(len(self)))

    @property
    def total(self):
        return int(self.packed.shape[1])

    def table(self):
        """2 x K int64 ndarray (channel, time): detect.convert_pick_times of these picks."""
        return self.packed.cpu().numpy()


_PICK_CAP = {}                       # (nx, ns) -> index slots per row worth allocating up front
_PICK_CAP_BYTES = 8 << 30            # ... while the index table stays below this


def _find_peaks_device(c, threshold, cap0=1024, lazy=False):
    """c: float32 CUDA [nx, ns] -> PickRows.  One host synchronisation per call (total and largest per-row count);
    the ragged result is compacted on the device.  threshold: a number, a Threshold (formed on the device), or one bar per
    channel (a ChannelThreshold, or nx values as a NumPy array, list or float32 CUDA tensor).  lazy=True:
    the picker is launched and the synchronisation (and the compaction behind it) is left to the first look at the result
    -- a chain over many blocks keeps the device busy and looks at the end; `c` stays alive until then."""
    nx, ns = c.shape
    # the widest row of the last call on this shape is the first guess of the next one: a stream of blocks with dense picks
    # (raw correlograms: thousands per row) would otherwise run the picker twice per block
    hint = _PICK_CAP.get((nx, ns), 0)
    if nx * hint * 4 > _PICK_CAP_BYTES:
        hint = 0
    cap = max(1, min(ns // 2 + 1, max(int(cap0), hint)))
    on_dev = isinstance(threshold, Threshold)
    if on_dev and threshold.value.device != c.device:
        raise ValueError("the threshold's value lives on another device than the block")
    rows = _per_channel(threshold, nx)
    if isinstance(rows, np.ndarray):
        rows = ChannelThreshold(1.0, torch.from_numpy(rows).to(c.device))
    if rows is not None and rows.values.device != c.device:
        raise ValueError("the threshold's values live on another device than the block")
    cnt = torch.empty(nx, dtype=torch.int32, device=c.device)
    off = torch.empty(nx, dtype=torch.int64, device=c.device)
    summ = torch.empty(2, dtype=torch.int64, device=c.device)
    stream = torch.cuda.current_stream(c.device)

    def launch(cap):
        idx = torch.empty((nx, cap), dtype=torch.int32, device=c.device)
        if rows is not None:
            check(lib.d4w_find_peaks_rowthr_f32(dev.ptr(c), nx, ns, dev.ptr(rows.values), rows.scale, dev.ptr(idx),
                                                dev.ptr(cnt), cap, int(stream.cuda_stream)))
        elif on_dev:
            check(lib.d4w_find_peaks_dthr_f32(dev.ptr(c), nx, ns, dev.ptr(threshold.value), threshold.scale, dev.ptr(idx),
                                              dev.ptr(cnt), cap, int(stream.cuda_stream)))
        else:
            check(lib.d4w_find_peaks_f32(dev.ptr(c), nx, ns, float(threshold), dev.ptr(idx), dev.ptr(cnt), cap,
                                         int(stream.cuda_stream)))
        check(lib.d4w_pick_offsets_i64(dev.ptr(cnt), nx, dev.ptr(off), dev.ptr(summ), int(stream.cuda_stream)))
        return idx

    def finish(idx, cap):
        with torch.cuda.device(c.device), torch.cuda.stream(stream):
            while True:
                need, total = (int(v) for v in summ.cpu())       # the call's one host synchronisation (a 16-byte copy)
                _PICK_CAP[(nx, ns)] = need + need // 4 + 16 if need > cap0 else 0
                if need <= cap:
                    break
                cap = min(ns // 2 + 1, max(need, 2 * cap))      # rare: a row with more peaks than the first guess
                idx = launch(cap)
            packed = torch.empty((2, total), dtype=torch.int64, device=c.device)
            check(lib.d4w_pack_picks_i64(dev.ptr(idx), dev.ptr(cnt), dev.ptr(off), nx, cap, total,
                                         dev.ptr(packed) if total else None, int(stream.cuda_stream)))
        return packed

    with torch.cuda.device(c.device):
        idx = launch(cap)
    if lazy:
        return PickRows(None, cnt, resolve=lambda: finish(idx, cap))
    return PickRows(finish(idx, cap), cnt)


def pick_times_env(corr_m, threshold, lazy=False):
    """Per row find_peaks(|hilbert(corr)|, prominence=threshold)[0] -- reference detect.py:169-195.  threshold: a number, a
    Threshold (formed on the device) or one bar per channel (a ChannelThreshold, or nx values as a NumPy array, list or float32
    CUDA tensor: row c is picked with prominence=threshold[c]); lazy: see _find_peaks_device (both beyond the reference's signature)."""
    from . import dsp
    if getattr(corr_m, "ndim", 0) != 2:
        raise ValueError("corr_m must be a 2-D [channel x time] array")
    _per_channel(threshold, int(corr_m.shape[0]))
    env = dsp._analytic(dev.to_device_f32(corr_m), 0)
    return _find_peaks_device(env, threshold, lazy=lazy)


def process_corr(corr, threshold):
    """One row of pick_times_env -- reference detect.py:198-218."""
    c = corr if dev.is_tensor(corr) else np.asarray(corr)
    return pick_times_env(c.reshape(1, -1), threshold)[0]


def pick_times_par(corr_m, threshold):
    """pick_times_env; the reference's thread-pool variant (detect.py:221-246) returns rows in
    completion order, here rows come back in channel order."""
    return pick_times_env(corr_m, threshold)


def pick_times(corr_m, threshold, lazy=False):
    """Per row find_peaks(corr, prominence=threshold)[0] -- reference detect.py:249-274 (threshold / lazy: pick_times_env)."""
    if getattr(corr_m, "ndim", 0) != 2:
        raise ValueError("corr_m must be a 2-D [channel x time] array")
    _per_channel(threshold, int(corr_m.shape[0]))
    return _find_peaks_device(dev.to_device_f32(corr_m), threshold, lazy=lazy)


# ---------------------------------------------------------------------------------------------
# STA/LTA energy detector and trigger events (no reference counterpart; DESIGN.md 3.3c, csrc/stalta.hip)
# ---------------------------------------------------------------------------------------------
_STALTA_FORMS = {"classic": 0, "recursive": 1}


class StaLtaState:
    """What sta_lta / trigger_onset / sta_lta_events of block k hand to block k + 1 (opaque): the last max(nsta, nlta + gap) - 1
    samples of every row (classic form; fewer while the record is shorter), the float64 (sta, lta) of every row and the number
    of samples seen (recursive form), the trigger's active flag of every row (None before a trigger has run)."""

    __slots__ = ("key", "tail", "rec", "seen", "active")

    def __init__(self, key, tail=None, rec=None, seen=0, active=None):
        self.key, self.tail, self.rec, self.seen, self.active = key, tail, rec, int(seen), active

    def with_active(self, active):
        return StaLtaState(self.key, self.tail, self.rec, self.seen, active)


def _stalta_check(data, nsta, nlta, gap, form, floor):
    if getattr(data, "ndim", 0) != 2:
        raise ValueError("x must be a 2-D [channel x time] array")
    if form not in _STALTA_FORMS:
        raise ValueError("form must be 'classic' or 'recursive', not %r" % (form,))
    for name, v in (("nsta", nsta), ("nlta", nlta), ("gap", gap)):
        if int(v) != v:
            raise ValueError("%s must be a whole number of samples" % name)
    nsta, nlta, gap = int(nsta), int(nlta), int(gap)
    wmax = int(lib.d4w_stalta_max_window())
    if nsta < 1 or nlta < 1 or gap < 0:
        raise ValueError("nsta and nlta must be at least 1 and gap at least 0")
    if form == "recursive" and gap != 0:
        raise ValueError("the recursive form takes gap = 0")
    if nlta + gap > wmax or nsta > wmax:
        raise ValueError("nlta + gap (and nsta) must not exceed %d samples" % wmax)
    if not (np.isfinite(floor) and floor >= 0):
        raise ValueError("floor must be finite and >= 0")
    return nsta, nlta, gap


def _rows_in_place(x):
    """x as the kernels read it: a float32 CUDA tensor with unit time stride and a row pitch stays as it is."""
    if dev.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 \
            and (x.shape[0] == 1 or x.stride(0) >= x.shape[1]):
        return x
    return dev.to_device_f32(x)


def _stalta_scale(xd, scale):
    nx = xd.shape[0]
    if scale is None:                                        # the row's max|x| in this block
        xc = xd if xd.is_contiguous() else dsp._copy_cols(xd, torch.empty(tuple(xd.shape), dtype=torch.float32, device=xd.device))
        return _row_stats_cached(xc)[1]
    s = scale.to(device=xd.device, dtype=torch.float32).contiguous() if dev.is_tensor(scale) \
        else torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32)).to(xd.device)
    if s.dim() != 1 or s.numel() != nx:
        raise ValueError("scale needs one value for each of the %d channels" % nx)
    return s


def _event_bars(thr, nx, device):
    """A trigger threshold (a number, a Threshold, a ChannelThreshold, nx values) as nx float64 values on the device."""
    rows = _per_channel(thr, nx)
    if rows is None:
        return torch.full((nx,), float(thr), dtype=torch.float64, device=device)
    if isinstance(rows, ChannelThreshold):
        if rows.values.device != device:
            raise ValueError("the threshold's values live on another device than the block")
        return rows.values.to(torch.float64) * rows.scale      # the product in float64, as the pickers form it
    return torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)).to(device)


def _event_thresholds(thr_on, thr_off, nx, device):
    on, off = _event_bars(thr_on, nx, device), _event_bars(thr_off, nx, device)
    if bool((off > on).any()):
        raise ValueError("thr_off must not exceed thr_on on any channel")
    return on, off


class EventRows(collections.abc.Sequence):
    """The trigger events of every channel: a read-only Sequence of per-channel [n, 3] int64 arrays (on, off, peak_index), backed
    by one packed 4 x K table on the device (`packed`: channel, on, off, peak_index) and the K peak values (`packed_peak`);
    nothing is copied to the host until a row, .table() or .peak is asked for.  on = -1: the event was active on entry;
    off = ns: it is still open at the end of the block."""

    def __init__(self, packed, packed_peak, counts):
        self.packed, self.packed_peak, self.counts = packed, packed_peak, counts
        self._host = None

    def _rows(self):
        if self._host is None:
            cnt = self.counts.cpu().numpy().astype(np.int64)
            self._host = (np.ascontiguousarray(self.packed[1:].cpu().numpy().T), np.concatenate(([0], np.cumsum(cnt))))
        return self._host

    def __len__(self):
        return int(self.counts.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        flat, off = self._rows()
        i = int(i)
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError("channel index out of range")
        return flat[off[i]:off[i + 1]]

    @property
    def total(self):
        return int(self.packed.shape[1])

    def table(self):
        """4 x K int64 ndarray: channel, on, off, peak_index."""
        return self.packed.cpu().numpy()

    @property
    def peak(self):
        """The K float32 peak values, in the table's order."""
        return self.packed_peak.cpu().numpy()

    def picks(self, which="on"):
        """The events as picks -- a PickRows, taken by everything that takes pick_times' result (convert_pick_times,
        select_picked_times, loc.associate_picks, shard.all_gather_picks): which="on" the onsets (an event that was already
        active on entry, on = -1, contributes none), which="peak" the peak positions."""
        if which == "peak":
            return PickRows(self.packed[[0, 3]].contiguous(), self.counts)
        if which != "on":
            raise ValueError("which must be 'on' or 'peak'")
        keep = self.packed[1] >= 0
        cnt = self.counts.to(torch.int64) - torch.bincount(self.packed[0][~keep], minlength=len(self))
        return PickRows(self.packed[:2][:, keep].contiguous(), cnt.to(torch.int32))


def _stalta_device(xd, nsta, nlta, gap, form, floor, scale, state, want_ratio, bars=None, cap0=1024):
    """One pass of csrc/stalta.hip over xd (float32 CUDA [nx, ns], any row pitch) -> (ratio or None, EventRows or None, the
    state after the block).  bars: (thr_on, thr_off) float64 device tensors -- the trigger runs on the ratios in registers."""
    nx, ns = xd.shape
    device = xd.device
    key = (form, nsta, nlta, gap)
    if isinstance(state, StaLtaState) and state.key is None:         # a flag from trigger_onset alone
        state = StaLtaState(key, active=state.active)
    if state is not None and (not isinstance(state, StaLtaState) or state.key != key):
        raise ValueError("state comes from a call with other parameters (form, nsta, nlta, gap)")
    classic = form == "classic"
    A = _stalta_scale(xd, scale)
    need = max(nsta, nlta + gap) - 1
    tail = state.tail if state is not None and classic else None
    if tail is not None and (tail.shape[0] != nx or tail.device != device):
        raise ValueError("state belongs to a block of another shape or device")
    rin = state.rec if state is not None and not classic else None
    seen = state.seen if state is not None else 0
    rout = torch.empty((nx, 2), dtype=torch.float64, device=device) if not classic else None
    ratio = torch.empty((nx, ns), dtype=torch.float32, device=device) if want_ratio else None
    act_in = state.active if state is not None and bars is not None else None
    stream = torch.cuda.current_stream(device)
    events = act_out = None

    def launch(cap):
        ev = pk = cnt = None
        if bars is not None:
            ev = torch.empty((nx, cap, 3), dtype=torch.int32, device=device)
            pk = torch.empty((nx, cap), dtype=torch.float32, device=device)
            cnt = torch.empty(nx, dtype=torch.int32, device=device)
        o = lambda t: dev.ptr(t) if t is not None else None
        check(lib.d4w_stalta_f32(dev.ptr(xd), int(xd.stride(0)) if nx > 1 else ns, nx, ns, o(tail), int(tail.stride(0)) if tail is not None else 0,
                                 int(tail.shape[1]) if tail is not None else 0, _STALTA_FORMS[form], nsta, nlta, gap, float(floor),
                                 dev.ptr(A), o(rin), o(rout), seen, o(ratio), ns if ratio is not None else 0,
                                 o(bars[0]) if bars else None, o(bars[1]) if bars else None, o(act_in), o(act_out), o(ev), o(pk), o(cnt),
                                 cap, int(stream.cuda_stream)))
        return ev, pk, cnt

    with torch.cuda.device(device):
        if bars is not None:
            act_out = torch.empty(nx, dtype=torch.int32, device=device)
            events = _pack_events(launch, nx, ns, cap0, device, stream)
        else:
            launch(0)
        # the tail is COPIED out (one strided-copy launch): a view would keep the whole block alive for one more call
        new_tail = None
        if classic and need > 0:
            if ns >= need:
                new_tail = dsp._copy_cols(xd[:, ns - need:], torch.empty((nx, need), dtype=torch.float32, device=device))
            else:
                keep = min(need - ns, tail.shape[1]) if tail is not None else 0
                new_tail = dsp._concat_cols(([tail[:, tail.shape[1] - keep:]] if keep else []) + [xd])
    return ratio, events, StaLtaState(key, new_tail, rout, seen + ns, act_out)


def _pack_events(launch, nx, ns, cap0, device, stream):
    """Run launch(cap) -> (ev, peak, counts) until every row's events fit, then pack the rows: one host synchronisation."""
    cap = max(1, min(ns // 2 + 1, int(cap0)))
    off = torch.empty(nx, dtype=torch.int64, device=device)
    summ = torch.empty(2, dtype=torch.int64, device=device)
    while True:
        ev, pk, cnt = launch(cap)
        check(lib.d4w_pick_offsets_i64(dev.ptr(cnt), nx, dev.ptr(off), dev.ptr(summ), int(stream.cuda_stream)))
        with torch.cuda.stream(stream):
            need, total = (int(v) for v in summ.cpu())
        if need <= cap:
            break
        cap = min(ns // 2 + 1, max(need, 2 * cap))
    packed = torch.empty((4, total), dtype=torch.int64, device=device)
    peaks = torch.empty(total, dtype=torch.float32, device=device)
    check(lib.d4w_pack_events_i64(dev.ptr(ev), dev.ptr(pk), dev.ptr(cnt), dev.ptr(off), nx, cap, total,
                                  dev.ptr(packed) if total else None, dev.ptr(peaks) if total else None, int(stream.cuda_stream)))
    return EventRows(packed, peaks, cnt)


def sta_lta(x, nsta, nlta, *, gap=0, form="classic", floor=1e-6, scale=None, state=None, return_state=False):
    """STA/LTA ratio of the energy e = x^2 of every row of a [channel x time] block, in the caller's container (a float32 CUDA
    tensor with unit time stride and a row pitch is read in place):
        form="classic"    STA[i] = mean e[i-nsta+1 .. i],  LTA[i] = mean e[i-gap-nlta+1 .. i-gap]  (the gap keeps a call out of
                          its own noise estimate);  r = STA / LTA where both windows lie in known samples and LTA > (floor A)^2
        form="recursive"  sta[i] = sta[i-1] + (e[i] - sta[i-1]) / nsta, lta likewise with nlta (gap = 0), both from 0 or from
                          `state`;  r = sta / lta once nlta samples have been seen and lta > (floor A)^2
    and 0 elsewhere.  A = scale[c] when `scale` holds one value per channel (a noise level, or a fixed level for a stream of
    files), else the row's max|x| in this block: results do not depend on the row's gain; dropouts and dead channels give 0.
    state: the StaLtaState an earlier call returned with return_state=True -- the block then continues that record, and the
    result equals the one call on the concatenation.  nlta + gap (and nsta) <= d4w_stalta_max_window() = 16384.  Inputs are
    finite: a NaN or Inf sample gives unspecified ratios downstream of it."""
    nsta, nlta, gap = _stalta_check(x, nsta, nlta, gap, form, floor)
    ratio, _, new = _stalta_device(_rows_in_place(x), nsta, nlta, gap, form, floor, scale, state, True)
    if state is not None:
        new = new.with_active(state.active)
    out = dev.like_input(ratio, x)
    return (out, new) if return_state else out


def trigger_onset(r, thr_on, thr_off, *, state=None, return_state=False, _cap0=1024):
    """Events of every row of the ratio r ([channel x time]): a sample is ON if r > thr_on[c], OFF if r < thr_off[c], KEEP
    otherwise (a NaN keeps); the flag after a sample is the last ON / OFF at or before it, else the flag `state` carries in.
    An event is a maximal run of active samples -> EventRows of (on, off, peak_index) per channel, `.peak` the largest r of
    every run.  thr_on / thr_off: numbers or one value per channel, in the forms pick_times takes (ChannelThreshold included);
    thr_off <= thr_on per channel.  return_state=True: also the state with the flag after the last sample."""
    if getattr(r, "ndim", 0) != 2:
        raise ValueError("r must be a 2-D [channel x time] array")
    rd = _rows_in_place(r)
    nx, ns = rd.shape
    if state is not None and not isinstance(state, StaLtaState):
        raise ValueError("state must be a StaLtaState")
    on, off = _event_thresholds(thr_on, thr_off, nx, rd.device)
    act_in = state.active if state is not None else None
    stream = torch.cuda.current_stream(rd.device)
    with torch.cuda.device(rd.device):
        act_out = torch.empty(nx, dtype=torch.int32, device=rd.device)

        def launch(cap):
            ev = torch.empty((nx, cap, 3), dtype=torch.int32, device=rd.device)
            pk = torch.empty((nx, cap), dtype=torch.float32, device=rd.device)
            cnt = torch.empty(nx, dtype=torch.int32, device=rd.device)
            check(lib.d4w_trigger_onset_f32(dev.ptr(rd), int(rd.stride(0)) if nx > 1 else ns, nx, ns, dev.ptr(on), dev.ptr(off),
                                            dev.ptr(act_in) if act_in is not None else None, dev.ptr(act_out), dev.ptr(ev), dev.ptr(pk),
                                            dev.ptr(cnt), cap, int(stream.cuda_stream)))
            return ev, pk, cnt
        events = _pack_events(launch, nx, ns, _cap0, rd.device, stream)
    if not return_state:
        return events
    new = state.with_active(act_out) if state is not None else StaLtaState(None, active=act_out)
    return events, new


def sta_lta_events(x, nsta, nlta, thr_on, thr_off, *, gap=0, form="classic", floor=1e-6, scale=None, state=None, return_state=False,
                   _cap0=1024):
    """trigger_onset(sta_lta(x, ...), thr_on, thr_off) in ONE read of x and no ratio written (4 B per sample instead of 8 + 4):
    the ratios are formed by the same device function and handed to the trigger in registers -- the events equal the
    composition's exactly.  Arguments as sta_lta and trigger_onset; the state carries the samples and the flag."""
    nsta, nlta, gap = _stalta_check(x, nsta, nlta, gap, form, floor)
    xd = _rows_in_place(x)
    bars = _event_thresholds(thr_on, thr_off, xd.shape[0], xd.device)
    _, events, new = _stalta_device(xd, nsta, nlta, gap, form, floor, scale, state, False, bars=bars, cap0=_cap0)
    return (events, new) if return_state else events


# ---------------------------------------------------------------------------------------------
# spectrogram correlation
# ---------------------------------------------------------------------------------------------
def _keep_bins(fs, nperseg, fmin, fmax):
    ff = np.linspace(0, fs / 2, num=nperseg // 2 + 1)                            # detect.py:386
    keep = np.where((ff >= fmin) & (ff <= fmax))[0]                              # detect.py:390
    if len(keep) == 0:
        raise ValueError("no STFT bin between fmin = %g and fmax = %g" % (fmin, fmax))
    return ff, int(keep[0]), int(keep[-1])


def get_sliced_nspectrogram(trace, fs, fmin, fmax, nperseg, nhop, plotflag=False):
    """|librosa.stft(trace, nperseg, nhop)| / max, rows with fmin <= f <= fmax; returns (p, ff, tt)
    -- reference detect.py:334-408 (plotflag is a plotting path of the reference and is ignored)."""
    from . import dsp
    if getattr(trace, "ndim", 0) != 1:
        raise ValueError("trace must be 1-D")
    ff, lo, hi = _keep_bins(fs, nperseg, fmin, fmax)
    x = dev.to_device_f32(trace.reshape(1, -1))
    S, mx = dsp._stft_mag(x, nperseg, nhop, lo, hi)
    dsp._scale_rows(S, mx, 0)                                                   # detect.py:387
    tt = np.linspace(0, trace.shape[0] / fs, num=S.shape[2])                    # detect.py:385
    return dev.like_input(S[0], trace), ff[lo:hi + 1], tt


def buildkernel(f0, f1, bdwdth, dur, f, t, samp, fmin, fmax, plotflag=False):
    """Hat-function kernel along a hyperbolic down-sweep, Hann-weighted in time; returns
    (tvec, fvec, BlueKernel) -- reference detect.py:411-492 (host, a few hundred values)."""
    t = np.asarray(t)
    tvec = np.linspace(0, dur, np.size(np.nonzero((t < dur * 8) & (t > dur * 7))))      # detect.py:456
    fvec = np.asarray(f)
    x = fvec[:, None] - (f0 * f1 * dur / ((f0 - f1) * tvec[None, :] + f1 * dur))        # detect.py:470
    kdist = (1 - np.square(x) / (bdwdth * bdwdth)) * np.exp(-np.square(x) / (2 * (bdwdth * bdwdth)))
    return tvec, fvec, kdist * np.hanning(len(tvec))[np.newaxis, :]                     # detect.py:474


def buildkernel_from_template(fmin, fmax, dur, fs, nperseg, nhop, plotflag=False):
    """Sliced normalised spectrogram of the windowed hyperbolic chirp -- reference detect.py:495-541."""
    template = gen_hyperbolic_chirp(fmin, fmax, dur, fs)
    template *= np.hanning(len(template))
    spectro, _, _ = get_sliced_nspectrogram(template, fs, fmin, fmax, nperseg, nhop, plotflag=False)
    return spectro


_kernel_memo = {}       # (kernel bytes, shape, device) -> device copy of a spectrogram-correlation kernel


def _kernel_on_device(K, device):
    key = (K.tobytes(), K.shape, str(device))
    with _cache_lock:
        Kd = _kernel_memo.get(key)
        if Kd is None:
            if len(_kernel_memo) > 16:
                _kernel_memo.clear()
            Kd = _kernel_memo[key] = torch.from_numpy(K).to(device)
    return Kd


def _spectrocorr_device(S, K, off, nout, med=None, zero_ends=False, out=None):
    """S: float32 CUDA [nx, nf, nt]; K: host [nf, nk] -> CUDA [nx, nout] (include/d4w.h d4w_spectrocorr_f32).
    out: optional contiguous [nx, nout] float32 CUDA rows to write into (a slice of a larger result)."""
    nx, nf, nt = S.shape
    K = np.ascontiguousarray(K, dtype=np.float32)
    if K.ndim != 2 or K.shape[0] != nf:
        raise ValueError("kernel has %s rows, the spectrogram %d" % (K.shape[:1], nf))
    Kd = _kernel_on_device(K, S.device)          # the same few hundred values file after file: uploaded once
    if out is None:
        out = torch.empty((nx, nout), dtype=torch.float32, device=S.device)
    with torch.cuda.device(S.device):
        if med is None:
            med = torch.empty(nx, dtype=torch.float32, device=S.device)
            check(lib.d4w_row_median_f32(dev.ptr(S), nx, nf * nt, dev.ptr(med), dev.stream_ptr(S)))   # detect.py:600
        check(lib.d4w_spectrocorr_f32(dev.ptr(S), nx, nf, nt, dev.ptr(Kd), K.shape[1], int(off), int(nout),
                                      dev.ptr(med), int(bool(zero_ends)), dev.ptr(out), dev.stream_ptr(S)))
        # Kd is a temporary on the stream the kernel runs on: the caching allocator re-uses it in stream order, no
        # host synchronisation (a stream of files stays asynchronous)
    return out


def _spectro_2d(spectro):
    if getattr(spectro, "ndim", 0) != 2:
        raise ValueError("spectro must be a 2-D [frequency x time] array")
    return dev.to_device_f32(spectro)[None]


def xcorr2d(spectro, kernel):
    """sum_f fftconvolve(spectro, flip(kernel, 1), 'same', axes=1), clipped at 0,
    / (median(spectro) * kernel.shape[1]) -- reference detect.py:579-602."""
    S = _spectro_2d(spectro)
    kernel = np.asarray(kernel)
    out = _spectrocorr_device(S, kernel, kernel.shape[1] // 2, S.shape[2])
    return dev.like_input(out[0], spectro)


def xcorr(t, f, Sxx, tvec, fvec, BlueKernel):
    """Valid-lag kernel x spectrogram correlation; returns [t_scale, CorrVal] -- reference detect.py:605-647."""
    nk, nfk = np.size(tvec), np.size(fvec)
    S = _spectro_2d(Sxx)
    med = torch.empty(1, dtype=torch.float32, device=S.device)
    with torch.cuda.device(S.device):                           # np.median(Sxx) is over the whole spectrogram
        check(lib.d4w_row_median_f32(dev.ptr(S), 1, S[0].numel(), dev.ptr(med), dev.stream_ptr(S)))
    S = S[:, :nfk].contiguous()                                 # detect.py:636: Sxx[:fvec_size, ...]
    nout = np.size(t) - (nk - 1)
    out = _spectrocorr_device(S, np.asarray(BlueKernel)[:nfk], 0, nout, med=med, zero_ends=True)
    t = np.asarray(t)
    t_scale = t[int(nk / 2) - 1:-int(np.ceil(nk / 2))]          # detect.py:645
    return [t_scale, dev.like_input(out[0], Sxx)]


def nxcorr2d(spectro, kernel):
    """max over the frequency lag of correlate(spectro, kernel, 'same') / (std(spectro) std(kernel) nt)
    -- reference detect.py:544-576.  One d4w_spectrocorr_f32 launch per frequency lag."""
    S = _spectro_2d(spectro)
    K = np.asarray(kernel, dtype=np.float64)
    nf, nt = S.shape[1], S.shape[2]
    nfk, nk = K.shape
    var = torch.empty(1, dtype=torch.float32, device=S.device)
    with torch.cuda.device(S.device):
        check(lib.d4w_row_var_f32(dev.ptr(S), 1, nf * nt, dev.ptr(var), dev.stream_ptr(S)))
    # out = raw / (med * nk) with med chosen so that the divisor is std(S) std(K) nt
    med = torch.sqrt(var) * float(np.std(K) * nt / nk)
    best = None
    for a in range(nf):                                          # output row a: K row fk meets S row a + fk - nfk//2
        Ka = np.zeros((nf, nk))
        lo = a - nfk // 2
        for fk in range(nfk):
            if 0 <= lo + fk < nf:
                Ka[lo + fk] = K[fk]
        # clipping at 0 is harmless only when the max is >= 0; keep exact semantics via two signs
        pos = _spectrocorr_device(S, Ka, nk // 2, nt, med=med)
        neg = _spectrocorr_device(S, -Ka, nk // 2, nt, med=med)
        row = pos - neg
        best = row if best is None else torch.maximum(best, row)
    return dev.like_input(best[0], spectro)


def compute_cross_correlogram_spectrocorr(data, fs, flims, kernel, win_size, overlap_pct):
    """Per-channel sliced spectrogram x hat kernel correlation -- reference detect.py:650-709.
    All channels go through one STFT launch, one median launch and one correlation launch; the
    spectrogram's max-normalisation (detect.py:387) cancels between numerator and median."""
    from . import dsp
    if getattr(data, "ndim", 0) != 2:
        raise ValueError("data must be a 2-D [channel x time] array")
    nperseg = int(win_size * fs)                                                 # detect.py:680
    nhop = int(np.floor(nperseg * (1 - overlap_pct)))                            # detect.py:681
    fmin, fmax = flims
    f1, f0, duration, bandwidth = kernel["f1"], kernel["f0"], kernel["dur"], kernel["bdwidth"]
    if fmax - f1 < 2 * bandwidth:                                                # detect.py:693-696
        fmax = f1 + 3 * bandwidth
    if f0 - fmin < 2 * bandwidth:
        fmin = f0 - 3 * bandwidth
    ff, lo, hi = _keep_bins(fs, nperseg, fmin, fmax)
    x = dev.to_device_f32(data)
    nx, ns = x.shape
    nt = int(lib.d4w_stft_frames(ns, nhop))
    tt = np.linspace(0, ns / fs, num=nt)                                         # detect.py:385
    _, _, ker = buildkernel(f0, f1, bandwidth, duration, ff[lo:hi + 1], tt, fs, fmin, fmax)   # detect.py:702
    out = torch.empty((nx, nt), dtype=torch.float32, device=x.device)
    per_ch = (hi - lo + 1) * nt * 4
    step = int(max(1, min(65535, (2 << 30) // per_ch)))          # <= 2 GiB of spectrogram in flight
    for a in range(0, nx, step):
        S, _ = dsp._stft_mag(x[a:a + step], nperseg, nhop, lo, hi, want_max=False)     # the max-normalisation cancels (docstring)
        _spectrocorr_device(S, ker, ker.shape[1] // 2, nt, out=out[a:a + step])        # rows a.. of the result, in place
    return dev.like_input(out, data)


# ---------------------------------------------------------------------------------------------
# pick utilities (index bookkeeping, host)
# ---------------------------------------------------------------------------------------------
def convert_pick_times(peaks_indexes_m):
    """Ragged per-channel index lists -> 2 x K array, row 0 = channel index, row 1 = time index
    -- reference detect.py:277-303."""
    if isinstance(peaks_indexes_m, PickRows):
        return peaks_indexes_m.table()
    ch = [np.full(len(p), i, dtype=np.int64) for i, p in enumerate(peaks_indexes_m)]
    if not ch:
        return np.zeros((2, 0), dtype=np.int64)
    return np.asarray((np.concatenate(ch), np.concatenate([np.asarray(p, dtype=np.int64) for p in peaks_indexes_m])))


def select_picked_times(idx_tp, tstart, tend, fs):
    """Keep picks with tstart*fs <= time index <= tend*fs -- reference detect.py:306-330."""
    keep = (idx_tp[1] >= tstart * fs) & (idx_tp[1] <= tend * fs)
    return (idx_tp[0][keep], idx_tp[1][keep])
