"""The reference's `tools` namespace (src/das4whales/tools.py): the three functions that compute something.

  disp_comprate(fk_filter)            tools.py:239-258   sizes of the sparse and the dense f-k mask
  spec(da)                            tools.py:212-236   Welch PSD of every 3000-sample chunk (fs = 200, nperseg = 1024)
  energy_TimeDomain(da, time_dim)     tools.py:84-157    sum of squares of every time chunk

spec and energy_TimeDomain run in csrc/welch.hip (one read of the block); dsp.welch_psd is the general form of spec.
The reference maps both over the dask chunks of an xarray.DataArray; here `da` is a 1-D [time] or 2-D [channel x time]
array or CUDA tensor and the chunk length is an argument.

Not mirrored, and no stubs (as with improcess.detect_long_lines):
  fk_filt_chunk, fk_filt, filtfilt, filtfilt_chunk   xarray map_blocks wrappers around arithmetic this package has in
      dsp.fk_filt and dsp.sosfiltfilt; they return xarray objects and are inexact at chunk edges by their own account
      (tools.py:164)
  _energy_TimeDomain_chunk, __spec_chunk             private per-chunk helpers of the two functions above
"""
import numpy as np
import torch

from . import _device as dev
from . import dsp
from ._lib import lib, check

_GIB = float(1024 ** 3)
_SPEC_FS, _SPEC_NPERSEG, _SPEC_CHUNK = 200, 1024, 3000          # hard-coded in the reference (tools.py:224,234)


def disp_comprate(fk_filter):
    """Print the sizes of the f-k mask as a sparse and as a dense float64 matrix and their ratio: the reference's three
    lines (tools.py:255-257).  fk_filter: what the designers of dsp return (DeviceMask / DesignedMask), a dense ndarray,
    or anything with `.data` and `.todense()` (sparse.COO).  A mask of this package is counted on the device
    (`.nnz`, `.shape`): neither its non-zero values nor its dense form cross PCIe to print two sizes."""
    if isinstance(fk_filter, dsp.DeviceMask):
        unformed = fk_filter._tensor is None                    # a DesignedMask nobody has asked the dense form of
        nnz, size = fk_filter.nnz, int(np.prod(fk_filter.shape))
        if unformed:
            fk_filter._tensor = None                            # counted on the device and dropped again: printing two
        size_sprfilt_coo = nnz * 8 / _GIB                       # sizes must not leave 4 nx ns bytes allocated
        sizefilt = size * 8 / _GIB                              # (float64 values, as the reference would hold)
    elif hasattr(fk_filter, "todense") and hasattr(fk_filter, "data"):
        size_sprfilt_coo = fk_filter.data.nbytes / _GIB
        densefk_filter = fk_filter.todense()
        sizefilt = densefk_filter.size * densefk_filter.itemsize / _GIB
    else:
        a = np.asarray(fk_filter)
        size_sprfilt_coo = int(np.count_nonzero(a)) * 8 / _GIB
        sizefilt = a.size * 8 / _GIB
    print(f'The size of the sparse filter is {size_sprfilt_coo:.4f} Gib')
    print(f'The size of the dense filter is {sizefilt:.2f} Gib')
    print(f'The compression ratio is {sizefilt / size_sprfilt_coo:.2f} ({abs(sizefilt - size_sprfilt_coo) *100 / sizefilt:.1f} %)')
    return


def spec(da):
    """Welch PSD of every whole 3000-sample chunk of `da`, as the reference's hard-coded case computes it
    (scipy.signal.welch(chunk, fs=200, nperseg=1024), tools.py:224-234).  [ns] -> [int(ns / 3000), 513], the values of
    the reference's DataArray; [nx, ns] -> [nx, int(ns / 3000), 513]."""
    x2, was1d = dsp._rows_2d(da)
    pxx = dsp._welch(dev.to_device_f32(x2), _SPEC_FS, _SPEC_NPERSEG, _SPEC_NPERSEG // 2, _SPEC_CHUNK)
    return dev.like_input(pxx[0] if was1d else pxx, da)


def energy_TimeDomain(da, time_dim='time', *, chunk=None):
    """Sum of squares of every chunk of `chunk` samples along time, the last axis (tools.py:84-157; the reference takes
    the chunks from the dask array).  The last chunk may be short; chunk=None: one chunk, the whole record.
    [ns] -> [nchunks]; [nx, ns] -> [nx, nchunks]."""
    if time_dim != 'time':
        raise ValueError("time is the last axis of the array: time_dim = %r is not supported" % (time_dim,))
    x2, was1d = dsp._rows_2d(da)
    x = dev.to_device_f32(x2)
    nx, ns = x.shape
    chunk = ns if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk = %d must be positive" % chunk)
    e = torch.empty((nx, -(-ns // chunk)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.d4w_chunk_energy_f32(dev.ptr(x), nx, ns, chunk, dev.ptr(e), dev.stream_ptr(x)))
    return dev.like_input(e[0] if was1d else e, da)
