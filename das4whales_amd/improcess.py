"""improcess -- the image pipeline of the Gabor detector: the part of the
reference's `das4whales.improcess` that scripts/main_gabordetect.py:78-166 runs, on the GPU.

    image    = trace2image(trf_fk)                         |hilbert| / std, min-max scaled to [0, 255]
    imagebin = binning(image, 1/10, 1/10)                  torchvision Resize (antialiased bilinear)
    up, down = gabor_filt_design(angle_fromspeed(c0, fs, dx, selected_channels))
    fimage   = filter2d(imagebin, up) + filter2d(imagebin, down)          (cv2.filter2D in the script)
    mask     = (filter2d(fimage > thr, up) + filter2d(fimage > thr, down)) > thr2
    masked   = apply_smooth_mask(trf_fk, binning(mask, 10, 10))

`gabor_mask` runs those steps in one call with everything resident on the device.  cv2 and torchvision
are not used (and not installed): `gabor_filt_design` evaluates OpenCV's getGaborKernel formula on the
host in float64, `filter2d` and `binning` are HIP kernels (csrc/image.hip) that follow cv2.filter2D
(correlation, BORDER_REFLECT_101) and aten's antialiased bilinear interpolation.

`compute_radon_transform` (improcess.py:347-367) is skimage.transform.radon(image, theta, circle=False)
as a HIP kernel (csrc/radon.hip).

The image operators outside the detector are HIP kernels too (csrc/edges.hip):

    gradient_oriented(image, direction)          improcess.py:143-169   recorded from the reference
    detect_diagonal_edges(matrix, threshold)     improcess.py:172-226   recorded from the reference
    diagonal_edge_detection(img, threshold)      improcess.py:229-266   recorded from the reference
    gaussian_filter(img, size, sigma)            improcess.py:370-392   documented definition, unpinned
    bilateral_filter(img, diameter, sigma_color, sigma_space)   :319-344   documented definition, unpinned

The first three are tested against outputs recorded from the reference itself (tests/golden/edges.npz).  The last
two are cv2.GaussianBlur and cv2.bilateralFilter; cv2 is not installed, so they follow OpenCV's documented
definitions (tests/known_answers_smooth.py) and their agreement with a real cv2 is not measured.  Only
`detect_long_lines` (Canny + randomised probabilistic Hough + plt.show()) is out of scope.  Arrays: NumPy
in -> NumPy out (float dtype kept, compute in float32), CUDA tensor in -> CUDA tensor out; masks are
bool.
"""
import ctypes
import operator

import numpy as np
import torch

from . import _device as dev
from . import dsp
from ._lib import lib, check


def _n(t):
    return int(t.numel())


def _minmax(x):
    mm = torch.empty(2, dtype=torch.float32, device=x.device)
    check(lib.d4w_minmax_f32(dev.ptr(x), _n(x), dev.ptr(mm), dev.stream_ptr(x)))
    return mm


def _scale_pixels_device(x, gain, out=None):
    y = torch.empty_like(x) if out is None else out
    with torch.cuda.device(x.device):
        mm = _minmax(x)
        check(lib.d4w_scale_pixels_f32(dev.ptr(x), dev.out_ptr(y), _n(x), dev.ptr(mm), float(gain), dev.stream_ptr(x)))
    return y


def scale_pixels(img):
    """(img - img.min()) / (img.max() - img.min()) -- reference improcess.py:23-40."""
    x = dev.to_device_f32(img)
    return dev.like_input(_scale_pixels_device(x, 1.0), img)


def _trace2image_device(x):
    nx, ns = x.shape
    var = torch.empty(nx, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.d4w_row_var_f32(dev.ptr(x), nx, ns, dev.ptr(var), dev.stream_ptr(x)))
    env = dsp._analytic(x, 4, var=var)                      # |hilbert(x)| / std(x) per row
    return _scale_pixels_device(env, 255.0, out=env)


def trace2image(trace):
    """|hilbert(trace, axis=1)| / std(trace, axis=1), min-max scaled to [0, 255] -- reference
    improcess.py:43-62."""
    if getattr(trace, "ndim", 0) != 2:
        raise ValueError("trace must be a 2-D [channel x time] array")
    return dev.like_input(_trace2image_device(dev.to_device_f32(trace)), trace)


def angle_fromspeed(c0, fs, dx, selected_channels):
    """Angle (degrees) of a c0 m/s arrival in the [channel x time] pixel grid -- reference
    improcess.py:65-96 (prints the ratio and the angle like the reference)."""
    ratio = c0 / (fs * dx * selected_channels[2])
    print('Detection speed ratio: ', ratio)
    theta_c0 = np.arctan(ratio) * 180 / np.pi
    print('Angle: ', theta_c0)
    return theta_c0


def get_gabor_kernel(ksize, sigma, theta, lambd, gamma, psi=np.pi * 0.5):
    """cv2.getGaborKernel(ksize, sigma, theta, lambd, gamma, psi, ktype=CV_64F) evaluated on the host:
    exp(-(x'^2 / sigma^2 + gamma^2 y'^2 / sigma^2) / 2) cos(2 pi x' / lambd + psi) on the grid
    [-h//2, h//2] x [-w//2, w//2], stored mirrored in both axes as OpenCV does."""
    xmax, ymax = int(ksize[0]) // 2, int(ksize[1]) // 2
    c, s = np.cos(theta), np.sin(theta)
    yy, xx = np.meshgrid(np.arange(-ymax, ymax + 1, dtype=np.float64), np.arange(-xmax, xmax + 1, dtype=np.float64),
                         indexing="ij")
    xr, yr = xx * c + yy * s, yy * c - xx * s
    sx, sy = float(sigma), float(sigma) / float(gamma)
    g = np.exp(-0.5 * (xr * xr / (sx * sx) + yr * yr / (sy * sy))) * np.cos(2.0 * np.pi / lambd * xr + psi)
    return np.ascontiguousarray(g[::-1, ::-1])


def gabor_filt_design(theta_c0, plot=False):
    """The two 101 x 101 Gabor kernels oriented along +-theta_c0 -- reference improcess.py:99-140
    (ksize 100, sigma 4, lambda 20, gamma 0.15, psi 0).  `plot` is accepted and ignored."""
    up = get_gabor_kernel((100, 100), 4, np.pi / 2 + np.deg2rad(theta_c0), 20, 0.15, 0)
    return up, np.flipud(up)


def _filter2d_device(img, kernels):
    """sum_k filter2D(img, kernels[k]) on the device; img float32 CUDA [h, w]."""
    h, w = img.shape
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        for i, k in enumerate(kernels):
            kd = dev.to_device_f32(k, img.device)
            kh, kw = kd.shape
            ws = torch.empty(int(lib.d4w_filter2d_ws_bytes(kh, kw)), dtype=torch.uint8, device=img.device)
            check(lib.d4w_filter2d_f32(dev.ptr(img), h, w, dev.ptr(kd), kh, kw, dev.ptr(out), int(i > 0), dev.ptr(ws),
                                       dev.stream_ptr(img)))
    return out


def filter2d(img, kernel):
    """cv2.filter2D(img, cv2.CV_64F, kernel) (scripts/main_gabordetect.py:109,132): correlation with the
    anchor at the kernel centre and BORDER_REFLECT_101 borders.  A bool image is taken as 0 / 1."""
    if getattr(img, "ndim", 0) != 2 or getattr(kernel, "ndim", 0) != 2:
        raise ValueError("img and kernel must be 2-D")
    x = dev.to_device_f32(img)
    y = _filter2d_device(x, [kernel])
    if dev.is_tensor(img):
        return y
    return y.cpu().numpy().astype(np.float64)


def _resize_device(x, oh, ow):
    h, w = x.shape
    if oh < 1 or ow < 1:
        raise ValueError(f"binning: output size ({oh}, {ow}) is empty")
    y = torch.empty((oh, ow), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws = torch.empty(int(lib.d4w_resize_ws_bytes(h, w, oh, ow)), dtype=torch.uint8, device=x.device)
        check(lib.d4w_resize_bilinear_aa_f32(dev.ptr(x), h, w, dev.ptr(y), oh, ow, dev.ptr(ws), dev.stream_ptr(x)))
    return y


def _is_bool(a):
    return (dev.is_tensor(a) and a.dtype == torch.bool) or (not dev.is_tensor(a) and np.asarray(a).dtype == bool)


def binning(image, ft, fx):
    """transforms.Resize((int(H * fx), int(W * ft)))(ToTensor()(image)) -- reference
    improcess.py:395-420: antialiased bilinear interpolation (torchvision >= 0.17 default).  A bool
    image comes back as bool: True wherever a True pixel has non-zero weight (torchvision casts to
    float32, interpolates and casts back)."""
    if getattr(image, "ndim", 0) != 2:
        raise ValueError("image must be 2-D")
    oh, ow = int(image.shape[0] * fx), int(image.shape[1] * ft)
    if _is_bool(image):
        y = _resize_device(dev.to_device_f32(image), oh, ow) != 0
        return y if dev.is_tensor(image) else y.cpu().numpy()
    return dev.like_input(_resize_device(dev.to_device_f32(image), oh, ow), image)


def _mask_mul_device(x, m):
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(lib.d4w_mask_mul_f32(dev.ptr(x), dev.ptr(m), dev.ptr(y), _n(x), dev.stream_ptr(x)))
    return y


def apply_smooth_mask(array, mask, sigma=1.5):
    """array * mask -- reference improcess.py:423-454.  The reference also blurs the mask with a
    Gaussian (sigma) and normalises it, but multiplies by the RAW mask (:452); the unused blur is not
    computed here."""
    if tuple(array.shape) != tuple(mask.shape):
        raise ValueError(f"operands could not be broadcast together with shapes {tuple(array.shape)} {tuple(mask.shape)}")
    x = dev.to_device_f32(array)
    m = dev.to_device_f32(mask, x.device)
    return dev.like_input(_mask_mul_device(x, m), array)


def gabor_mask(trf_fk, fs, dx, selected_channels, c0=1500., threshold=9100., threshold2=150., bin_factor=10):
    """scripts/main_gabordetect.py:78-166 in one call, all intermediates on the device.

    Returns a dict: "image" (trace2image), "imagebin", "fimage" (Gabor line score), "mask" (bool, binned
    grid), "mask_sparse" (bool, full grid) and "masked_tr" (trf_fk * mask_sparse).  NumPy input gives
    NumPy outputs (float arrays in the input dtype), CUDA tensors give CUDA tensors."""
    if getattr(trf_fk, "ndim", 0) != 2:
        raise ValueError("trf_fk must be a 2-D [channel x time] array")
    x = dev.to_device_f32(trf_fk)
    nx, ns = x.shape
    image = _trace2image_device(x)
    ratio = c0 / (fs * dx * selected_channels[2])
    up, down = gabor_filt_design(np.arctan(ratio) * 180 / np.pi)
    bh, bw = int(nx * (1 / bin_factor)), int(ns * (1 / bin_factor))
    imagebin = _resize_device(image, bh, bw)
    both = up + down                                        # filter2D is linear in the kernel: one pass for the pair
    fimage = _filter2d_device(imagebin, [both])
    binary = torch.empty_like(fimage)
    with torch.cuda.device(x.device):
        check(lib.d4w_threshold_f32(dev.ptr(fimage), dev.ptr(binary), _n(fimage), float(threshold), dev.stream_ptr(x)))
        score = _filter2d_device(binary, [both])
        mask = torch.empty_like(score)
        check(lib.d4w_threshold_f32(dev.ptr(score), dev.ptr(mask), _n(score), float(threshold2), dev.stream_ptr(x)))
    uh, uw = int(bh * bin_factor), int(bw * bin_factor)
    if (uh, uw) != (nx, ns):
        raise ValueError(f"operands could not be broadcast together with shapes ({nx},{ns}) ({uh},{uw})")
    # binning() of a bool mask is bool (True wherever a True pixel has non-zero weight, improcess.py:416-420): the
    # interpolated weights are binarised before the multiplication (array * bool mask, improcess.py:452)
    mask_sparse = (_resize_device(mask, uh, uw) != 0)
    masked = _mask_mul_device(x, mask_sparse.to(torch.float32))
    res = {"image": image, "imagebin": imagebin, "fimage": fimage, "score": score, "mask": mask != 0,
           "mask_sparse": mask_sparse, "masked_tr": masked}
    if dev.is_tensor(trf_fk):
        return res
    out = {}
    for k, v in res.items():
        out[k] = v.cpu().numpy() if v.dtype == torch.bool else dev.like_input(v, trf_fk)
    return out


def _radon_input(image):
    """skimage's convert_to_float(image, preserve_range=False): float32 / float64 kept, other floats computed in float32,
    bool as 0 / 1, unsigned integers / max, signed integers (2 x + 1) / (max - min) (img_as_float).  Returns the float32
    CUDA tensor and the NumPy dtype of the result (None for tensors)."""
    if dev.is_tensor(image):
        x = image
        if x.dtype == torch.bool:
            x = x.to(torch.float32)
        elif not x.dtype.is_floating_point:
            if x.dtype.is_complex:
                raise TypeError("compute_radon_transform: complex images are not supported")
            info = torch.iinfo(x.dtype)
            x = x.to(torch.float64)
            x = x / float(info.max) if info.min == 0 else (2.0 * x + 1.0) / float(info.max - info.min)
        return dev.to_device_f32(x), None
    a = np.asarray(image)
    if a.dtype.kind == "f":
        return dev.upload_f32(a), a.dtype
    if a.dtype.kind == "b":
        return dev.upload_f32(a), np.dtype(np.float64)
    if a.dtype.kind == "u":
        return dev.upload_f32(a / float(np.iinfo(a.dtype).max)), np.dtype(np.float64)
    if a.dtype.kind == "i":
        info = np.iinfo(a.dtype)
        return dev.upload_f32((2.0 * a.astype(np.float64) + 1.0) / float(info.max - info.min)), np.dtype(np.float64)
    raise TypeError("compute_radon_transform: unsupported image dtype %s" % a.dtype)


def _radon_device(x, theta):
    """Sinogram [P, len(theta)] of the float32 CUDA image x; theta = float64 NumPy angles in degrees."""
    h, w = x.shape
    n = int(theta.size)
    P = lib.d4w_radon_size(h, w)
    if P < 0:
        check(P)
    out = torch.empty((P, n), dtype=torch.float32, device=x.device)
    if n == 0:
        return out
    with torch.cuda.device(x.device):
        ws = torch.empty(int(lib.d4w_radon_ws_bytes(h, w, n)), dtype=torch.uint8, device=x.device)
        check(lib.d4w_radon_f32(dev.ptr(x), h, w, theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n,
                                dev.out_ptr(out), dev.ptr(ws), dev.stream_ptr(x)))
    return out


def compute_radon_transform(image, theta=None):
    """Radon transform of a 2-D image -- reference improcess.py:347-367, skimage.transform.radon(image, theta,
    circle=False): the image zero-padded to P x P (P = ceil(sqrt(2) max(h, w)), centred as skimage pads it), each angle
    (degrees, default np.arange(180)) a bilinear rotation about P // 2 summed over rows.  Returns [P, len(theta)]: NumPy
    in the dtype skimage returns (float32 / float64 kept, integers and bool as float64), a CUDA tensor as float32."""
    if getattr(image, "ndim", np.ndim(image)) != 2:
        raise ValueError("The input image must be 2-D")
    th = np.arange(180, dtype=np.float64) if theta is None else theta
    if dev.is_tensor(th):
        th = th.detach().cpu().numpy()
    th = np.ascontiguousarray(th, dtype=np.float64)
    if th.ndim != 1:
        raise ValueError("theta must be a 1-D array of angles in degrees")
    x, dtype = _radon_input(image)
    y = _radon_device(x, th)
    if dev.is_tensor(image):
        return y if image.is_cuda else y.to(image.device)
    return dev.download(y, dtype)


_P_DOUBLE = ctypes.POINTER(ctypes.c_double)


def _require_2d(a, name):
    if getattr(a, "ndim", np.ndim(a)) != 2:
        raise ValueError("%s must be a 2-D array" % name)


def _stencil_device(x, kernel, anchor):
    """Correlation of the float32 CUDA image x with a float64 host kernel of at most 7 x 7, zeros outside the image."""
    h, w = x.shape
    k = np.ascontiguousarray(kernel, dtype=np.float64)
    out = torch.empty_like(x)
    if _n(x) == 0:
        return out
    with torch.cuda.device(x.device):
        check(lib.d4w_stencil_zero_f32(dev.ptr(x), h, w, k.ctypes.data_as(_P_DOUBLE), k.shape[0], k.shape[1], int(anchor[0]),
                                       int(anchor[1]), dev.out_ptr(out), dev.stream_ptr(x)))
    return out


def gradient_oriented(image, direction):
    """Three-point oriented difference -- reference improcess.py:143-169.  direction = (dft, dfx), non-negative integers:
    dfx == 0: -(image[:, :-dft] - image[:, dft:]) [h, w - dft]; dft == 0: -(image[dfx:] - image[:-dfx]) [h - dfx, w]; else
    -(image[dfx:-dfx, :-dft] - 0.5 image[2 dfx:, dft:] - 0.5 image[:-2 dfx, dft:]) [h - 2 dfx, w - dft].  (0, 0) gives the
    reference's empty [h, 0]; a shift that leaves no output gives the empty array of that shape."""
    _require_2d(image, "image")
    try:
        dft, dfx = (operator.index(d) for d in direction)
    except TypeError:
        raise ValueError("direction must be a pair of non-negative integers (dft, dfx)") from None
    if dft < 0 or dfx < 0:
        raise ValueError("direction must be a pair of non-negative integers (dft, dfx)")
    h, w = int(image.shape[0]), int(image.shape[1])
    oh = h if dfx == 0 else max(h - dfx, 0) if dft == 0 else max(h - 2 * dfx, 0)
    ow = max(w - dft, 0) if (dft or dfx) else 0
    if oh == 0 or ow == 0:                                  # nothing to compute: no upload, no launch
        if dev.is_tensor(image):
            return torch.empty((oh, ow), dtype=torch.float32, device=image.device)
        t = np.asarray(image).dtype
        return np.empty((oh, ow), dtype=t if t.kind == "f" else np.float64)
    x = dev.to_device_f32(image)
    out = torch.empty((oh, ow), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.d4w_gradient_oriented_f32(dev.ptr(x), h, w, dft, dfx, dev.out_ptr(out), dev.stream_ptr(x)))
    return dev.like_input(out, image)


# diagonal_filter + fliplr(diagonal_filter) of improcess.py:192-216: the two fftconvolve calls are linear in the kernel
_DIAG5 = np.array([[1, 2, 2, 2, 1], [0, 1, 2, 1, 0], [0, 0, 0, 0, 0], [0, -1, -2, -1, 0], [-1, -2, -2, -2, -1]], dtype=np.float64)
# weight_left + flip(weight_left, [0]) of improcess.py:251-255
_DIAG3 = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], dtype=np.float64)


def detect_diagonal_edges(matrix, threshold):
    """fftconvolve(matrix, D, 'same') + fftconvolve(matrix, fliplr(D), 'same') with the 5 x 5 diagonal kernel D -- reference
    improcess.py:172-226 -- as one zero-border stencil with the summed kernel (a convolution: the kernel is applied flipped
    in both axes).  `threshold` is accepted and unused, as in the reference.  NumPy input gives float64."""
    _require_2d(matrix, "matrix")
    y = _stencil_device(dev.to_device_f32(matrix), _DIAG5[::-1, ::-1], (2, 2))
    if dev.is_tensor(matrix):
        return y if matrix.is_cuda else y.to(matrix.device)
    return dev.download(y, np.float64)


def diagonal_edge_detection(img, threshold):
    """conv2d(img, W, padding=1) + conv2d(img, flipud(W), padding=1) with the 3 x 3 diagonal kernel W -- reference
    improcess.py:229-266 -- as one zero-border stencil with the summed kernel.  Like the reference it returns a CPU float32
    torch.Tensor [h, w] for array input; a CUDA tensor gives a CUDA tensor.  `threshold` is unused, as in the reference."""
    _require_2d(img, "img")
    y = _stencil_device(dev.to_device_f32(img), _DIAG3, (1, 1))
    if dev.is_tensor(img) and img.is_cuda:
        return y
    return y.cpu()


def get_gaussian_kernel(ksize, sigma):
    """cv2.getGaussianKernel(ksize, sigma) as OpenCV documents it, float64 [ksize]: exp(-(i - (ksize - 1) / 2)^2 / (2 sigma^2))
    normalised to sum 1; sigma <= 0 means sigma = 0.3 ((ksize - 1) 0.5 - 1) + 0.8, except the fixed tables of ksize 1, 3, 5, 7."""
    n = int(ksize)
    fixed = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    if sigma <= 0 and n in fixed:
        return np.array(fixed[n], dtype=np.float64)
    s = float(sigma) if sigma > 0 else 0.3 * ((n - 1) * 0.5 - 1.0) + 0.8
    i = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    t = np.exp(-(i * i) / (2.0 * s * s))
    return t / t.sum()


def _is_uint8(a):
    return a.dtype == (torch.uint8 if dev.is_tensor(a) else np.uint8)


def _smooth_output(y, img):
    """cv2's output depth is the input's: uint8 images are rounded half to even and saturated, floats keep their dtype."""
    if not dev.is_tensor(img):
        img = np.asarray(img)
    if _is_uint8(img):
        q = torch.round(y).clamp_(0.0, 255.0).to(torch.uint8)
        if dev.is_tensor(img):
            return q if img.is_cuda else q.to(img.device)
        return q.cpu().numpy()
    return dev.like_input(y, img)


def _gaussian_blur_device(x, taps_y, taps_x):
    h, w = x.shape
    out = torch.empty_like(x)
    if _n(x) == 0:
        return out
    ky, kx = int(taps_y.size), int(taps_x.size)
    with torch.cuda.device(x.device):
        nws = int(lib.d4w_gaussian_blur_ws_bytes(h, w, ky, kx))
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
        check(lib.d4w_gaussian_blur_f32(dev.ptr(x), h, w, taps_y.ctypes.data_as(_P_DOUBLE), taps_x.ctypes.data_as(_P_DOUBLE),
                                        ky, kx, dev.out_ptr(out), dev.ptr(ws) if nws else None, dev.stream_ptr(x)))
    return out


def gaussian_filter(img, size, sigma):
    """cv2.GaussianBlur(img, (size, size), sigma) -- reference improcess.py:370-392 -- by OpenCV's documented definition:
    separable correlation with get_gaussian_kernel(size, sigma) along both axes, BORDER_REFLECT_101.  `size` must be odd
    and positive.  float32 / float64 keep their dtype, uint8 comes back as uint8 (rounded half to even, saturated).
    Unpinned: cv2 is not installed, and real OpenCV filters uint8 images in fixed point."""
    _require_2d(img, "img")
    try:
        n = operator.index(size)
    except TypeError:
        raise ValueError("size must be an odd positive integer") from None
    if n < 1 or n % 2 == 0:
        raise ValueError("size must be an odd positive integer, got %d" % n)
    taps = get_gaussian_kernel(n, float(sigma))
    return _smooth_output(_gaussian_blur_device(dev.to_device_f32(img), taps, taps), img)


def bilateral_space_weights(radius, sigma_space):
    """exp(-(i^2 + j^2) / (2 sigma_space^2)) over the (2 radius + 1)^2 square, 0 outside the circle i^2 + j^2 <= radius^2."""
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    rr = i[:, None] ** 2 + i[None, :] ** 2
    return np.where(rr <= float(radius) ** 2, np.exp(-rr / (2.0 * float(sigma_space) ** 2)), 0.0)


def bilateral_radius(diameter, sigma_space):
    """diameter <= 0: max(round(1.5 sigma_space), 1) (sigma_space <= 0 counts as 1); else diameter // 2."""
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    return max(int(round(1.5 * ss)), 1) if diameter <= 0 else int(diameter) // 2


def bilateral_filter(img, diameter, sigma_color, sigma_space):
    """cv2.bilateralFilter(img, diameter, sigma_color, sigma_space) -- reference improcess.py:319-344 -- by OpenCV's
    documented definition: out(p) = sum_q w I(q) / sum_q w over the offsets q - p = (i, j) with i^2 + j^2 <= r^2,
    w = exp(-(i^2 + j^2) / (2 sigma_space^2) - (I(q) - I(p))^2 / (2 sigma_color^2)), BORDER_REFLECT_101; a sigma <= 0 counts
    as 1; r = diameter // 2, or max(round(1.5 sigma_space), 1) for diameter <= 0.  dtypes as gaussian_filter.
    Unpinned: cv2 is not installed, and real OpenCV reads the float range weight from an interpolated table."""
    _require_2d(img, "img")
    try:
        d = operator.index(diameter)
    except TypeError:
        raise ValueError("diameter must be an integer") from None
    sc = float(sigma_color) if sigma_color > 0 else 1.0
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    if not (np.isfinite(sc) and np.isfinite(ss)):
        raise ValueError("sigma_color and sigma_space must be finite")
    r = bilateral_radius(d, ss)
    x = dev.to_device_f32(img)
    h, w = x.shape
    out = torch.empty_like(x)
    if _n(x):
        with torch.cuda.device(x.device):
            sw = dev.to_device_f32(bilateral_space_weights(r, ss), x.device)
            check(lib.d4w_bilateral_f32(dev.ptr(x), h, w, r, dev.ptr(sw), sc, dev.out_ptr(out), dev.stream_ptr(x)))
    return _smooth_output(out, img)
