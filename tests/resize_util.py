"""Anti-aliased resize: the scipy oracle (the operator's definition), the numpy tap-loop restatement of the kernel's rounding contract
and a seeded plane maker, shared by test_resize_host.py, test_gpu_resize.py and test_gpu_resample_pipeline.py."""
import warnings

import numpy as np
import scipy.ndimage as ndi

MODES = ("constant", "nearest", "reflect", "mirror")
ULP = 2.0 ** -24

# (H, W, oh, ow, sigma, cval): the smallest shapes at which the kernel can still go wrong
SHAPES = [
    (37, 53, 9, 13, 1.5, 0.0),
    (64, 40, 11, 7, 2.5, -9999.0),            # with a block of cval pixels
    (50, 50, 50, 25, 0.5, 3.0),               # one axis identity-sized but blurred
    (23, 31, 4, 5, 5.5, 0.0),
    (9, 5, 3, 2, 5.5, 0.0),                   # radius larger than twice the axis
    (1, 7, 1, 3, 1.5, 2.0),
    (6, 6, 1, 1, 2.5, 0.0),
    (40, 40, 13, 13, 0.0, 0.0),
    (256, 668, 21, 56, 5.5, 0.0),             # the flight line's width and the 60 m ratio
]


def make_plane(H, W, seed, cval=None):
    """seeded float32 plane in [0, 100); with ``cval`` a block of cval pixels in its upper-left corner"""
    x = (np.random.default_rng(seed).random((H, W)) * 100).astype(np.float32)
    if cval is not None:
        x[:max(1, H // 8), :max(1, W // 6)] = cval
    return x


def sigma_pair(sigma):
    return (float(sigma), float(sigma)) if np.ndim(sigma) == 0 else (float(sigma[0]), float(sigma[1]))


def oracle64(x, output_shape, sigma, mode, cval):
    """the operator: scipy's Gaussian then scipy's bilinear zoom (grid_mode), evaluated in float64"""
    x = np.asarray(x, dtype=np.float64)
    sy, sx = sigma_pair(sigma)
    f = ndi.gaussian_filter(x, (sy, sx), mode=mode, cval=float(cval)) if (sy > 0 or sx > 0) else x
    with warnings.catch_warnings():
        # scipy recommends grid-constant with grid_mode; with o <= n no source coordinate leaves [0, n - 1], the two are the same here
        warnings.simplefilter("ignore", UserWarning)
        y = ndi.zoom(f, (output_shape[0] / x.shape[0], output_shape[1] / x.shape[1]), order=1, mode=mode, cval=float(cval),
                     grid_mode=True)
    assert y.shape == tuple(output_shape), (y.shape, output_shape)
    return y


def apply_axis0(x, start, w, wc, cval):
    """the rounding contract along axis 0 of a float32 (n, m) array: float64 products added in ascending tap order onto +0.0, the
    cval term last, one rounding to float32"""
    x = np.asarray(x, dtype=np.float32)
    acc = np.zeros((w.shape[0], x.shape[1]), np.float64)
    for k in range(w.shape[1]):
        acc = acc + w[:, k, None] * x[start + k].astype(np.float64)
    acc = acc + (wc * np.float64(np.float32(cval)))[:, None]
    return acc.astype(np.float32)


def restatement(x, output_shape, sigma, mode, cval):
    """what the kernel computes, bit for bit: the vertical pass, rounded to float32, then the horizontal pass"""
    from starcop_amd import resample
    H, W = x.shape
    sy, sx = sigma_pair(sigma)
    t = apply_axis0(x, *resample.axis_taps(H, output_shape[0], sy, mode), cval)
    return np.ascontiguousarray(apply_axis0(t.T, *resample.axis_taps(W, output_shape[1], sx, mode), cval).T)


def gate(x, cval):
    """4 * 2^-24 * M: twice the derived bound of two float32 roundings of values that never exceed M = max(max|x|, |cval|)"""
    return 4.0 * ULP * max(float(np.abs(x).max()), abs(float(cval)))


def ulps(got, want, x, cval):
    """worst distance in units of 2^-24 * M"""
    return float(np.abs(got.astype(np.float64) - want).max()) / (ULP * max(float(np.abs(x).max()), abs(float(cval))))
