"""Anti-aliased downscaling on the GPU: the ``read.resize(..., anti_aliasing=True, anti_aliasing_sigma=sigma_bands)`` that ends the
reference's ``transform_to_srf`` (starcop/data/aviris.py:333-338).  georeader's ``read.resize`` wraps
``skimage.transform.resize(order=1, anti_aliasing=True)``, which since skimage 0.19 is, per 2-D plane,

    f = scipy.ndimage.gaussian_filter(x, (sigma_y, sigma_x), mode=m, cval=c)      # truncate 4.0: radius int(4 sigma + 0.5)
    y = scipy.ndimage.zoom(f, (oh / H, ow / W), order=1, mode=m, cval=c, grid_mode=True)
    # source coordinate of output j: (j + 0.5) * n / o - 0.5

That pair is separable and linear in ``(x, cval)``: per axis, output ``j`` is ``sum_k w[j][k] * x[start[j] + k] + wc[j] * cval``.
:func:`axis_taps` builds those tables on the host in float64; ``sc_resize_aa`` (include/starcop_hip.h) applies them, the vertical axis
first, with one rounding to float32 per axis.  Downscaling only: with ``o <= n`` every bilinear source coordinate lies in
``[0, n - 1]``, so the border mode matters to the Gaussian alone.
"""
import functools

import numpy as np
import torch

from . import _lib
from ._lib import check, stream

MODES = ("constant", "nearest", "reflect", "mirror")      # scipy.ndimage's names


def gaussian_kernel(sigma):
    """scipy.ndimage's 1-D Gaussian at truncate 4.0: ``exp(-0.5 / sigma^2 * t^2)`` over ``t = -r..r``, ``r = int(4 sigma + 0.5)``,
    normalised by its sum; sigma 0 is the identity.  -> (weights float64 [2 r + 1], r)"""
    sigma = float(sigma)
    if sigma == 0.0:
        return np.ones(1, np.float64), 0
    r = int(4.0 * sigma + 0.5)
    t = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 / (sigma * sigma) * t ** 2)
    return g / g.sum(), r


def _fold(i, n, mode):
    """sample index that scipy's border ``mode`` reads for the (possibly outside) index ``i``; -1 = the constant ``cval``"""
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    if mode == "reflect":                     # d c b a | a b c d | d c b a
        m = np.mod(i, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    if mode == "mirror":                      # d c b | a b c d | c b a
        if n == 1:
            return np.zeros_like(i)
        m = np.mod(i, 2 * n - 2)
        return np.where(m < n, m, 2 * n - 2 - m)
    return np.where((i >= 0) & (i < n), i, -1)


def _check(n, o, sigma, mode):
    if mode not in MODES:
        raise ValueError(f"border mode '{mode}': expected one of {MODES}")
    if n < 1 or o < 1:
        raise ValueError(f"axis of {n} samples resized to {o}")
    if o > n:
        raise ValueError(f"output axis of {o} samples is larger than the input's {n}: downscaling only")
    if not sigma >= 0.0:
        raise ValueError(f"anti-aliasing sigma {sigma}: expected >= 0")


@functools.lru_cache(maxsize=64)
def _axis_taps(n, o, sigma, mode):
    g, r = gaussian_kernel(sigma)
    c = (np.arange(o, dtype=np.float64) + 0.5) * (n / o) - 0.5              # in [0, n - 1] since o <= n
    i0 = np.floor(c).astype(np.int64)
    t = c - i0
    k = np.arange(-r, r + 1, dtype=np.int64)
    # the two samples of the lerp, each spread by the Gaussian: (o, 2, 2 r + 1) source indices and weights
    idx = (np.stack([i0, i0 + 1], axis=1))[:, :, None] + k[None, None, :]
    val = np.stack([1.0 - t, t], axis=1)[:, :, None] * g[None, None, :]
    idx = _fold(idx, n, mode).reshape(o, -1)
    val = val.reshape(o, -1)
    used = val != 0.0                                                           # t == 0: the second sample (i0 + 1 may be n) has no weight
    inside = used & (idx >= 0)
    first = np.where(inside, idx, n).min(axis=1)
    last = np.where(inside, idx, -1).max(axis=1)
    first = np.where(last < 0, 0, first)                                        # every tap outside: all the weight goes to cval
    T = max(1, int((last - first).max()) + 1)
    start = np.minimum(first, n - T).astype(np.int32)
    rows = np.broadcast_to(np.arange(o)[:, None], idx.shape)
    w = np.zeros((o, T), np.float64)
    np.add.at(w, (rows[inside], (idx - start[:, None])[inside]), val[inside])
    wc = np.zeros(o, np.float64)
    np.add.at(wc, rows[used & (idx < 0)], val[used & (idx < 0)])
    for a in (start, w, wc):
        a.setflags(write=False)
    return start, w, wc


def axis_taps(n, o, sigma, mode="constant"):
    """Tap table of one axis of ``n`` samples resized to ``o <= n``: ``(start int32 [o], w float64 [o, T], wc float64 [o])`` with
    output ``j = sum_k w[j, k] * x[start[j] + k] + wc[j] * cval``.  The window ``[start[j], start[j] + T)`` lies inside ``[0, n)``;
    ``T <= min(n, 2 r + 2)``; rows with fewer taps are zero-padded; ``wc`` is zero unless ``mode`` is "constant".  The arrays are
    cached and read-only."""
    n, o, sigma = int(n), int(o), float(sigma)
    _check(n, o, sigma, mode)
    return _axis_taps(n, o, sigma, mode)


def default_sigma(n, o):
    """skimage's default anti-aliasing sigma of an axis: ``max(0, (n / o - 1) / 2)``"""
    return max(0.0, (n / o - 1.0) / 2.0)


def output_shape_for(shape, resolution_src, resolution_dst):
    """(oh, ow) of a raster of ``shape[-2:]`` pixels of size ``resolution_src`` resampled to pixels of ``resolution_dst`` (each a number
    or ``(y, x)``): ``max(1, int(np.round(n * res_src / res_dst)))`` per axis"""
    src = _pair(resolution_src)
    dst = _pair(resolution_dst)
    return tuple(max(1, int(np.round(int(n) * s / d))) for n, s, d in zip(tuple(shape)[-2:], src, dst))


def _pair(v):
    if np.ndim(v) == 0:
        return (abs(float(v)),) * 2
    if len(v) != 2:
        raise ValueError(f"resolution {v}: expected a number or (y, x)")
    return (abs(float(v[0])), abs(float(v[1])))


def _sigmas(sigma, P, shape, output_shape):
    """-> float64 (P, 2): (sigma_y, sigma_x) of every plane"""
    if sigma is None:
        s = np.tile([default_sigma(n, o) for n, o in zip(shape, output_shape)], (P, 1))
    else:
        s = np.asarray(sigma, dtype=np.float64)
        if s.ndim == 0:
            s = np.full((P, 2), float(s))
        elif s.shape == (P,):
            s = np.repeat(s[:, None], 2, axis=1)
        elif s.shape != (P, 2):
            raise ValueError(f"sigma of shape {s.shape}: expected a scalar, ({P},) or ({P}, 2)")
    if not np.all(s >= 0.0):
        raise ValueError("anti-aliasing sigma must be >= 0")
    return s


class _Axis:
    """the tables of one axis for the planes of a call: equal sigmas share a table; rows padded to the widest table's T"""

    def __init__(self, n, o, sigmas, mode):
        uniq, inverse = np.unique(sigmas, return_inverse=True)
        tabs = [axis_taps(n, o, s, mode) for s in uniq]
        self.n, self.o, self.n_tables = int(n), int(o), len(tabs)
        self.T = max(w.shape[1] for _, w, _ in tabs)
        self.start = np.stack([s for s, _, _ in tabs]).astype(np.int32)
        self.taps = np.array([w.shape[1] for _, w, _ in tabs], np.int32)
        self.w = np.zeros((self.n_tables, self.o, self.T), np.float64)
        for i, (_, w, _) in enumerate(tabs):
            self.w[i, :, :w.shape[1]] = w
        self.wc = np.stack([c for _, _, c in tabs])
        self.table = np.ascontiguousarray(inverse.reshape(-1), dtype=np.int32)
        self.dev = None

    def upload(self, device):
        if self.dev is None:
            self.dev = [torch.from_numpy(np.ascontiguousarray(a)).to(device)
                        for a in (self.start, self.taps, self.w, self.wc, self.table)]
        return self

    def fill(self, ax):
        ax.n, ax.o, ax.n_tables, ax.T = self.n, self.o, self.n_tables, self.T
        ax.start, ax.taps, ax.w, ax.wc = (t.data_ptr() for t in self.dev[:4])
        ax.start_host, ax.taps_host = self.start.ctypes.data, self.taps.ctypes.data


@functools.lru_cache(maxsize=16)
def _axis_on_device(n, o, sigmas, mode, device):
    """the packed tables of an axis, uploaded once per (axis, sigmas of the planes, mode, device): a flight line is resampled with the
    same few tables call after call"""
    return _Axis(n, o, np.array(sigmas, dtype=np.float64), mode).upload(device)


def resize_antialiased(x, output_shape, sigma=None, mode="constant", cval=0.0, out=None):
    """Gaussian anti-aliasing followed by a bilinear downscale of every plane of ``x`` to ``output_shape = (oh, ow)``: scipy's
    ``zoom(gaussian_filter(x, sigma, mode, cval), order=1, mode, cval, grid_mode=True)`` (the module docstring has the operator).

    ``x``: (P, H, W) or (H, W) float32 device tensor with any strides (a permuted view is read in place), or a numpy array (numpy in,
    numpy out).  ``sigma``: None (skimage's default ``max(0, (n / o - 1) / 2)`` per axis), a scalar, (P,) or (P, 2) as (sigma_y,
    sigma_x); planes with equal sigma share a tap table.  ``mode``: "constant" (with ``cval``), "nearest", "reflect" or "mirror".
    ``out``: optional (P, oh, ow) float32 device view with dense samples, e.g. a line range of a larger buffer.
    ValueError for a larger output, a negative sigma or an unknown mode."""
    host = isinstance(x, np.ndarray)
    flat = x.ndim == 2
    if x.ndim not in (2, 3):
        raise ValueError(f"resize_antialiased: expected (P, H, W) or (H, W), got {tuple(x.shape)}")
    P = 1 if flat else int(x.shape[0])
    H, W = (int(v) for v in x.shape[-2:])
    if len(output_shape) != 2:
        raise ValueError(f"resize_antialiased: output_shape {output_shape}: expected (oh, ow)")
    oh, ow = (int(v) for v in output_shape)
    if P < 1:
        raise ValueError("resize_antialiased: no planes")
    sig = _sigmas(sigma, P, (H, W), (oh, ow))
    for n, o in ((H, oh), (W, ow)):
        _check(n, o, 0.0, mode)

    lib = _lib.load()
    if host:
        if x.dtype != np.float32:
            raise ValueError(f"resize_antialiased: float32 expected, got {x.dtype}")
        _lib.require_device()
        x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise ValueError(f"resize_antialiased: float32 expected, got {x.dtype}")
    x3 = x[None] if flat else x
    if out is None:
        out3 = torch.empty((P, oh, ow), dtype=torch.float32, device=x.device)
    else:
        _lib.require_device(out)
        out3 = out[None] if out.dim() == 2 else out
        if out3.dtype != torch.float32 or tuple(out3.shape) != (P, oh, ow):
            raise ValueError(f"resize_antialiased: out of shape {tuple(out.shape)} / {out.dtype}, expected float32 {(P, oh, ow)}")
        if ow > 1 and out3.stride(2) != 1:
            raise ValueError("resize_antialiased: output samples must be dense")
    ay = _axis_on_device(H, oh, tuple(sig[:, 0].tolist()), mode, x.device)
    ax = _axis_on_device(W, ow, tuple(sig[:, 1].tolist()), mode, x.device)
    work = torch.empty(lib.sc_resize_workspace_bytes(P, oh, W) // 4, dtype=torch.float32, device=x.device)
    a = _lib.sc_resize_args()
    a.x = x3.data_ptr()
    a.plane_stride, a.line_stride, a.sample_stride = x3.stride()
    a.P, a.cval = P, float(cval)
    a.out = out3.data_ptr()
    a.out_plane_stride, a.out_line_stride = out3.stride(0), out3.stride(1)
    ay.fill(a.y)
    ax.fill(a.xs)
    a.table_y, a.table_x = ay.dev[4].data_ptr(), ax.dev[4].data_ptr()
    a.table_y_host, a.table_x_host = ay.table.ctypes.data, ax.table.ctypes.data
    a.work, a.work_bytes = work.data_ptr(), work.numel() * 4
    check(lib.sc_resize_aa(a, stream()))
    if out is not None:
        return out
    res = out3[0] if flat else out3
    return res.cpu().numpy() if host else res
