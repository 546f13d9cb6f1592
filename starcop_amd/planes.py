"""The plane front-end of the raster operators (``ortho``, ``warp``, ``mosaic``, ``window_dataset``, ``scene``): what a call's
``data`` may be and how its planes, fill values and per-plane operations reach the argument structures of include/starcop_hip.h.
Host only, and nothing here touches a device: every refusal comes before the caller's first device call, and a numpy input is
uploaded by the caller after its own checks.  Depends on ``_lib`` alone."""
import functools

import numpy as np
import torch

from . import _lib

EXPECTED = "a tensor (H, W) or (P, H, W), a numpy array or a list of 2-D tensors"


@functools.lru_cache(maxsize=None)
def _numpy_of(dt):
    """numpy's dtype of a torch dtype, None where numpy has none; asked of torch once per dtype, since every call of an operator asks"""
    try:
        return torch.empty(0, dtype=dt).numpy().dtype
    except TypeError:
        return None


def numpy_dtype(dt, who):
    """numpy's dtype of the torch dtype ``dt``; ValueError unless it is a 1-, 2-, 4- or 8-byte integer or float"""
    nd = _numpy_of(dt)
    if nd is None or nd.kind not in "fiu" or nd.itemsize not in (1, 2, 4, 8):
        raise ValueError(f"{who}: dtype {dt} is not supported (1-, 2-, 4- or 8-byte integers and floats)")
    return nd


def fill_bits(value, nd, who):
    """Bit pattern of ``value`` as numpy stores it in dtype ``nd`` (what ``np.full(shape, value, dtype)`` holds), for a fill
    that is WRITTEN: the pixels that get it must read back as the value the caller named, so a value the dtype cannot hold
    (a fraction, NaN or an out-of-range number for an integer dtype) is a ValueError.  Floats hold what numpy's conversion gives.
    :func:`match_bits` is the lenient counterpart for a fill that is only compared."""
    if nd.kind in "iu":
        f = float(value)
        info = np.iinfo(nd)
        if f != f or f != int(f) or not info.min <= int(f) <= info.max:
            raise ValueError(f"{who}: fill value {value!r} cannot be represented in {nd}")
        a = np.array(int(f), dtype=nd)
    else:
        a = np.asarray(value).astype(nd) if isinstance(value, (np.generic, np.ndarray)) else np.array(value, dtype=nd)
    return int(a.reshape(1).view(f"u{nd.itemsize}")[0])


def match_bits(value, nd):
    """Bit pattern of ``value`` in dtype ``nd`` for a fill that is only COMPARED with the elements of a plane, or None when no
    element can equal it: a value the dtype cannot hold exactly, and NaN, which equals nothing.  Nothing is written, so such a
    value is no error -- it simply never matches.  Wherever this answers, :func:`fill_bits`, the strict form, gives the same bits."""
    f = float(value)
    if nd.kind in "iu":
        info = np.iinfo(nd)
        if f != f or f != int(f) or not info.min <= int(f) <= info.max:
            return None
        a = np.array(int(f), dtype=nd)
    else:
        if f != f:
            return None
        a = np.array(f, dtype=nd)
        if float(a) != f:
            return None
    return int(a.reshape(1).view(f"u{nd.itemsize}")[0])


def as_planes(data, who, expected=EXPECTED, bad_type=ValueError, same_shape=True):
    """``data`` -- a tensor (H, W) or (P, H, W), a list of 2-D tensors or a numpy array -- -> ``(planes, single, host)``: the 2-D
    planes as views (nothing is copied; a permuted pixel-interleaved cube stays strided), whether the input was 2-D, and whether
    it was numpy.  The planes of a numpy array are CPU tensors over its memory (over a contiguous copy when it has a negative
    stride): the caller uploads them once its own checks are through.  The planes share one dtype and device and have no negative
    stride; ``same_shape=False`` leaves their shapes to the caller.  ``bad_type``: what anything else than these forms raises."""
    host = isinstance(data, np.ndarray)
    if host:
        data = torch.from_numpy(data if all(s >= 0 for s in data.strides) else np.ascontiguousarray(data))
    single = False
    if isinstance(data, (list, tuple)):
        planes = [torch.as_tensor(p) for p in data]
        if not planes or any(p.dim() != 2 for p in planes):
            raise ValueError(f"{who}: a list must hold at least one 2-D tensor")
    elif not isinstance(data, torch.Tensor):
        raise bad_type(f"{who}: expected {expected}, got {type(data).__name__}")
    elif data.dim() == 2:
        planes, single = [data], True
    elif data.dim() == 3 and data.shape[0] >= 1:
        planes = list(data.unbind(0))
    else:
        raise ValueError(f"{who}: expected {expected}, got {tuple(data.shape)}")
    dt, dev, shape = planes[0].dtype, planes[0].device, planes[0].shape
    if any(p.dtype != dt or p.device != dev or (same_shape and p.shape != shape) for p in planes):
        raise ValueError(f"{who}: all planes of a call share one dtype" + (", device and shape" if same_shape else " and device"))
    if any(s < 0 for p in planes for s in p.stride()):
        raise ValueError(f"{who}: negative strides are not supported")
    return planes, single, host


def per_plane(value, P, who, what, default=None):
    """a scalar (None: ``default``) or one value per plane -> a list of P values"""
    if isinstance(value, (list, tuple, np.ndarray)) and np.ndim(value) == 1:
        if len(value) != P:
            raise ValueError(f"{who}: {len(value)} {what} for {P} planes")
        return list(value)
    return [default if value is None else value] * P


def chunks(P, limit):
    """[(first plane, number of planes)] of the launches that take P planes ``limit`` at a time; P = 0 is one launch of none"""
    return [(p0, min(limit, P - p0)) for p0 in range(0, max(P, 1), limit)]


def set_planes(a, planes, k0=0, rows=None, cols=None):
    """Pointer and strides of ``planes[k0:]``, as many as the structure ``a`` takes, into ``a.src``, ``a.row_stride`` and
    ``a.col_stride`` -> their number.  ``rows`` / ``cols``: the arrays of ``a`` that take each plane's extent, where it has them."""
    n = min(len(a.src), len(planes) - k0)
    for k in range(n):
        t = planes[k0 + k]
        a.src[k] = t.data_ptr()
        a.row_stride[k], a.col_stride[k] = t.stride()
        if rows is not None:
            rows[k], cols[k] = t.shape
    return n


def set_plane_ops(a, k, bits, scale, clip):
    """The ``ops`` word of plane ``k`` of ``sc_wcut_args`` / ``sc_scene_planes_args`` and what goes with it; each may be None:
    ``bits`` -- elements with this pattern read as 0, ``scale`` -- one float32 multiply, ``clip`` -- then (lo, hi).  The float
    fields round a Python float to float32 as ``np.float32`` does (to nearest, ties to even, overflow to infinity)."""
    ops = 0
    if bits is not None:
        ops |= _lib.WCUT_FILL
        a.fill_bits[k] = bits
    if scale is not None:
        ops |= _lib.WCUT_SCALE
        a.scale[k] = float(scale)
    if clip is not None:
        ops |= _lib.WCUT_CLIP
        a.clip_lo[k], a.clip_hi[k] = float(clip[0]), float(clip[1])
    a.ops[k] = ops
