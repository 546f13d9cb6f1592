"""Mask morphology on the GPU: the exact Euclidean distance transform of binary images and what is a threshold on it.

``distance_transform`` is ``sc_edt`` (include/starcop_hip.h): int32 squared distances or float32 distances to the nearest set (or
unset) pixel.  ``dilate`` / ``erode`` by a disc of any radius are one ``sc_edt`` call each that stores only the thresholded
mask; ``opening`` / ``closing`` are their compositions.  ``remove_small_objects`` is the sieve: ``connected_components``, a device
bincount of the labels and one gather (``sc_label_keep``).

``nearest_index`` is ``sc_edt_nearest``, the feature transform: WHICH target is the nearest one, as the int32 raster index
``row * W + col``.  Among equally near targets the one with the smallest column wins, then the one with the smallest row (scipy's
``distance_transform_edt(return_indices=True)`` breaks ties by another, undocumented rule; the two agree wherever the nearest
target is unique).  ``expand_labels`` (skimage's, away from ties) and ``fill_nearest`` (the scipy idiom ``data[tuple(indices)]``)
are the same call gathering a label or value plane at that index.

Every function takes an (H, W) or (N, H, W) mask, numpy or a device tensor of any dtype; anything but uint8 / bool becomes
``x != 0``, uint8 device tensors are read in place through their strides (a band of an (H, W, 4) image, a ``[:, ::2]`` view).
numpy in, numpy out; device in, device out.  There is no CPU fallback.

Conventions.  The disc of radius r is {(dy, dx): dy^2 + dx^2 <= floor(r * r)}; r = 1 is the 3 x 3 cross (skimage's ``disk(1)``).
Dilation sees no pixels outside the image.  Erosion treats the outside as set (skimage's border convention): a pixel survives
when it is set and no UNSET pixel inside the image lies within r of it."""
import math

import numpy as np
import torch

from . import _lib, stacks
from ._lib import check, ptr, stream
from .mask_creation import connected_components

FAR = _lib.EDT_FAR
WINDOW_MAX_R = _lib.EDT_WINDOW_MAX_R
VARIANTS = {None: 0, "window": _lib.EDT_WINDOW, "envelope": _lib.EDT_ENVELOPE}
_D2_MAX = FAR - 1


def _check_mask(mask, who):
    stacks.check_stack(mask, who, "mask")
    H, W = mask.shape[-2:]
    if not (0 < H <= 32767 and 0 < W <= 32767) or mask.shape[0] == 0:
        raise ValueError(f"{who}: bad shape {tuple(mask.shape)} (H, W in 1..32767, no empty batch)")


def _cap(v, who, what):
    """floor(v * v) of a radius / distance in pixels, in float64 with no epsilon, kept inside the int32 range of d2"""
    v = float(v)
    if not v >= 0.0:
        raise ValueError(f"{who}: {what} {v!r} must be >= 0")
    sq = v * v
    return _D2_MAX if sq >= _D2_MAX else int(math.floor(sq))


def _edt(m3, invert, want, max_dist2=0, thresh2=0, negate=False, pixel_size=1.0, variant=0):
    """one ``sc_edt`` call on a device uint8 (N, H, W) view -> the output tensor ``want`` (``dist2``, ``dist`` or ``within``)"""
    lib = _lib.load()
    N, H, W = m3.shape
    dtype = {"dist2": torch.int32, "dist": torch.float32, "within": torch.uint8}[want]
    out = torch.empty((N, H, W), dtype=dtype, device=m3.device)
    a = _lib.sc_edt_args()
    a.mask, a.stride_n, a.stride_h, a.stride_w = m3.data_ptr(), m3.stride(0), m3.stride(1), m3.stride(2)
    a.N, a.H, a.W, a.invert = N, H, W, int(bool(invert))
    a.max_dist2, a.thresh2, a.variant, a.negate = int(max_dist2), int(thresh2), int(variant), int(bool(negate))
    a.pixel_size = float(pixel_size)
    setattr(a, want, out.data_ptr())
    wb = lib.sc_edt_call_workspace_bytes(a)                  # what this call's row pass needs; 0 where the call itself will refuse
    stacks.call_with_workspace(lib.sc_edt, a, wb, m3.device)
    return out


def edt_variant(H, W, max_dist2=0, forced=None):
    """host: which row pass ``sc_edt`` takes for an (H, W) image and a cap on the squared distance (0: none) -> ``"window"`` or
    ``"envelope"``; ``forced`` one of the two names.  ValueError where the library refuses (the window beyond its limit)."""
    if forced not in VARIANTS:
        raise ValueError(f"edt_variant: variant {forced!r}; expected one of None, 'window', 'envelope'")
    v = _lib.load().sc_edt_variant(int(H), int(W), int(max_dist2), VARIANTS[forced])
    check(v if v < 0 else 0)
    return "window" if v == _lib.EDT_WINDOW else "envelope"


def distance_transform(mask, to="set", max_distance=None, squared=False, pixel_size=1.0, variant=None):
    """Exact Euclidean distance of every pixel to the nearest set pixel (``to="set"``) or, scipy's ``distance_transform_edt(mask)``
    convention, to the nearest unset one (``to="unset"``): float32 ``sqrt(d2) * pixel_size`` rounded once from float64, or with
    ``squared=True`` the int32 squared distance in pixels.  An image without a target gives ``inf`` / ``INT32_MAX`` everywhere.
    ``max_distance`` (pixels) caps the result: pixels whose squared distance exceeds ``floor(max_distance * max_distance)`` are
    ``inf`` / ``INT32_MAX``, and a small cap takes the windowed row pass.  ``variant``: None for the library's rule, ``"window"`` or
    ``"envelope"`` to force a row pass (tests, benchmark)."""
    who = "distance_transform"
    _check_mask(mask, who)
    if to not in ("set", "unset"):
        raise ValueError(f"{who}: to={to!r}; expected 'set' or 'unset'")
    if variant not in VARIANTS:
        raise ValueError(f"{who}: variant {variant!r}; expected one of None, 'window', 'envelope'")
    if not float(pixel_size) > 0.0:
        raise ValueError(f"{who}: pixel_size {pixel_size!r} must be positive")
    cap = None if max_distance is None else _cap(max_distance, who, "max_distance")
    if cap == _D2_MAX:
        cap = None                                           # no distance in an image reaches it
    if variant == "window" and (cap is None or math.isqrt(cap) > WINDOW_MAX_R):
        raise ValueError(f"{who}: variant='window' needs a max_distance of at most {WINDOW_MAX_R} pixels")
    m3, single, host = stacks.device_mask(mask)
    invert = to == "unset"
    if cap == 0:                                             # only the targets themselves lie within the cap
        on = _edt(m3, invert, "within", thresh2=0, variant=VARIANTS[variant])
        out = torch.where(on != 0, 0, FAR).to(torch.int32) if squared else torch.where(on != 0, 0.0, math.inf).to(torch.float32)
        return stacks.finish(out, single, host)
    out = _edt(m3, invert, "dist2" if squared else "dist", max_dist2=cap or 0, pixel_size=pixel_size, variant=VARIANTS[variant])
    return stacks.finish(out, single, host)


def _nearest(m3, invert, max_dist2=0, variant=0, index=False, dist2=False, planes=()):
    """one ``sc_edt_nearest`` call on a device uint8 (N, H, W) view -> (index or None, dist2 or None, [gathered planes]);
    ``planes``: (N, H, W) device tensors of a 4-byte dtype, read in place where their H x W planes are dense"""
    lib = _lib.load()
    N, H, W = m3.shape
    a = _lib.sc_edt_nearest_args()
    a.mask, a.stride_n, a.stride_h, a.stride_w = m3.data_ptr(), m3.stride(0), m3.stride(1), m3.stride(2)
    a.N, a.H, a.W, a.invert = N, H, W, int(bool(invert))
    a.max_dist2, a.variant, a.n_planes = int(max_dist2), int(variant), len(planes)
    idx = torch.empty((N, H, W), dtype=torch.int32, device=m3.device) if index else None
    d2 = torch.empty((N, H, W), dtype=torch.int32, device=m3.device) if dist2 else None
    a.index, a.dist2 = (idx.data_ptr() if index else None), (d2.data_ptr() if dist2 else None)
    srcs, outs = [stacks.plane_operand(p) for p in planes], []      # holds the tensors the pointers belong to until the call is enqueued
    for i, (t, stride) in enumerate(srcs):
        outs.append(torch.empty((N, H, W), dtype=t.dtype, device=m3.device))
        a.src[i], a.src_stride[i], a.dst[i] = t.data_ptr(), stride, outs[i].data_ptr()
    wb = lib.sc_edt_nearest_call_workspace_bytes(a)          # 0 where the call itself will refuse
    stacks.call_with_workspace(lib.sc_edt_nearest, a, wb, m3.device)
    return idx, d2, outs


def _distance_cap(max_distance, who, what="max_distance"):
    """None (no cap) or floor(max_distance^2); a cap no distance in an image reaches is none"""
    cap = None if max_distance is None else _cap(max_distance, who, what)
    return None if cap == _D2_MAX else cap


def nearest_index(mask, to="set", max_distance=None, return_distance=False, variant=None):
    """The feature transform: for every pixel the int32 raster index ``row * W + col`` of the nearest set pixel (``to="set"``) or
    unset pixel (``to="unset"``) of its image; among equally near targets the smallest column, then the smallest row.  A target's
    index is its own.  -1 everywhere in an image without a target and, with ``max_distance`` (pixels), wherever the squared
    distance exceeds ``floor(max_distance * max_distance)``: a cap of 0 leaves the targets alone.  ``return_distance``: also the
    int32 squared distance (``INT32_MAX`` where the index is -1), bit-equal to ``distance_transform(..., squared=True)``.
    ``variant`` as in ``distance_transform``."""
    who = "nearest_index"
    _check_mask(mask, who)
    if to not in ("set", "unset"):
        raise ValueError(f"{who}: to={to!r}; expected 'set' or 'unset'")
    if variant not in VARIANTS:
        raise ValueError(f"{who}: variant {variant!r}; expected one of None, 'window', 'envelope'")
    cap = _distance_cap(max_distance, who)
    if variant == "window" and (cap is None or math.isqrt(cap) > WINDOW_MAX_R):
        raise ValueError(f"{who}: variant='window' needs a max_distance of at most {WINDOW_MAX_R} pixels")
    m3, single, host = stacks.device_mask(mask)
    invert = to == "unset"
    if cap == 0:                                             # only the targets themselves lie within the cap
        N, H, W = m3.shape
        on = (m3 != 0) != invert
        idx = torch.where(on, torch.arange(H * W, dtype=torch.int32, device=m3.device).view(1, H, W), -1).to(torch.int32)
        d2 = torch.where(on, 0, FAR).to(torch.int32)
    else:
        idx, d2, _ = _nearest(m3, invert, cap or 0, VARIANTS[variant], index=True, dist2=bool(return_distance))
    if return_distance:
        return stacks.finish(idx, single, host), stacks.finish(d2, single, host)
    return stacks.finish(idx, single, host)


def expand_labels(labels, distance=1.0):
    """skimage's ``expand_labels``: an integer label image, 0 the background -> int32, every background pixel within ``distance``
    pixels (squared distance <= ``floor(distance * distance)``) of a labelled one takes the label of its nearest labelled pixel,
    labelled pixels keep theirs.  Where two labels are equally near, the tie rule of ``nearest_index`` decides (skimage inherits
    scipy's; the results agree away from ties).  ``distance=0`` returns the labels as int32.  One ``sc_edt_nearest`` call."""
    who = "expand_labels"
    _check_mask(labels, who)
    t = _cap(distance, who, "distance")
    lab, single, host = stacks.device_labels(labels, who, "mask", integers=True)
    if t == 0:
        return stacks.finish(lab if host or labels.dtype != torch.int32 else lab.clone(), single, host)
    m3 = (lab != 0).to(torch.uint8)
    out = _nearest(m3, False, 0 if t == _D2_MAX else t, planes=[lab])[2][0]
    return stacks.finish(out, single, host)


MAX_FILL_PLANES = _lib.EDT_NEAREST_MAX_PLANES


def fill_nearest(data, invalid, max_distance=None):
    """Nearest-value fill of no-data pixels: ``data`` a float32 (H, W) / (N, H, W) plane, or a list of up to 8 such planes that
    share ``invalid``, a mask of that shape.  Every pixel with ``invalid != 0`` takes the value (the bits: NaN payloads survive) of
    the nearest pixel with ``invalid == 0`` of its image, by the tie rule of ``nearest_index``; valid pixels keep theirs, and so
    do invalid pixels farther than ``max_distance`` (pixels) or in an image without a valid pixel.  The mask is read in place
    (uint8 / bool device tensors through their strides), all planes are gathered in one ``sc_edt_nearest`` call.  A plane in, a
    plane out; a list in, a list out."""
    who = "fill_nearest"
    many = isinstance(data, (list, tuple))
    planes = list(data) if many else [data]
    if not 1 <= len(planes) <= MAX_FILL_PLANES:
        raise ValueError(f"{who}: {len(planes)} planes, 1 to {MAX_FILL_PLANES} per call")
    _check_mask(invalid, who)
    host = isinstance(invalid, np.ndarray)
    for i, p in enumerate(planes):
        if isinstance(p, np.ndarray) != host or not isinstance(p, (np.ndarray, torch.Tensor)):
            raise ValueError(f"{who}: plane {i} and the mask must both be numpy arrays or both tensors")
        if tuple(p.shape) != tuple(invalid.shape):
            raise ValueError(f"{who}: plane {i} has shape {tuple(p.shape)}, the mask {tuple(invalid.shape)}")
        if p.dtype not in (np.float32, torch.float32):
            raise ValueError(f"{who}: plane {i} must be float32, got {p.dtype}")
    cap = _distance_cap(max_distance, who)
    m3, single, _ = stacks.device_mask(invalid)
    if host:
        planes = [stacks.upload(p, m3.device) for p in planes]
    else:
        for p in planes:
            _lib.require_device(p)
    planes = [p[None] if single else p for p in planes]
    if cap == 0:
        outs = [p.clone() for p in planes]
    else:
        outs = _nearest(m3, True, cap or 0, planes=planes)[2]
    outs = [stacks.finish(o, single, host) for o in outs]
    return outs if many else outs[0]


def _binary(mask, single, host):
    return stacks.finish((mask != 0).to(torch.uint8), single, host)


def _disc_op(m3, t, erosion):
    """dilation or erosion of a device uint8 (N, H, W) view by the disc d2 <= t, one ``sc_edt`` call -> device uint8 0 / 1"""
    if t == 0:
        return (m3 != 0).to(torch.uint8)
    return _edt(m3, erosion, "within", thresh2=t, negate=erosion)


def _disc_ops(mask, radius, who, steps):
    """the arguments checked once, then ``steps`` (True: erosion, False: dilation) in order"""
    _check_mask(mask, who)
    t = _cap(radius, who, "radius")
    m3, single, host = stacks.device_mask(mask)
    for erosion in steps:
        m3 = _disc_op(m3, t, erosion)
    return stacks.finish(m3, single, host)


def dilate(mask, radius):
    """Binary dilation of ``mask != 0`` by the disc of ``radius`` pixels -> uint8 0 / 1.  Pixels outside the image are unset."""
    return _disc_ops(mask, radius, "dilate", (False,))


def erode(mask, radius):
    """Binary erosion of ``mask != 0`` by the disc of ``radius`` pixels -> uint8 0 / 1.  Pixels outside the image count as set."""
    return _disc_ops(mask, radius, "erode", (True,))


def opening(mask, radius):
    """``dilate(erode(mask, radius), radius)``: removes what the disc does not fit into"""
    return _disc_ops(mask, radius, "opening", (True, False))


def closing(mask, radius):
    """``erode(dilate(mask, radius), radius)``: fills what the disc does not fit into"""
    return _disc_ops(mask, radius, "closing", (False, True))


def remove_small_objects(mask, min_area, connectivity=2):
    """The sieve: the components of ``connected_components(mask, connectivity)`` with at least ``min_area`` pixels -> uint8 0 / 1.
    ``min_area <= 1`` returns the mask as 0 / 1 without labelling.  One read-back (the largest component count sizes the table)."""
    _check_mask(mask, "remove_small_objects")
    if connectivity not in (1, 2):
        raise ValueError(f"remove_small_objects: connectivity {connectivity!r} (1 or 2)")
    min_area = int(min_area)
    m3, single, host = stacks.device_mask(mask)
    if min_area <= 1:
        return _binary(m3, single, host)
    labels, counts = connected_components(m3, connectivity=connectivity)
    N, H, W = labels.shape
    M = max(int(counts.max().item()), 0)                     # the one read-back: sizes the table
    area = torch.stack([torch.bincount(labels[n].reshape(-1), minlength=M + 1) for n in range(N)])     # on the int32 labels as they are
    keep = (area >= min_area).to(torch.uint8)
    keep[:, 0] = 0
    out = torch.empty((N, H, W), dtype=torch.uint8, device=labels.device)
    check(_lib.load().sc_label_keep(ptr(labels), ptr(keep.contiguous()), ptr(out), N, M, H, W, stream()))
    return stacks.finish(out, single, host)
