"""The image-stack front-end of the mask and label-image operators (``mask_creation``, ``morphology``, ``plumes``): how an (H, W) or
(N, H, W) mask, label image or value plane, numpy or device, reaches the argument structures of include/starcop_hip.h as a device
(N, H, W) tensor, and how the columns a call leaves on the device come back to the host.  The sibling of ``planes.py``, which serves
the (P, H, W) rasters of the raster operators.  Every check here raises before ``require_device`` is called, so a caller that
checks its own arguments first refuses every bad argument without a device.  Depends on ``_lib`` and ``planes`` alone."""
import numpy as np
import torch

from . import _lib, planes
from ._lib import check, ptr, stream


def check_stack(x, who, what="array"):
    """the shape check: ``x`` must be an (H, W) or (N, H, W) numpy array or tensor -> whether it is (H, W)"""
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{who}: expected a numpy array or a tensor, got {type(x).__name__}")
    n = x.ndim
    if n != 2 and n != 3:
        raise ValueError(f"{who}: expected an (H, W) or (N, H, W) {what}, got {tuple(x.shape)}")
    return n == 2


def stack3(x, who, what="array"):
    """``check_stack`` -> ``(x3, single)``: the (N, H, W) view (making one costs about a microsecond: a caller that only checks asks
    ``check_stack``) and whether ``x`` was (H, W)"""
    single = check_stack(x, who, what)
    return (x[None] if single else x), single


def stack_like(x, shape, who):
    """an operand of a ``component_*`` call -- ``who`` names call and operand, ``"component_stats: plane 0"`` -- as (N, H, W): a tensor
    of the ``shape`` of the labels it rides with, or of its last two dimensions"""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{who} must be a device tensor, got {type(x).__name__} (plume_table takes numpy masks)")
    x3 = stack3(x, who)[0]
    if x3.shape != shape:
        raise ValueError(f"{who} has shape {tuple(x3.shape)}, labels {tuple(shape)}")
    return x3


def upload(a, device=None):
    """a numpy array -> a device tensor of its dtype, after ``require_device``; a tensor is returned as it is"""
    if isinstance(a, np.ndarray):
        _lib.require_device()
        return torch.from_numpy(np.ascontiguousarray(a)).to(device if device is not None else "cuda")
    return a


def device_mask(mask):
    """the mask front-end: -> ((N, H, W) device uint8 view -- in place for uint8 / bool device tensors, ``x != 0`` of anything else --,
    was (H, W), was numpy)"""
    host = isinstance(mask, np.ndarray)
    if host:
        m = upload(mask if mask.dtype == np.uint8 else (mask != 0).astype(np.uint8))
    else:
        _lib.require_device(mask)
        m = mask
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)
        elif m.dtype != torch.uint8:
            m = (m != 0).to(torch.uint8)
    single = m.dim() == 2
    return (m[None] if single else m), single, host


def device_labels(labels, who, what="label image", integers=False):
    """the label front-end: an (H, W) or (N, H, W) label image, numpy or tensor -> (device int32 contiguous (N, H, W), was (H, W), was
    numpy).  ``integers``: a floating-point or complex image is a ValueError (without it, it is truncated as ``.to(int32)`` does)."""
    lab, single = stack3(labels, who, what)
    host = isinstance(lab, np.ndarray)
    if integers and ((lab.dtype.kind not in "iub") if host else (lab.dtype.is_floating_point or lab.dtype.is_complex)):
        raise ValueError(f"{who}: labels must be integers, got {lab.dtype}")
    return labels_i32(upload(np.ascontiguousarray(lab, dtype=np.int32)) if host else lab), single, host


def labels_i32(lab):
    """the device half of the label front-end, for a caller that has checked the shape itself: a label tensor -> int32, contiguous,
    on the device (``require_device`` refuses one that is not)"""
    _lib.require_device(lab)
    if lab.dtype != torch.int32:
        lab = lab.to(torch.int32)
    return lab.contiguous()


def counts_i32(counts, N, device, who):
    """the counts front-end: an int (one image) or an (N,) array or tensor -> int32 (N,) on ``device`` (None: where it is, for a caller
    that only wants the length checked).  The length is checked on the counts as given, before anything is moved."""
    if isinstance(counts, int):
        c = torch.tensor([counts], dtype=torch.int32)
    else:
        c = (counts if isinstance(counts, torch.Tensor) else torch.as_tensor(counts)).reshape(-1)
    if c.numel() != N:
        raise ValueError(f"{who}: {c.numel()} counts for {N} images")
    return c.to(device=device, dtype=torch.int32).contiguous()


def plane_operand(t, dtype=None):
    """an (N, H, W) tensor as a kernel reads it -> (tensor, elements between images): a view whose H x W planes are dense at one
    non-overlapping stride (e.g. channel 3 of an (N, 4, H, W) tensor) is used in place, anything else is copied.  ``dtype``: what
    the kernel reads; another dtype is converted first, to uint8 as ``t != 0``."""
    if dtype is not None and t.dtype != dtype:
        t = (t != 0).to(dtype) if dtype == torch.uint8 else t.to(dtype)
    B, H, W = t.shape
    dense = (W == 1 or t.stride(2) == 1) and (H == 1 or t.stride(1) == W) and (B == 1 or t.stride(0) >= H * W)
    if not dense:
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else H * W)


def finish(out, single, host):
    """a device (N, H, W) result as the caller gave the input: (H, W) for an (H, W) input, numpy for numpy"""
    out = out[0] if single else out
    return out.cpu().numpy() if host else out


def output_columns(a, spec, device):
    """the output columns of a call: ``spec`` an iterable of (field, dtype, shape) -> {field: uninitialised device tensor}, with each
    pointer -- NULL for a column without elements -- stored in the field of that name of the argument structure ``a``"""
    out = {}
    for f, dtype, shape in spec:
        out[f] = t = torch.empty(shape, dtype=dtype, device=device)
        setattr(a, f, t.data_ptr() if t.numel() else None)
    return out


def call_with_workspace(fn, a, work_bytes, device):
    """``fn(a, work, work_bytes, stream)`` with ``work_bytes`` of scratch memory on ``device``.  A size of 0 is what the size
    functions answer for arguments the call refuses: the call is made all the same and raises with the library's message."""
    work = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=device)
    check(fn(a, ptr(work), work_bytes, stream()))


def read_back(columns):
    """{key: device tensor} -> {key: numpy array of the same dtype and shape} in ONE device-to-host copy: the columns travel as
    their bytes in one flat buffer, whatever their dtypes (1-, 2-, 4- and 8-byte integers and floats) and shapes, columns without
    elements included.  Every array owns its memory, so it is aligned and C-contiguous wherever its bytes lay in the buffer."""
    if not columns:
        return {}
    parts = [t.contiguous().reshape(-1).view(torch.uint8) for t in columns.values()]
    flat = torch.cat(parts).cpu().numpy()
    out, at = {}, 0
    for (key, t), p in zip(columns.items(), parts):
        n = p.numel()
        out[key] = flat[at:at + n].copy().view(planes.numpy_dtype(t.dtype, "read_back")).reshape(tuple(t.shape))
        at += n
    return out
