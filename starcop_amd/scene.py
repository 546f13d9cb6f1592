"""Scene windows: the plan behind ``CDModel.predict_scene`` (Sentinel-2 tiles) and ``ModelModule.predict_scene`` (AVIRIS-NG lines).

The (virtual) reflect-padded scene is walked in equally shaped windows (:func:`scene_windows`); the plan travels as the int32 rows
of ``sc_scene_win`` (:func:`scene_table`), on the device for the kernels and on the host for the argument checks of the entry
points.  :func:`table_rows` is the one check of such a pair, :func:`window_batches` the batch loop of both models.  Depends on
``_lib``, ``padding`` and ``planes`` only: ``network``, ``model_module``, ``pipeline`` and ``sentinel2`` import this module.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from .padding import find_padding
from .planes import set_plane_ops, set_planes

# Receptive field of smp.Unet('mobilenet_v2'): encoder 3x3 convolutions at strides 1..32 reach 490 px, the decoder
# adds 126 -> a logit depends on inputs at most 308 px away.  Halo >= 320 (a multiple of 32, the network's stride) therefore makes a
# tile's core logits IDENTICAL to the whole-scene forward in eval mode (BatchNorm is affine there); smaller halos are an approximation.
RECEPTIVE_HALO = 320
ScenePlan = collections.namedtuple("ScenePlan", "pad_rows pad_cols padded window offsets cores dests")
SCENE_BATCH_PIXELS = 16 * 512 * 512         # default batch of predict_scene: the most windows whose pixels stay below this
SCENE_TILE = 2048                           # default core size: the faster of 1024 / 2048 on a 10 980^2 tile (profiles/cdmodel_scene.txt)


def _axis_windows(n, pad, P, w, tile, halo):
    """one axis of :func:`scene_windows`: [(window offset, core start, core end)] with the core in padded coordinates"""
    if P <= w:
        return [(0, pad, pad + n)]
    out = []
    for t0 in range(0, P, tile):
        lo, hi = max(t0, pad), min(t0 + tile, P, pad + n)
        out.append((min(max(t0 - halo, 0), P - w), lo, max(lo, hi)))
    return out


def scene_windows(H, W, tile=SCENE_TILE, halo=RECEPTIVE_HALO):
    """The window plan of an (H, W) scene: ``pad_rows`` / ``pad_cols`` = ``find_padding(H, 32)`` / ``find_padding(W, 32)`` as ``predict``
    pads, ``padded`` = (Hp, Wp), ONE ``window`` shape (min(Hp, tile + 2 halo), min(Wp, tile + 2 halo)) and, per window, (n, 2) / (n, 4) /
    (n, 2) int32 arrays: ``offsets`` (row, column of the window in the padded scene), ``cores`` (y0, y1, x0, x1 inside the window) and
    ``dests`` (row, column of the core in the (H, W) image).  Cores are the ``tile`` x ``tile`` partition of the padded scene
    intersected with the image (ragged at the far border; y1 <= y0 or x1 <= x0 where a tile holds padding only).  At the padded
    scene's border a window is shifted inward, not clipped (``pipeline.scene_tiles`` clips), and everything is a multiple of 32, so
    one network plan serves every batch and a core pixel is at least ``halo`` away from every window side that is not a border of
    the padded scene -- with ``halo`` >= RECEPTIVE_HALO the eval-mode logits of a core equal the whole-scene forward's.  An axis along
    which the padded scene is no longer than a window has one window."""
    H, W, tile, halo = int(H), int(W), int(tile), int(halo)
    if tile <= 0 or tile % 32 or halo < 0 or halo % 32:
        raise ValueError(f"scene_windows: tile={tile} must be a positive and halo={halo} a non-negative multiple of 32")
    if H < 1 or W < 1:
        raise ValueError(f"scene_windows: bad scene size {H} x {W}")
    pr, pc = find_padding(H, 32), find_padding(W, 32)
    if max(pr) >= H or max(pc) >= W:
        raise ValueError("scene_windows: reflect padding needs the image to be larger than the pad")
    Hp, Wp = H + sum(pr), W + sum(pc)
    wh, ww = min(Hp, tile + 2 * halo), min(Wp, tile + 2 * halo)
    rows, cols = _axis_windows(H, pr[0], Hp, wh, tile, halo), _axis_windows(W, pc[0], Wp, ww, tile, halo)
    off = [(r, c) for r, _, _ in rows for c, _, _ in cols]
    cores = [(y0 - r, y1 - r, x0 - c, x1 - c) for r, y0, y1 in rows for c, x0, x1 in cols]
    dests = [(y0 - pr[0], x0 - pc[0]) for _, y0, _ in rows for _, x0, _ in cols]
    return ScenePlan(pr, pc, (Hp, Wp), (wh, ww), np.asarray(off, np.int32).reshape(-1, 2), np.asarray(cores, np.int32).reshape(-1, 4),
                     np.asarray(dests, np.int32).reshape(-1, 2))


def scene_table(plan):
    """the plan as the (n, 8) int32 rows of ``sc_scene_win``: row_off, col_off, core y0, y1, x0, x1, dst_row, dst_col"""
    return np.ascontiguousarray(np.concatenate([plan.offsets, plan.cores, plan.dests], axis=1), dtype=np.int32)


def table_rows(who, table_dev, table_host, first, n):
    """The check of a window table every entry point relies on -- a contiguous device int32 (m, 8) tensor, the same contiguous int32
    numpy array on the host, rows [first, first + n) inside it -- and -> (device pointer, host pointer) of row ``first``."""
    if (table_dev.dtype != torch.int32 or not table_dev.is_contiguous() or table_host.dtype != np.int32 or not table_host.flags.c_contiguous
            or table_dev.dim() != 2 or tuple(table_dev.shape) != tuple(table_host.shape) or table_dev.shape[1] != 8
            or first < 0 or n < 1 or first + n > table_dev.shape[0]):
        raise ValueError(f"{who}: the table must be a device int32 (m, 8) tensor and the same numpy int32 array, first + n <= m")
    off = C.sizeof(_lib.sc_scene_win) * int(first)
    return table_dev.data_ptr() + off, table_host.ctypes.data + off


def window_batches(n, window, channels, device, batch=None):
    """The batch loop of ``predict_scene``: yields (first, k, buffer) for the windows [first, first + k) of n, ``batch`` at a time (default:
    the most with batch x window pixels <= SCENE_BATCH_PIXELS; clamped to [1, n]); ``buffer``: float32 (k, channels, wh, ww), one per k."""
    wh, ww = window
    if batch is None:
        batch = max(1, SCENE_BATCH_PIXELS // (wh * ww))
    batch = max(1, min(int(batch), n))
    bufs = {}
    for first in range(0, n, batch):
        k = min(batch, n - first)
        if k not in bufs:
            bufs[k] = torch.empty((k, channels, wh, ww), dtype=torch.float32, device=device)
        yield first, k, bufs[k]


def float_bits(value):
    """bit pattern of ``float32(value)``: how the plume-scene kernels compare a fill value.  Beside ``planes.match_bits``, not over it:
    the scenes' fill may be NaN, which matches the elements that hold this very pattern"""
    return int(np.array(value, dtype=np.float32).view(np.uint32))


def scene_gather(src, pads, table_dev, table_host, first, n, window, scale=1.0, out=None):
    """``sc_scene_gather``: windows [first, first + n) of the table out of the device scene ``src`` ((C, H, W), uint16 bits or float32,
    any non-negative strides) -> (n, C, wh, ww) float32.  ``pads`` = (pad_top, pad_left) of the virtual reflect-padded scene."""
    _lib.require_device(src)
    if src.dim() != 3 or src.element_size() not in (2, 4) or (src.element_size() == 4 and src.dtype != torch.float32):
        raise TypeError(f"scene_gather: expected a (C, H, W) uint16 or float32 tensor, got {tuple(src.shape)} {src.dtype}")
    wh, ww = window
    win, win_host = table_rows("scene_gather", table_dev, table_host, first, n)
    if out is None:
        out = torch.empty((n, src.shape[0], wh, ww), dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n * src.shape[0] * wh * ww or out.device != src.device:
        raise ValueError("scene_gather: out must be a dense float32 (n, C, wh, ww) tensor on the scene's device")
    a = _lib.sc_scene_args()
    a.src, a.elem_bytes = src.data_ptr(), src.element_size()
    a.C, a.H, a.W = src.shape
    a.chan_stride, a.row_stride, a.col_stride = src.stride()
    a.pad_top, a.pad_left = int(pads[0]), int(pads[1])
    a.n, a.win_h, a.win_w, a.scale = int(n), int(wh), int(ww), float(scale)
    a.win, a.win_host = win, win_host
    a.out = out.data_ptr()
    _lib.check(_lib.load().sc_scene_gather(C.byref(a), _lib.stream()))
    return out


def scene_gather_planes(planes, pads, table_dev, table_host, first, n, window, fills=None, scales=None, clips=None, out=None):
    """``sc_scene_gather_planes``: windows [first, first + n) of the table out of P <= 16 float32 device planes of one (H, W) shape,
    each read in place through its own pointer and non-negative strides -> (n, P, wh, ww) float32.  Per plane (entries may be
    None): ``fills`` -- elements with the bits of float32(fill) become 0; ``scales`` -- else one float32 multiply by float32(scale);
    ``clips`` -- then (lo, hi) as ``numpy.clip``: the order of ``window_dataset.window_cut``."""
    P = len(planes)
    if not 1 <= P <= _lib.SCENE_MAX_PLANES:
        raise ValueError(f"scene_gather_planes: {P} planes (1 .. {_lib.SCENE_MAX_PLANES} expected)")
    H, W = (int(v) for v in planes[0].shape[-2:])
    for p in planes:
        if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.dtype != torch.float32 or tuple(p.shape) != (H, W):
            raise TypeError("scene_gather_planes: every plane must be an (H, W) float32 tensor of one shape")
        _lib.require_device(p)
    win, win_host = table_rows("scene_gather_planes", table_dev, table_host, first, n)
    wh, ww = window
    dev = planes[0].device
    if out is None:
        out = torch.empty((n, P, wh, ww), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n * P * wh * ww or out.device != dev:
        raise ValueError("scene_gather_planes: out must be a dense float32 (n, P, wh, ww) tensor on the planes' device")
    a = _lib.sc_scene_planes_args()
    a.P, a.H, a.W = P, H, W
    a.pad_top, a.pad_left = int(pads[0]), int(pads[1])
    a.n, a.win_h, a.win_w = int(n), int(wh), int(ww)
    set_planes(a, planes)
    for i in range(P):
        fill, scale, clip = (seq[i] if seq is not None else None for seq in (fills, scales, clips))
        set_plane_ops(a, i, float_bits(fill) if fill is not None else None, scale, clip)
    a.win, a.win_host = win, win_host
    a.out = out.data_ptr()
    _lib.check(_lib.load().sc_scene_gather_planes(C.byref(a), _lib.stream()))
    return out


def scene_core_counts(plane, fill, table_dev, table_host, out=None):
    """``sc_scene_core_counts``: for every row of the table the number of pixels in the window's core destination rectangle of the
    (H, W) float32 device ``plane`` whose bits differ from float32(fill) -> int32 (n,) device tensor (no synchronisation)."""
    if not isinstance(plane, torch.Tensor) or plane.dim() != 2 or plane.dtype != torch.float32:
        raise TypeError("scene_core_counts: plane must be an (H, W) float32 tensor")
    _lib.require_device(plane)
    n = int(table_host.shape[0])
    win, win_host = table_rows("scene_core_counts", table_dev, table_host, 0, n)
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=plane.device)
    _lib.check(_lib.load().sc_scene_core_counts(plane.data_ptr(), plane.stride(0), plane.stride(1), plane.shape[0], plane.shape[1],
                                                float_bits(fill), win, win_host, n, out.data_ptr(), _lib.stream()))
    return out
