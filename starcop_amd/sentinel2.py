"""Sentinel-2 cloud / cloud-shadow detector: mirror of ``starcop/sentinel2/models.py``.

The reference's ``CDModel`` is ``smp.Unet("mobilenet_v2", encoder_weights=None, in_channels=13, classes=4)`` followed by
``torch.argmax(dim=1).type(torch.uint8)`` (models.py:63-78), run over a whole image through ``padded_predict(tensor, model, 32)``
(models.py:27-52, 80-89).  Here the network is :class:`starcop_amd.network.HyperStarcopUNet` (13, 4) on libstarcop_hip.so: the
13-band stem (``sc_stem_conv_fwd``), the shared 61 convolutions, and a head that writes the class index itself
(``sc_head_conv_fwd_k`` with the fused argmax) -- the (N, 4, H, W) logits never reach memory.  Inference only.

``predict`` is the reference's procedure: the whole reflect-padded image as one batch element.  ``predict_scene`` is the mode for a
whole 10 980 x 10 980 tile, whose activations do not fit that way: the (virtual) padded scene is walked in equally shaped windows
(:func:`scene_windows`), ``sc_scene_gather`` cuts and converts a batch of them straight from the uint16 / float32 scene, and the head
writes the class index of every window's core into the (H, W) result (``sc_head_conv_fwd_k_mosaic``).

No checkpoint is shipped: the reference's sits in a private bucket (``load_weights`` reads a local copy).
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .network import HyperStarcopUNet
from .padding import find_padding, padded_predict       # same arithmetic as models.py:20-25 / 27-52; pad and crop on the device
from .pipeline import RECEPTIVE_HALO

__all__ = ["INTERPRETATION_CLOUDSEN12", "load_weights", "find_padding", "padded_predict", "CDModel", "RECEPTIVE_HALO", "SCENE_TILE",
           "ScenePlan", "scene_windows", "scene_table", "scene_gather", "scene_gather_planes", "scene_core_counts", "float_bits",
           "cloud_mask_file"]

INTERPRETATION_CLOUDSEN12 = ["clear", "Thick cloud", "Thin cloud", "Cloud shadow"]      # models.py:11


def load_weights(path, map_location=None):
    """``torch.load`` of a local checkpoint file (models.py:13-18 opens ``path`` on Google Cloud Storage)."""
    if str(path).startswith("gs://"):
        raise NotImplementedError(f"{path}: reading from Google Cloud Storage is not supported; pass a local copy")
    if not os.path.exists(path):
        raise ValueError(f"Pretrained weights file: {path} does not exists")
    with open(path, "rb") as fh:
        return torch.load(fh, map_location=map_location)


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


def scene_gather(src, pads, table_dev, table_host, first, n, window, scale=1.0, out=None):
    """``sc_scene_gather``: windows [first, first + n) of the table out of the device scene ``src`` ((C, H, W), uint16 bits or float32,
    any non-negative strides) -> (n, C, wh, ww) float32.  ``pads`` = (pad_top, pad_left) of the virtual reflect-padded scene."""
    _lib.require_device(src)
    if src.dim() != 3 or src.element_size() not in (2, 4) or (src.element_size() == 4 and src.dtype != torch.float32):
        raise TypeError(f"scene_gather: expected a (C, H, W) uint16 or float32 tensor, got {tuple(src.shape)} {src.dtype}")
    wh, ww = window
    if (table_dev.dtype != torch.int32 or not table_dev.is_contiguous() or table_host.dtype != np.int32 or not table_host.flags.c_contiguous
            or table_dev.dim() != 2 or tuple(table_dev.shape) != tuple(table_host.shape) or table_dev.shape[1] != 8
            or first < 0 or n < 1 or first + n > table_dev.shape[0]):
        raise ValueError("scene_gather: the table must be a device int32 (m, 8) tensor and the same numpy int32 array, first + n <= m")
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
    a.win = table_dev.data_ptr() + 32 * first
    a.win_host = table_host.ctypes.data + 32 * first
    a.out = out.data_ptr()
    _lib.check(_lib.load().sc_scene_gather(C.byref(a), _lib.stream()))
    return out


def _check_table(who, table_dev, table_host, first, n):
    if (table_dev.dtype != torch.int32 or not table_dev.is_contiguous() or table_host.dtype != np.int32 or not table_host.flags.c_contiguous
            or table_dev.dim() != 2 or tuple(table_dev.shape) != tuple(table_host.shape) or table_dev.shape[1] != 8
            or first < 0 or n < 1 or first + n > table_dev.shape[0]):
        raise ValueError(f"{who}: the table must be a device int32 (m, 8) tensor and the same numpy int32 array, first + n <= m")


def float_bits(value):
    """bit pattern of ``float32(value)``: how the plume-scene kernels compare a fill value"""
    return int(np.array(value, dtype=np.float32).view(np.uint32))


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
    _check_table("scene_gather_planes", table_dev, table_host, first, n)
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
    for i, p in enumerate(planes):
        a.src[i] = p.data_ptr()
        a.row_stride[i], a.col_stride[i] = p.stride()
        fill, scale, clip = (seq[i] if seq is not None else None for seq in (fills, scales, clips))
        ops = 0
        if fill is not None:
            ops |= _lib.WCUT_FILL
            a.fill_bits[i] = float_bits(fill)
        if scale is not None:
            ops |= _lib.WCUT_SCALE
            a.scale[i] = float(np.float32(scale))
        if clip is not None:
            ops |= _lib.WCUT_CLIP
            a.clip_lo[i], a.clip_hi[i] = float(clip[0]), float(clip[1])
        a.ops[i] = ops
    a.win = table_dev.data_ptr() + 32 * first
    a.win_host = table_host.ctypes.data + 32 * first
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
    _check_table("scene_core_counts", table_dev, table_host, 0, n)
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=plane.device)
    _lib.check(_lib.load().sc_scene_core_counts(plane.data_ptr(), plane.stride(0), plane.stride(1), plane.shape[0], plane.shape[1],
                                                float_bits(fill), table_dev.data_ptr(), table_host.ctypes.data, n, out.data_ptr(),
                                                _lib.stream()))
    return out


class CDModel(torch.nn.Module):
    """
    Example:
        model = CDModel()
        weights = load_weights("CDmodel.ckpt", map_location="cpu")      # a local copy of the reference's checkpoint
        model.load_state_dict(weights["state_dict"])
        classes = model.predict(bands)                                  # (13, H, W) -> (H, W) uint8

    ``state_dict`` keys are the reference's (``model.encoder...``, ``model.decoder...``, ``model.segmentation_head.0...``,
    the BatchNorm ``num_batches_tracked`` entries included).

    ``predict`` runs the whole (reflect-padded) image as ONE batch element, as the reference does; a full 10 980 x 10 980
    Sentinel-2 tile goes through ``predict_scene`` (sliding windows with a receptive-field halo, uint16 or float32 input).
    """

    NUM_BANDS, NUM_CLASSES = 13, 4

    def __init__(self, device=torch.device("cuda")):
        super().__init__()
        self.model = HyperStarcopUNet(in_channels=self.NUM_BANDS, classes=self.NUM_CLASSES)
        self.device = torch.device(device)
        self.model.eval()
        self.model.to(self.device)

    def forward(self, tensor: torch.Tensor) -> torch.Tensor:
        """(N, 13, H, W), H and W multiples of 32 -> (N, H, W) uint8 class indices"""
        return self.model.predict_classes(tensor)

    def predict(self, tensor: np.ndarray) -> np.ndarray:
        """
            tensor: np.array (13, H, W)

        Returns:
            uint8 np.array (H, W) with interpretation {0: clear, 1: Thick cloud, 2: thin cloud, 3: cloud shadow}
        """
        assert tensor.shape[0] == 13, f"Expected 13 channels found {tensor.shape[0]}"

        return padded_predict(np.asarray(tensor, dtype=np.float32), self, 32, self.device)

    @torch.no_grad()
    def predict_scene(self, bands, tile=SCENE_TILE, halo=RECEPTIVE_HALO, batch=None, scale=1.0):
        """
            bands: (13, H, W) uint16 or float32, numpy array or device tensor, any (non-negative) strides
            scale: the network sees ``float32(bands) * float32(scale)`` (1.0: no multiply)

        Sliding-window form of ``predict`` for scenes whose activations do not fit as one image: the windows of
        ``scene_windows(H, W, tile, halo)`` are cut out of the virtual reflect-padded scene and converted to float32 by
        ``sc_scene_gather`` in batches of ``batch`` (default: the most windows with batch x window pixels <= 16 x 512^2), run through
        the network, and the head writes the class index of each window's core straight into the (H, W) result.  The scene stays in
        its own dtype on the device; no padded copy, no logits, no per-window class tensors.  With ``halo`` >= RECEPTIVE_HALO the
        logits behind every class equal the whole-scene forward's.

        Returns:
            uint8 (H, W): a numpy array for a numpy input, a device tensor for a device tensor
        """
        is_np = not isinstance(bands, torch.Tensor)
        if len(bands.shape) != 3:
            raise AssertionError(f"Expected 3D tensor, found {len(bands.shape)}D tensor")
        assert bands.shape[0] == 13, f"Expected 13 channels found {bands.shape[0]}"
        kind = {np.dtype(np.uint16): "u2", np.dtype(np.float32): "f4"}.get(bands.dtype) if is_np else \
            {torch.uint16: "u2", torch.float32: "f4"}.get(bands.dtype)
        if kind is None:
            raise TypeError(f"CDModel.predict_scene: bands must be uint16 or float32, got {bands.dtype}")
        _, H, W = (int(v) for v in bands.shape)
        plan = scene_windows(H, W, tile, halo)
        if self.device.type != "cuda":
            raise _lib.StarcopHipError(f"CDModel.predict_scene runs on a gfx950 GPU only; this model is on {self.device}")
        if is_np:
            if any(st < 0 for st in bands.strides):
                bands = np.ascontiguousarray(bands)
            host = bands.view(np.int16) if kind == "u2" else bands        # (the bits travel; torch.from_numpy has no uint16 everywhere)
            src = torch.from_numpy(host).to(self.device)
        else:
            _lib.require_device(bands)
            src = bands.view(torch.int16) if kind == "u2" else bands
        wh, ww = plan.window
        n = plan.offsets.shape[0]
        if batch is None:
            batch = max(1, SCENE_BATCH_PIXELS // (wh * ww))
        batch = max(1, min(int(batch), n))
        table = scene_table(plan)
        table_dev = torch.from_numpy(table).to(src.device)
        mosaic = torch.empty((H, W), dtype=torch.uint8, device=src.device)
        bufs = {}
        for first in range(0, n, batch):
            k = min(batch, n - first)
            if k not in bufs:
                bufs[k] = torch.empty((k, self.NUM_BANDS, wh, ww), dtype=torch.float32, device=src.device)
            x = scene_gather(src, (plan.pad_rows[0], plan.pad_cols[0]), table_dev, table, first, k, plan.window, scale, out=bufs[k])
            self.model.predict_classes_into(x, mosaic, (table_dev, table, first))
        return mosaic.cpu().numpy() if is_np else mosaic


def cloud_mask_file(src_tif, dst_tif, model, **kw):
    """13-band GeoTIFF -> uint8 cloud-mask GeoTIFF (``model.predict_scene(bands, **kw)``): 128 x 128 blocks, the source's
    georeferencing tags, band description "cloudmask" and the class names in the GDAL metadata.  Returns the (H, W) mask."""
    from . import io_formats
    info = io_formats.tiff_info(src_tif)
    bands = io_formats.read_tiff(src_tif, info=info)
    mask = model.predict_scene(bands, **kw)
    tags = {t: v for t, v in info.geo_tags().items() if t not in (42112, 42113)}       # (the source's metadata / nodata describe its bands)
    tags.update(io_formats.gdal_metadata_tag({f"class_{i}": name for i, name in enumerate(INTERPRETATION_CLOUDSEN12)}, ["cloudmask"]))
    io_formats.write_tiff(dst_tif, mask, blocksize=128, extra_tags=tags)
    return mask
