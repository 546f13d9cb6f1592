"""Sentinel-2 cloud / cloud-shadow detector: mirror of ``starcop/sentinel2/models.py``.

The reference's ``CDModel`` is ``smp.Unet("mobilenet_v2", encoder_weights=None, in_channels=13, classes=4)`` followed by
``torch.argmax(dim=1).type(torch.uint8)`` (models.py:63-78), run over a whole image through ``padded_predict(tensor, model, 32)``
(models.py:27-52, 80-89).  Here the network is :class:`starcop_amd.network.HyperStarcopUNet` (13, 4) on libstarcop_hip.so: the
13-band stem (``sc_stem_conv_fwd``), the shared 61 convolutions, and a head that writes the class index itself
(``sc_head_conv_fwd_k`` with the fused argmax) -- the (N, 4, H, W) logits never reach memory.  Inference only.

``predict`` is the reference's procedure: the whole reflect-padded image as one batch element.  ``predict_scene`` is the mode for a
whole 10 980 x 10 980 tile, whose activations do not fit that way: the (virtual) padded scene is walked in equally shaped windows
(:func:`starcop_amd.scene.scene_windows`, re-exported here), ``sc_scene_gather`` cuts and converts a batch of them straight from the uint16 / float32 scene, and the head
writes the class index of every window's core into the (H, W) result (``sc_head_conv_fwd_k_mosaic``).

No checkpoint is shipped: the reference's sits in a private bucket (``load_weights`` reads a local copy).
"""
import os

import numpy as np
import torch

from . import _lib
from .network import HyperStarcopUNet
from .padding import find_padding, padded_predict       # same arithmetic as models.py:20-25 / 27-52; pad and crop on the device
from .scene import (RECEPTIVE_HALO, SCENE_BATCH_PIXELS, SCENE_TILE, ScenePlan, float_bits, scene_core_counts,  # noqa: F401  (the window
                    scene_gather, scene_gather_planes, scene_table, scene_windows, window_batches)             # plan lives in scene.py)

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
        table = scene_table(plan)
        table_dev = torch.from_numpy(table).to(src.device)
        mosaic = torch.empty((H, W), dtype=torch.uint8, device=src.device)
        for first, k, buf in window_batches(table.shape[0], plan.window, self.NUM_BANDS, src.device, batch):
            x = scene_gather(src, (plan.pad_rows[0], plan.pad_cols[0]), table_dev, table, first, k, plan.window, scale, out=buf)
            self.model.predict_classes_into(x, mosaic, (table_dev, table, first))
        return mosaic.cpu().numpy() if is_np else mosaic


def cloud_mask_file(src_tif, dst_tif, model, cog=False, **kw):
    """13-band GeoTIFF -> uint8 cloud-mask GeoTIFF (``model.predict_scene(bands, **kw)``): 128 x 128 blocks, the source's
    georeferencing tags, band description "cloudmask" and the class names in the GDAL metadata.  Returns the (H, W) mask.
    ``cog=True`` (or a dict of ``cog.write_cog`` keyword arguments) keeps the mask on the device and writes it as a
    Cloud-Optimized GeoTIFF -- tiles and mode-resampled overviews made on the device, all-zero tiles left out; the default
    leaves every byte of the file as it was."""
    from . import io_formats, products
    info = io_formats.tiff_info(src_tif)
    bands = io_formats.read_tiff(src_tif, info=info)
    if cog and bands.dtype == np.uint16:                      # the COG is made from the device mask: the bands go there first
        bands = torch.from_numpy(bands.view(np.int16)).to(model.device).view(torch.uint16)
    elif cog:
        bands = torch.from_numpy(bands).to(model.device)
    mask = model.predict_scene(bands, **kw)
    tags = {t: v for t, v in info.geo_tags().items() if t not in (42112, 42113)}       # (the source's metadata / nodata describe its bands)
    tags.update(io_formats.gdal_metadata_tag({f"class_{i}": name for i, name in enumerate(INTERPRETATION_CLOUDSEN12)}, ["cloudmask"]))
    products.write_raster(dst_tif, mask, tags, cog)
    return mask.cpu().numpy() if cog else mask
