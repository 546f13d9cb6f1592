"""Sentinel-2 cloud / cloud-shadow detector: mirror of ``starcop/sentinel2/models.py``.

The reference's ``CDModel`` is ``smp.Unet("mobilenet_v2", encoder_weights=None, in_channels=13, classes=4)`` followed by
``torch.argmax(dim=1).type(torch.uint8)`` (models.py:63-78), run over a whole image through ``padded_predict(tensor, model, 32)``
(models.py:27-52, 80-89).  Here the network is :class:`starcop_amd.network.HyperStarcopUNet` (13, 4) on libstarcop_hip.so: the
13-band stem (``sc_stem_conv_fwd``), the shared 61 convolutions, and a head that writes the class index itself
(``sc_head_conv_fwd_k`` with the fused argmax) -- the (N, 4, H, W) logits never reach memory.  Inference only.

No checkpoint is shipped: the reference's sits in a private bucket (``load_weights`` reads a local copy).
"""
import os

import numpy as np
import torch

from .network import HyperStarcopUNet
from .padding import find_padding, padded_predict       # same arithmetic as models.py:20-25 / 27-52; pad and crop on the device

__all__ = ["INTERPRETATION_CLOUDSEN12", "load_weights", "find_padding", "padded_predict", "CDModel"]

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

    ``predict`` runs the whole (reflect-padded) image as ONE batch element: there is no tiled whole-scene mode, so a full
    10 980 x 10 980 Sentinel-2 tile is out of scope (its activations do not fit); cut such a scene into windows first.
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
