"""The EMIT evaluation set as a data module: the loaders ``run_validation`` is fed with for EMIT scenes.

Mirrors /root/reference/starcop/emit_tools:
  ``load_emit_dataset`` / ``load_data``   emit_data_utils.py:6-78 (scene folders under ``plume_events`` and ``confounders``, the
                                          ``*_RGB`` / ``*_magic`` ENVI files read with ``io_formats.open_envi``, the label with
                                          ``read_tiff``; a scene without a label gets zeros)
  ``STARCOPEMITDataset``                  emit_dataset.py:11-117 (crop to multiples of 32, EMIT -> AVIRIS value range, label / 255)
  ``EMITDataModule``                      emit_as_datamodule.py:27-115 (``prepare_data`` and ``test_dataloader``)
The rescale runs on the device (``features.emit_to_aviris_input`` over ``sc_clip_scale``); each scene is uploaded once.
"""
import logging
import os
from glob import glob
from typing import Dict, List, Optional

import numpy as np
import torch

from . import features, io_formats
from .datamodule import _DataModuleBase

HYPERPARAMS = ("MAGIC_DIV_BY", "RGB_DIV_BY", "MAGIC_CLIP_TO", "RGB_CLIP_TO", "MAGIC_MULT_BY", "RGB_MULT_BY")


def load_emit_dataset(emit_dataset_folder, labels_name="label.tif", verbose=False) -> List[List[Optional[str]]]:
    """[[rgb path, magic path, label path or None], ...] of the scene folders, plume events first"""
    positive_files = sorted(glob(os.path.join(emit_dataset_folder, "plume_events", "*")))
    negative_files = sorted(glob(os.path.join(emit_dataset_folder, "confounders", "*")))
    all_files = [a for a in positive_files + negative_files if os.path.isdir(a)]
    dataset_paths = []
    for one_location in all_files:
        subfiles = sorted(glob(os.path.join(one_location, "*")))
        rgbs = [f for f in subfiles if ("RGB" in f and ".hdr" not in f)]
        if not rgbs:
            raise FileNotFoundError(f"{one_location}: no *_RGB file")
        label_p = os.path.join(one_location, labels_name)
        dataset_paths.append([rgbs[0], rgbs[0].replace("_RGB", "_magic"), label_p if os.path.isfile(label_p) else None])
    if verbose:
        print("The dataset contains", len(dataset_paths))
    return dataset_paths


def _read_envi(path) -> np.ndarray:
    """(bands, lines, samples) array of an ENVI file: what ``rasterio.open(path).read()`` returns"""
    cube, _ = io_formats.open_envi(path)
    return np.ascontiguousarray(np.moveaxis(np.asarray(cube), 2, 0))


def load_data(dataset_paths, load_products="all") -> List[list]:
    """[[rgb (3,H,W), magic (H,W), label (H,W), rgb path], ...], or without the rgb array when ``load_products`` is "mag1c_only" """
    data = []
    for rgb_p, magic_p, label_p in dataset_paths:
        magic_data = _read_envi(magic_p)[0]
        label_data = np.zeros_like(magic_data) if label_p is None else io_formats.read_tiff(label_p)[0]
        if load_products != "mag1c_only":
            data.append([_read_envi(rgb_p), magic_data, label_data, rgb_p])
        else:
            data.append([magic_data, label_data, rgb_p])
    return data


class STARCOPEMITDataset:
    def __init__(self, dataframe_substitute, input_products: List[str], output_products: List[str], weight_loss: Optional[str] = None,
                 spatial_augmentations=None, extra_products: Optional[List[str]] = None, window_size_sample=None, hyperparams=None,
                 device="cuda"):
        self.dataframe_substitute = dataframe_substitute
        self.hyperparams = dict(hyperparams or {})
        self.input_products, self.output_products = input_products, output_products
        self.load_products = "mag1c_only" if len(input_products) == 1 and "mag1c" in input_products else "all"
        self.weight_loss = weight_loss
        self.spatial_augmentations = spatial_augmentations
        self.window_size_sample = window_size_sample
        self.extra_products = [] if extra_products is None else extra_products
        self.add_rgb_aviris = False
        self.device = device
        self._resident: Dict[int, tuple] = {}

    def add_extra_products(self, products_add: List[str]):
        p_add = [p for p in products_add if p not in self.extra_products and p not in self.input_products]
        self.extra_products.extend(p_add)

    def __len__(self):
        return len(self.dataframe_substitute)

    def _scene(self, idx: int):
        if idx not in self._resident:
            data_iter = self.dataframe_substitute[idx]
            rgb, magic = (data_iter[0], data_iter[1]) if self.load_products != "mag1c_only" else (None, data_iter[0])
            up = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(self.device)      # noqa: E731
            self._resident[idx] = (up(magic), None if rgb is None else up(rgb))
        return self._resident[idx]

    def __getitem__(self, idx: int):
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        data_iter = self.dataframe_substitute[idx]
        label, rgb_path = data_iter[-2], data_iter[-1]
        kw = {}
        if len(self.hyperparams) > 0:
            kw = {k.lower(): self.hyperparams[k] for k in HYPERPARAMS}
        magic, rgb = self._scene(idx)
        h, w = (magic.shape[0] // 32) * 32, (magic.shape[1] // 32) * 32
        label = label[:h, :w]
        has_plume = bool(np.max(label) != 0.0)
        plume_data = {"input": features.emit_to_aviris_input(magic, rgb, **kw),
                      "output": torch.from_numpy(np.ascontiguousarray(label / 255.)).unsqueeze(0).to(self.device),
                      "id": [int(idx)], "has_plume": [has_plume]}
        plume_data["weight_loss"] = torch.ones_like(plume_data["output"])        # the reference fakes this one too
        plume_data["debug_rgb_path"] = [rgb_path]
        return plume_data


class EMITLoader:
    """``DataLoader(dataset, batch_size, shuffle=False)`` over scenes of one size: tensors are stacked, the one-element lists
    ``id`` / ``has_plume`` / ``debug_rgb_path`` collate as torch's default collate does ([tensor (B,)] / [list of str])."""

    def __init__(self, dataset: STARCOPEMITDataset, batch_size: int = 1):
        self.dataset, self.batch_size = dataset, int(batch_size)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        dev = self.dataset.device
        for s in range(0, len(self.dataset), self.batch_size):
            items = [self.dataset[i] for i in range(s, min(s + self.batch_size, len(self.dataset)))]
            batch = {k: torch.stack([it[k] for it in items]) for k in ("input", "output", "weight_loss")}
            batch["id"] = [torch.tensor([it["id"][0] for it in items])]                    # stays on the host, like a collated list
            batch["has_plume"] = [torch.tensor([it["has_plume"][0] for it in items], device=dev)]
            batch["debug_rgb_path"] = [[it["debug_rgb_path"][0] for it in items]]
            yield batch


class EMITDataModule(_DataModuleBase):
    def __init__(self, settings, labels_filename="label.tif", hyperparams=None, root_folder=None, device="cuda"):
        super().__init__()
        if root_folder is None:
            raise ValueError("EMITDataModule: root_folder (the folder holding plume_events/ and confounders/) is required")
        self.settings = settings
        self.products_plot = settings.products_plot
        self.batch_size = settings.dataloader.batch_size
        self.num_workers = settings.dataloader.num_workers
        self.input_products = settings.dataset.input_products
        self.output_products = settings.dataset.output_products
        self.load_products = "mag1c_only" if len(self.input_products) == 1 and "mag1c" in self.input_products else "all"
        self.labels_filename = labels_filename
        self.hyperparams = dict(hyperparams or {})
        self.root_folder = root_folder
        self.device_resident = device
        self.weight_loss = settings.dataset.weight_loss if settings.dataset.use_weight_loss else None
        self.weight_sampling = settings.dataset.weight_sampling

    def setup(self, stage: Optional[str] = None) -> None:
        pass

    def prepare_data(self):
        log = logging.getLogger(__name__)
        dataset_paths = load_emit_dataset(self.root_folder, labels_name=self.labels_filename)
        emit_data = load_data(dataset_paths, self.load_products)

        def dataset():
            return STARCOPEMITDataset(emit_data, input_products=self.input_products, weight_loss=self.weight_loss,
                                      output_products=self.output_products, hyperparams=self.hyperparams, device=self.device_resident)
        self.test_dataset = dataset()
        self.test_dataset_plot = dataset()
        if "rgb_aviris" in self.products_plot and not all(b in self.input_products for b in
                                                          ["TOA_AVIRIS_640nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_460nm"]):
            self.test_dataset_plot.add_rgb_aviris = True
        if "mag1c" in self.products_plot and "mag1c" not in self.input_products:
            self.test_dataset_plot.add_extra_products(["mag1c"])
        log.info("Data module ready")
        log.info(f"Input products: {self.input_products} Output products: {self.output_products} Weight loss: {self.weight_loss}")
        log.info(f"Test dataset {len(self.test_dataset)}")

    def test_dataloader(self, num_workers: Optional[int] = None, batch_size: Optional[int] = None):
        return EMITLoader(self.test_dataset, batch_size=batch_size or self.batch_size)
