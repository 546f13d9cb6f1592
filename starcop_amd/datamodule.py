"""Training data path with the tiles resident in HBM.

Mirrors the sample-selection and augmentation logic of /root/reference/starcop/data/datamodule.py and dataset.py:
  ``create_windows``          georeader.slices.create_windows as called at datamodule.py:27-28 (third-party, absent: restated
                              for the one call the reference makes -- (512,512) tiles, window 128, overlap 64, complete windows)
  ``tiled_table``             ``tiled_dataframe`` :17-64: one row per window, ``frac_positives``, ``has_plume`` = frac > 10/64**2,
                              id ``{id}_r{row}_c{col}_w{w}_h{h}``
  ``add_sample_weight``       :342-348 (1/plume_fraction vs 1/(1-plume_fraction))
  ``tile_window_sums``        the label sums behind ``frac_positives`` (:44-49), one ``sc_tile_window_sums`` launch for all tiles
  ``Permian2019DataModule``   :68-315 with the ``STARCOPDataset`` of dataset.py:11-102 (``TileDataset``) over resident tiles
  ``TrainLoader``             ``train_dataloader`` :306-326: ``WeightedRandomSampler(weights, num_samples=len, replacement=True)``
                              (= ``torch.multinomial``), batches of dict(input, output, weight_loss, id, has_plume)
  augmentation                :128-134 kornia ``RandomRotation(p=.5, degrees=90)`` -> ``RandomHorizontalFlip(p=.5)`` ->
                              ``RandomVerticalFlip(p=.5)`` applied to input, label and loss weight with the same parameters
                              (dataset.py:99-102)

What is different underneath: the reference decodes one GeoTIFF window per product per sample in DataLoader workers and
augments on the CPU; 1 GPU consumes ~940 tiles/s = 23 GB/s of decoded fp32 samples, which no host pipeline sustains.  The
whole STARCOP training set (~3 400 tiles x 6 products x 1 MB = 20 GB) fits 14 times into one MI355X's 288 GB, so the tiles
are uploaded once and every batch is cut, rotated and flipped by ONE gather kernel per tensor (``sc_gather_augment``)
straight out of HBM.  The sample folders on disk (one tiled GeoTIFF per product) are decoded by ``io_formats.load_tileset``
(own TIFF reader, thread pool, pinned staging buffers, asynchronous upload) into the ``ResidentTileSet`` below.
kornia is absent from the build image: the rotation follows kornia 0.6.7's ``rotate`` -> ``warp_affine`` ->
``F.grid_sample(align_corners=True, padding_mode="zeros")`` chain and is tested against ``F.grid_sample`` itself.
"""
import logging
import math
import os
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

from . import _lib
from ._lib import check, ptr, stream

try:  # Lightning is optional (absent in the build image): the data module is a plain class without it
    import pytorch_lightning as pl
    _DataModuleBase = pl.LightningDataModule
    HAVE_LIGHTNING = True
except Exception:  # pragma: no cover
    pl = None
    _DataModuleBase = object
    HAVE_LIGHTNING = False

ROTATE, HFLIP, VFLIP = 1, 2, 4
RGB_AVIRIS = ["TOA_AVIRIS_640nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_460nm"]

# what rasterio.windows.Window carries in the reference's tables (datamodule.py:100-103), in read_tiff's order
Window = namedtuple("Window", ["row_off", "col_off", "height", "width"])


def create_windows(shape: Tuple[int, int], window_size: Tuple[int, int], overlap: Tuple[int, int],
                   include_incomplete: bool = False) -> List[Tuple[int, int, int, int]]:
    """(row_off, col_off, height, width) windows on a ``shape`` grid, row-major, stride = window - overlap."""
    sr, sc = window_size[0] - overlap[0], window_size[1] - overlap[1]
    assert sr > 0 and sc > 0, "overlap must be smaller than the window"
    out = []
    for r in range(0, shape[0], sr):
        for c in range(0, shape[1], sc):
            h, w = min(window_size[0], shape[0] - r), min(window_size[1], shape[1] - c)
            if (h, w) != tuple(window_size) and not include_incomplete:
                continue
            out.append((r, c, h, w))
    return out


def add_sample_weight(dataframe: pd.DataFrame) -> pd.DataFrame:
    plume_fraction = np.sum(dataframe["has_plume"]) / dataframe.shape[0]
    plume_weight = 1 / plume_fraction
    non_plume_weight = 1 / (1 - plume_fraction)
    dataframe["sample_weight"] = dataframe["has_plume"].apply(lambda x: plume_weight if x else non_plume_weight)
    return dataframe


def gather_augment(tiles: torch.Tensor, tile, row_off, col_off, cos_t, sin_t, flags, size: Tuple[int, int],
                   mode: str = "bilinear") -> torch.Tensor:
    """(B,C,h,w) batch cut from ``tiles`` (M,C,H,W) on the device; per-item int32 / float32 device tensors."""
    _lib.require_device(tiles)
    lib = _lib.load()
    assert tiles.dtype == torch.float32 and tiles.is_contiguous() and tiles.dim() == 4
    M, C_, Hs, Ws = tiles.shape
    B = tile.numel()
    out = torch.empty((B, C_, size[0], size[1]), dtype=torch.float32, device=tiles.device)
    check(lib.sc_gather_augment(ptr(tiles), M, C_, Hs, Ws, ptr(tile), ptr(row_off), ptr(col_off), ptr(cos_t), ptr(sin_t),
                                ptr(flags), B, size[0], size[1], {"bilinear": 0, "nearest": 1}[mode], ptr(out), stream()))
    return out


def tile_window_sums(labels: torch.Tensor, windows) -> torch.Tensor:
    """float64 (M, K) device tensor: the sum of every window (row_off, col_off, height, width) of ``windows`` over every
    tile of the float32 (M, H, W) device tensor ``labels`` (``sc_tile_window_sums``: fp64, fixed order, exact for {0,1})."""
    labels = torch.as_tensor(labels)
    if labels.dtype != torch.float32 or labels.dim() != 3:
        raise ValueError(f"tile_window_sums: labels must be a float32 (M, H, W) tensor, got {labels.dtype} {tuple(labels.shape)}")
    _lib.require_device(labels)
    lib = _lib.load()
    win = np.ascontiguousarray(np.asarray([tuple(int(v) for v in w) for w in windows], dtype=np.int32).reshape(-1, 4))
    labels = labels.contiguous()
    M, H, W = labels.shape
    K = win.shape[0]
    win_d = torch.from_numpy(win).to(labels.device)
    out = torch.empty((M, K), dtype=torch.float64, device=labels.device)
    check(lib.sc_tile_window_sums(ptr(labels), M, H, W, ptr(win_d), win.ctypes.data, K, ptr(out), stream()))
    return out


class ResidentTileSet:
    """All samples of a split on the device: ``inputs`` (M,C,H,W), ``outputs`` (M,1,H,W), optional ``weight_loss`` (M,1,H,W)."""

    def __init__(self, inputs, outputs, weight_loss=None, ids: Optional[Sequence[str]] = None, device="cuda", extras=None):
        def up(t):
            return None if t is None else torch.as_tensor(t, dtype=torch.float32).to(device).contiguous()
        self.inputs, self.outputs, self.weight_loss = up(inputs), up(outputs), up(weight_loss)
        self.extras = {k: up(v) for k, v in (extras or {}).items()}      # product name -> (M,1,H,W): planes no other tensor holds
        M = self.inputs.shape[0]
        assert self.outputs.shape[0] == M and self.outputs.shape[-2:] == self.inputs.shape[-2:]
        self.ids = list(ids) if ids is not None else [f"sample_{i:05d}" for i in range(M)]
        self.shape = tuple(self.inputs.shape[-2:])

    def __len__(self):
        return self.inputs.shape[0]

    def tiled_table(self, tile_size=(128, 128), overlap=(64, 64)) -> pd.DataFrame:
        """One row per training window (datamodule.py:17-64); the label fractions are summed on the device."""
        wins = create_windows(self.shape, tile_size, overlap, include_incomplete=False)
        sums = tile_window_sums(self.outputs[:, 0], wins).cpu().numpy()       # exact for {0,1} labels
        rows = []
        for m, sid in enumerate(self.ids):
            for k, (ro, co, hh, ww) in enumerate(wins):
                rows.append({"id": f"{sid}_r{ro}_c{co}_w{ww}_h{hh}", "id_original": sid, "tile": m, "window_row_off": ro,
                             "window_col_off": co, "window_width": ww, "window_height": hh,
                             "frac_positives": sums[m, k] / (hh * ww)})
        df = pd.DataFrame(rows)
        df["has_plume"] = df["frac_positives"] > (10 / 64 ** 2)
        return df.set_index("id")


class TrainLoader:
    """Iterable of training batches drawn like the reference's ``train_dataloader`` and augmented on the device."""

    def __init__(self, tileset: ResidentTileSet, table: Optional[pd.DataFrame] = None, batch_size: int = 32,
                 training_size=(128, 128), weight_sampling: bool = True, augment: bool = True, seed: int = 0,
                 mask_mode: str = "bilinear", drop_last: bool = False):
        self.ts = tileset
        self.size = tuple(training_size)
        if table is None:
            if self.size == tileset.shape:
                lab = tileset.outputs.flatten(1)
                table = pd.DataFrame({"id": tileset.ids, "tile": np.arange(len(tileset)), "window_row_off": 0, "window_col_off": 0,
                                      "frac_positives": (lab.sum(1) / lab.shape[1]).cpu().numpy()})
                table["has_plume"] = table["frac_positives"] > (10 / 64 ** 2)
                table = table.set_index("id")
            else:
                table = tileset.tiled_table(self.size)
        self.table = table
        self.batch_size, self.weight_sampling, self.augment = batch_size, weight_sampling, augment
        self.mask_mode, self.drop_last = mask_mode, drop_last
        self.gen = torch.Generator().manual_seed(seed)
        dev = tileset.inputs.device
        self._tile = torch.as_tensor(table["tile"].values, dtype=torch.int32)
        self._row = torch.as_tensor(table["window_row_off"].values, dtype=torch.int32)
        self._col = torch.as_tensor(table["window_col_off"].values, dtype=torch.int32)
        self._has = torch.as_tensor(table["has_plume"].values.astype(np.int64))
        self._ids = list(table.index)
        self._dev = dev

    def __len__(self):
        n = len(self.table)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def epoch_indices(self) -> torch.Tensor:
        """Sample order of one epoch (datamodule.py:311-326)."""
        n = len(self.table)
        if self.weight_sampling:
            w = torch.as_tensor(add_sample_weight(self.table.copy())["sample_weight"].values, dtype=torch.double)
            return torch.multinomial(w, n, True, generator=self.gen)          # == WeightedRandomSampler(w, n, replacement=True)
        return torch.randperm(n, generator=self.gen)

    def draw_augmentation(self, n: int):
        """(cos, sin, flags) of n samples: rotation by U(-90, 90) degrees w.p. .5, h-flip w.p. .5, v-flip w.p. .5."""
        if not self.augment:
            return torch.ones(n), torch.zeros(n), torch.zeros(n, dtype=torch.int32)
        u = torch.rand((4, n), generator=self.gen)
        ang = (u[1] * 180.0 - 90.0) * (math.pi / 180.0)
        rot = u[0] < 0.5
        flags = rot.int() * ROTATE + (u[2] < 0.5).int() * HFLIP + (u[3] < 0.5).int() * VFLIP
        return torch.where(rot, torch.cos(ang), torch.ones(n)), torch.where(rot, torch.sin(ang), torch.zeros(n)), flags.int()

    def make_batch(self, idx: torch.Tensor, cos_t, sin_t, flags):
        dev = self._dev
        a = [t.to(dev, non_blocking=True) for t in (self._tile[idx], self._row[idx], self._col[idx], cos_t.float(), sin_t.float(), flags)]
        ts = self.ts
        batch = {"input": gather_augment(ts.inputs, *a, self.size),
                 "output": gather_augment(ts.outputs, *a, self.size, mode=self.mask_mode)}
        if ts.weight_loss is not None:
            batch["weight_loss"] = gather_augment(ts.weight_loss, *a, self.size)
        batch["id"] = [self._ids[i] for i in idx.tolist()]
        batch["has_plume"] = self._has[idx].to(dev)
        return batch

    def __iter__(self):
        order = self.epoch_indices()
        for s in range(0, order.numel(), self.batch_size):
            idx = order[s:s + self.batch_size]
            if self.drop_last and idx.numel() < self.batch_size:
                break
            yield self.make_batch(idx, *self.draw_augmentation(idx.numel()))


# ------------------------------------------------------------------------------------------------ the data module
def _collate_windows(frame: pd.DataFrame, idx: Sequence[int]):
    rows = frame.iloc[list(idx)]
    size = {(int(h), int(w)) for h, w in zip(rows["window_height"], rows["window_width"])}
    if len(size) != 1:
        raise ValueError(f"the windows of a batch must share one size, got {sorted(size)}")
    return rows, size.pop()


class TileDataset:
    """``STARCOPDataset`` (dataset.py:11-102) over a ``ResidentTileSet``: the rows of ``dataframe`` name a tile (column ``tile``)
    and a window inside it; an item is the reference's dict with device tensors, cut by ``sc_gather_augment`` (exact copies)."""

    def __init__(self, dataframe: pd.DataFrame, tileset: ResidentTileSet, input_products: List[str], output_products: List[str],
                 weight_loss: Optional[str] = None, extra_products: Optional[List[str]] = None):
        assert "folder" in dataframe.columns, "folder not in columns of dataframe"
        self.dataframe, self.tileset = dataframe, tileset
        self.input_products, self.output_products, self.weight_loss = list(input_products), list(output_products), weight_loss
        self.extra_products = [] if extra_products is None else extra_products
        self.add_rgb_aviris = False

    def add_extra_products(self, products_add: List[str]):
        p_add = [p for p in products_add if p not in self.extra_products and p not in self.input_products]
        self.extra_products.extend(p_add)

    def __len__(self):
        return self.dataframe.shape[0]

    def _plane(self, name: str, items, size, batch):
        ts = self.tileset
        if name in ts.extras:
            return gather_augment(ts.extras[name], *items, size)
        if name in self.input_products:
            c = self.input_products.index(name)
            return batch["input"][:, c:c + 1]
        raise KeyError(f"product {name!r} is not resident: load it as an input or an extra product")

    def batch(self, idx: Sequence[int]) -> Dict[str, object]:
        """the rows ``idx`` as one batch dict (what the reference's DataLoader collates from ``__getitem__``)"""
        rows, size = _collate_windows(self.dataframe, idx)
        ts, dev, n = self.tileset, self.tileset.inputs.device, len(rows)
        col = lambda name: torch.as_tensor(rows[name].values.astype(np.int32)).to(dev)     # noqa: E731
        items = (col("tile"), col("window_row_off"), col("window_col_off"), torch.ones(n, device=dev), torch.zeros(n, device=dev),
                 torch.zeros(n, dtype=torch.int32, device=dev))
        out = {"input": gather_augment(ts.inputs, *items, size), "output": gather_augment(ts.outputs, *items, size)}
        if self.weight_loss is not None:
            out["weight_loss"] = gather_augment(ts.weight_loss, *items, size)
        for name in self.extra_products:
            out[name] = self._plane(name, items, size, out)
        if self.add_rgb_aviris:
            from .features import _clip_scale
            rgb = torch.cat([self._plane(name, items, size, out) for name in RGB_AVIRIS], dim=1)
            out["rgb_aviris"] = _clip_scale(rgb, 50.0, -math.inf, math.inf, 1.0)        # float32 x / 50.
        out["id"] = [str(i) for i in rows.index]
        out["has_plume"] = torch.as_tensor(rows["has_plume"].values.astype(np.int64)).to(dev)
        return out

    def __getitem__(self, idx: int):
        if not -len(self) <= idx < len(self):
            raise IndexError(idx)
        b = self.batch([idx])
        item = {k: v[0] for k, v in b.items() if torch.is_tensor(v) and k != "has_plume"}
        item["id"] = b["id"][0]
        item["has_plume"] = int(b["has_plume"][0])
        return item


class TileLoader:
    """Batches of a ``TileDataset`` without augmentation: in table order (the evaluation loaders), shuffled, or drawn like
    ``WeightedRandomSampler(sample_weight, len, replacement=True)`` (``train_plot_dataloader`` :252-267)."""

    def __init__(self, dataset: TileDataset, batch_size: int = 1, shuffle: bool = False, weight_sampling: bool = False,
                 seed: Optional[int] = None):
        self.dataset, self.batch_size, self.shuffle, self.weight_sampling = dataset, int(batch_size), shuffle, weight_sampling
        self.gen = torch.Generator().manual_seed(_seed(seed))

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.dataset)
        if self.weight_sampling:
            w = torch.as_tensor(add_sample_weight(self.dataset.dataframe.copy())["sample_weight"].values, dtype=torch.double)
            order = torch.multinomial(w, n, True, generator=self.gen).tolist()
        elif self.shuffle:
            order = torch.randperm(n, generator=self.gen).tolist()
        else:
            order = list(range(n))
        for s in range(0, n, self.batch_size):
            yield self.dataset.batch(order[s:s + self.batch_size])


def _seed(seed: Optional[int]) -> int:
    """the reference's loaders are unseeded: without a seed, one is drawn from torch's global generator"""
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if seed is None else int(seed)


TILED_COLUMNS = ["frac_positives", "has_plume", "window_col_off", "window_row_off", "window_width", "window_height", "id_original"]


def tiled_dataframe(dataframe: pd.DataFrame, tileset: ResidentTileSet, tile_size: Tuple[int, int], overlap: Tuple[int, int]) -> pd.DataFrame:
    """datamodule.py:17-64: one row per (sample, window) with the sample's own columns, ``frac_positives`` (label sum / window
    size, all label sums from one ``tile_window_sums`` launch), ``has_plume`` = frac > 10/64**2, the window columns,
    ``id_original`` and the index ``{id}_r{row}_c{col}_w{w}_h{h}``.  The window grid covers the tiles' own shape."""
    wins = [Window(*w) for w in create_windows(tileset.shape, tuple(tile_size), tuple(overlap), include_incomplete=False)]
    lab = tileset.outputs
    M, Co, H, W = lab.shape
    sums = tile_window_sums(lab.reshape(M * Co, H, W), wins).reshape(M, Co, len(wins)).sum(1).cpu().numpy()
    rows = []
    for row in dataframe.reset_index().to_dict(orient="records"):
        for k in ("window_row_off", "window_col_off", "window_width", "window_height"):
            del row[k]
        m = int(row["tile"])
        for k, w in enumerate(wins):
            row_copy = dict(row)
            row_copy["window"] = w
            row_copy["frac_positives"] = sums[m, k] / (Co * w.height * w.width)
            rows.append(row_copy)
    df = pd.DataFrame(rows)
    df["has_plume"] = df["frac_positives"] > (10 / 64 ** 2)
    for attr_name in ["col_off", "row_off", "width", "height"]:
        df[f"window_{attr_name}"] = df["window"].apply(lambda x: getattr(x, attr_name))
    df["id_original"] = df["id"].copy()
    df["id"] = df.apply(lambda r: f"{r['id']}_r{r.window_row_off}_c{r.window_col_off}_w{r.window_width}_h{r.window_height}", axis=1)
    return df.set_index("id")


def _add_windows(df: pd.DataFrame) -> pd.DataFrame:
    df["window"] = df.apply(lambda row: Window(row_off=int(row.window_row_off), col_off=int(row.window_col_off),
                                               height=int(row.window_height), width=int(row.window_width)), axis=1)
    return df


class Permian2019DataModule(_DataModuleBase):
    """The reference's data module (datamodule.py:68-315) over tiles resident in HBM: same attributes, ``prepare_data`` and
    loader methods; the datasets are ``TileDataset`` objects and the loaders yield batch dicts of device tensors.  Where the
    reference downloads a missing split, this one raises ``FileNotFoundError``."""

    def __init__(self, settings, device="cuda"):
        super().__init__()
        self.settings = settings
        self.device_resident = device
        self.products_plot = settings.products_plot
        self.batch_size = settings.dataloader.batch_size
        self.num_workers = settings.dataloader.num_workers
        self.input_products = settings.dataset.input_products
        self.output_products = settings.dataset.output_products
        self.training_size = settings.dataset.training_size
        self.training_size_overlap = settings.dataset.training_size_overlap
        self.root_folder = settings.dataset.root_folder
        self.train_csv = settings.dataset.train_csv
        self.test_csv = "test.csv"
        self.weight_loss = settings.dataset.weight_loss if settings.dataset.use_weight_loss else None
        self.weight_sampling = settings.dataset.weight_sampling

    def setup(self, stage: Optional[str] = None) -> None:
        pass

    def load_dataframe(self, path) -> pd.DataFrame:
        df = _add_windows(pd.read_csv(path))
        df["folder"] = df["id"].apply(lambda x: os.path.join(self.root_folder, str(x)))
        return df.set_index("id")

    def split_products(self) -> Tuple[List[str], List[str]]:
        """(raw bands, features to extract) among the input, output and loss-weight products (datamodule.py:137-143)"""
        from . import features
        raw = set(features.raw_bands_available())
        wanted = list(self.input_products) + list(self.output_products) + ([self.weight_loss] if self.weight_loss is not None else [])
        return [f for f in wanted if f in raw], [f for f in wanted if f not in raw]

    def tiled_csv_path(self) -> str:
        name_csv, ext = os.path.splitext(self.train_csv)
        return os.path.join(self.root_folder, f"{name_csv}_tiled_{self.training_size[0]}_{self.training_size[1]}{ext}")

    def _resident(self, dataframe: pd.DataFrame, extras: List[str]) -> ResidentTileSet:
        from . import io_formats
        ts = io_formats.load_tileset(list(dataframe["folder"]), self.input_products, self.output_products, self.weight_loss,
                                     ids=[str(i) for i in dataframe.index], device=self.device_resident, extra_products=extras,
                                     workers=max(1, int(self.num_workers or 1)))
        dataframe["tile"] = np.arange(len(dataframe))
        return ts

    def prepare_data(self):
        from . import features
        log = logging.getLogger(__name__)
        self.raw_bands, self.features_extract = self.split_products()
        train_dataset_path = os.path.join(self.root_folder, self.train_csv)
        test_dataset_path = os.path.join(self.root_folder, self.test_csv)
        for path in (train_dataset_path, test_dataset_path):
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path} not found: the reference downloads the split here; this build does not. "
                                        f"sampling.WindowDataset.cache(folder, name) writes the sample folders and {os.path.basename(path)}")
        # products only the plot loaders show (:236-243); each plane is stored once, so only what the inputs do not hold
        rgb_plot = "rgb_aviris" in self.products_plot and not all(b in self.input_products for b in RGB_AVIRIS)
        mag1c_plot = "mag1c" in self.products_plot and "mag1c" not in self.input_products
        extras = [b for b in (RGB_AVIRIS if rgb_plot else []) + (["mag1c"] if mag1c_plot else []) if b not in self.input_products]

        self.train_dataframe_original = self.load_dataframe(train_dataset_path)
        if len(self.features_extract) > 0:
            features.extract_features(self.features_extract, self.train_dataframe_original, device=self.device_resident)
        self.train_tiles = self._resident(self.train_dataframe_original, extras)

        if np.any(np.array(self.training_size) < np.array(self.train_tiles.shape)):
            path_tiled = self.tiled_csv_path()
            if not os.path.exists(path_tiled):
                log.info(f"Tiled dataset {path_tiled} not found. Generating")
                train_dataframe = tiled_dataframe(self.train_dataframe_original, self.train_tiles, self.training_size,
                                                  self.training_size_overlap)
                train_dataframe[[c for c in train_dataframe.columns if c not in ("window", "tile")]].to_csv(path_tiled)
            else:
                log.info(f"Loading tiled dataset {path_tiled}")
                train_dataframe = _add_windows(pd.read_csv(path_tiled))
                train_dataframe["folder"] = train_dataframe["id_original"].apply(lambda x: os.path.join(self.root_folder, str(x)))
                tile_of = {str(i): t for i, t in zip(self.train_dataframe_original.index, self.train_dataframe_original["tile"])}
                train_dataframe["tile"] = train_dataframe["id_original"].apply(lambda x: tile_of[str(x)])
                train_dataframe = train_dataframe.set_index("id")
        else:
            train_dataframe = self.train_dataframe_original

        def dataset(frame, tiles):
            return TileDataset(frame, tiles, self.input_products, self.output_products, self.weight_loss)
        self.train_dataset = dataset(train_dataframe, self.train_tiles)            # augmented by train_dataloader
        self.train_dataset_plot = dataset(train_dataframe, self.train_tiles)
        self.train_dataset_non_tiled = dataset(self.train_dataframe_original, self.train_tiles)

        test_dataframe = self.load_dataframe(test_dataset_path)
        test_dataframe = test_dataframe.sort_values(["has_plume", "qplume"], ascending=False)
        if len(self.features_extract) > 0:
            features.extract_features(self.features_extract, test_dataframe, device=self.device_resident)
        self.test_tiles = self._resident(test_dataframe, extras)
        self.test_dataset = dataset(test_dataframe, self.test_tiles)
        self.test_dataset_plot = dataset(test_dataframe, self.test_tiles)
        if rgb_plot:
            self.train_dataset_plot.add_rgb_aviris = True
            self.test_dataset_plot.add_rgb_aviris = True
        if mag1c_plot:
            self.train_dataset_plot.add_extra_products(["mag1c"])
            self.test_dataset_plot.add_extra_products(["mag1c"])
        self.val_dataset = self.test_dataset
        log.info("Data module ready")
        log.info(f"Input products: {self.input_products} Output products: {self.output_products} Weight loss: {self.weight_loss}")
        log.info(f"Train dataset {len(self.train_dataset)} chipsize: {self.training_size}")
        log.info(f"Val dataset {len(self.val_dataset)}")
        log.info(f"Test dataset {len(self.test_dataset)}")

    def loader(self, dataset: TileDataset, batch_size: int = 1, shuffle: bool = False, seed: Optional[int] = None) -> TileLoader:
        """what ``DataLoader(dataset, batch_size=..., shuffle=...)`` is in the reference's scripts (train.py:159)"""
        return TileLoader(dataset, batch_size=batch_size, shuffle=shuffle, seed=seed)

    def train_plot_dataloader(self, batch_size: int, num_workers: int = 0, seed: Optional[int] = None):
        return TileLoader(self.train_dataset_plot, batch_size=batch_size, shuffle=not self.weight_sampling,
                          weight_sampling=bool(self.weight_sampling), seed=seed)

    def test_plot_dataloader(self, batch_size: int, num_workers: int = 0):
        return TileLoader(self.test_dataset_plot, batch_size=batch_size)

    def train_dataloader(self, num_workers: Optional[int] = None, batch_size: Optional[int] = None, seed: Optional[int] = None):
        """``TrainLoader``: the reference's sampler, augmentation by ``sc_gather_augment``"""
        frame = self.train_dataset.dataframe
        size = {(int(h), int(w)) for h, w in zip(frame["window_height"], frame["window_width"])}
        assert len(size) == 1, f"training windows of several sizes: {sorted(size)}"
        loader = TrainLoader(self.train_tiles, frame, batch_size=batch_size or self.batch_size, training_size=size.pop(),
                             weight_sampling=bool(self.weight_sampling), augment=True, seed=_seed(seed))
        loader.dataset = self.train_dataset
        return loader

    def val_dataloader(self, num_workers: Optional[int] = None, batch_size: Optional[int] = None):
        return TileLoader(self.val_dataset, batch_size=batch_size or self.batch_size)

    def test_dataloader(self, num_workers: Optional[int] = None, batch_size: Optional[int] = None):
        return TileLoader(self.test_dataset, batch_size=batch_size or self.batch_size)
