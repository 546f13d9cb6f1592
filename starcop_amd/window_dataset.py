"""Cutting the sampled windows of flight lines into sample folders on the GPU: step 4 of the reference's dataset production.

Mirrors starcop/data/sampling_dataset.py:182-386 (``WindowDataset.__getitem__``, ``cache_item``, ``cache``):
  ``WindowDataset[idx]``     every product of the row's flight-line folder read "boundless" through the row's window (pixels the
                             raster does not hold and nodata become 0), S2 / WV3 bands turned into top-of-atmosphere reflectance
                             (``* factor / 100 / SOLAR_IRRADIANCE`` and a clip to [0, 2]), AVIRIS bands normalised (``* factor``),
                             mag1c clipped to [0, 10000], and ``labelbinary`` = ``mask_creation.proposed_mask`` of the cut arrays
  ``WindowDataset.cache``    one sample folder per row with one tiled GeoTIFF per product, and the two tables of the split
All windows of a chunk of a flight line and all products of one element width are cut, scaled and clipped by ONE
``sc_window_cut`` launch (include/starcop_hip.h) from sources that are decoded once per chunk; there is no CPU fallback.

Three things are restated or moved, because georeader, rasterio and pysolar are not dependencies of this package (equality with
the reference is argued from these restatements, the reference itself cannot be executed without them):
  * ``pad_window_to_size`` restates ``georeader.window_utils.pad_window_to_size``: a dimension smaller than the target grows by
    ``pad = target - size``, ``pad // 2`` on the leading side and the rest on the trailing side; a dimension that is already
    large enough is unchanged;
  * the multiply is ``x * float32(s)`` with ``s`` evaluated in float64 in the reference's order: what ``values *= s`` computes on
    a float32 array under numpy 1.x (the numpy of the published dataset; numpy >= 2 would round a float64 product);
  * the solar altitude behind the acquisition-date factor is an input (``toa_correction_factor={folder: factor}`` or a
    ``solar_altitude`` column in degrees), see ``aviris.observation_date_correction_factor``.
A window is a ``(row_off, col_off, height, width)`` tuple or an object with those attributes, as in ``sampling.py``.
"""
import json
import os
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, aviris, mask_creation
from . import io_formats as io
from ._lib import check, sc_wcut_args, stream
from .planes import chunks, match_bits, set_plane_ops, set_planes
from .sampling import _nodata, _rchw

NOUT_MAX = _lib.WCUT_MAX_PLANES
MEMORY_BUDGET = 2 << 30            # bytes of source row band a chunk of windows may hold on the device


# ------------------------------------------------------------------------------------------------ host rules
def pad_window_to_size(window, size: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """``georeader.window_utils.pad_window_to_size(window, size)`` restated (see the module docstring): ``size`` = (height,
    width) -> (row_off, col_off, height, width)"""
    r, c, h, w = _rchw(window)
    th, tw = int(size[-2]), int(size[-1])
    if h < th:
        r, h = r - (th - h) // 2, th
    if w < tw:
        c, w = c - (tw - w) // 2, tw
    return r, c, h, w


def _is_toa(name: str) -> bool:
    return name.startswith("S2") or name.startswith("WV")


def save_name(key: str, normalize_by_acquisition_date: bool = True) -> str:
    """file stem of a product in a sample folder (sampling_dataset.py:338-347): with normalisation ``TOA_{k}`` for S2 / WV
    products and ``TOA_AVIRIS_{k}`` for ``..nm`` and numeric keys (a normalised radiance, not a reflectance); else the key"""
    if normalize_by_acquisition_date and (_is_toa(key) or key.endswith("nm") or key.isnumeric()):
        return f"TOA_AVIRIS_{key}" if (key.endswith("nm") or key.isnumeric()) else f"TOA_{key}"
    return key


def product_ops(path_name: str, normalize_by_acquisition_date: bool, factor: Optional[float]):
    """(scale, clip) of a product read from ``{path_name}.tif`` (sampling_dataset.py:273-293): ``scale`` is the float64 the
    reference multiplies by (None: no multiply), ``clip`` = (lo, hi) or None"""
    scale, clip = None, None
    if normalize_by_acquisition_date and (_is_toa(path_name) or path_name.isnumeric()):
        if _is_toa(path_name):
            sensor, band = path_name.split("_")
            if len(band) == 2:
                band = f"B0{band[-1]}"
            scale = factor / 100 / aviris.SOLAR_IRRADIANCE[sensor][band]
            clip = (0.0, 2.0)
        else:
            scale = factor
    if path_name == "mag1c":
        clip = (0.0, 10_000.0)
    return scale, clip


def plan_chunks(folders: Sequence[str], windows: Sequence[Any], scene_rows: Dict[str, int], row_bytes: Dict[str, int],
                budget_bytes: int = MEMORY_BUDGET) -> List[Dict[str, Any]]:
    """Rows of the table -> chunks that are cut together.  Rows are grouped by ``folder`` (first appearance order); inside a
    flight line they are sorted by row offset (stable) and taken in order into a chunk while the joint row band of the chunk,
    ``row_bytes[folder]`` bytes per row, fits ``budget_bytes`` (a chunk always takes at least one window).  Returns
    [{"folder", "rows": positions in the table, "band": (first row, end row)}]; the band is the part of the flight line
    (``scene_rows[folder]`` rows) its windows touch, at least one row."""
    by_folder: Dict[str, List[int]] = {}
    for i, f in enumerate(folders):
        by_folder.setdefault(f, []).append(i)
    chunks = []
    for f, rows in by_folder.items():
        H = int(scene_rows[f])

        def band(lo, hi):
            b0 = min(max(lo, 0), H - 1)
            return b0, min(max(hi, b0 + 1), H)
        rows = sorted(rows, key=lambda i: _rchw(windows[i])[0])
        cur, lo, hi = [], 0, 0
        for i in rows:
            r, _, h, _ = _rchw(windows[i])
            nlo, nhi = (r, r + h) if not cur else (min(lo, r), max(hi, r + h))
            b0, b1 = band(nlo, nhi)
            if cur and (b1 - b0) * int(row_bytes[f]) > budget_bytes:
                chunks.append({"folder": f, "rows": cur, "band": band(lo, hi)})
                cur, nlo, nhi = [], r, r + h
            cur.append(i)
            lo, hi = nlo, nhi
        if cur:
            chunks.append({"folder": f, "rows": cur, "band": band(lo, hi)})
    return chunks


# ------------------------------------------------------------------------------------------------ the launch
class Plane(NamedTuple):
    """one source plane of ``window_cut``: a 2-D device view (any non-negative strides) whose element (0, 0) is the scene's
    (row0, col0); ``fill``: the value that reads as 0 (None: none), ``scale``: float64 multiplier (None: none), ``clip``: (lo, hi)"""
    data: torch.Tensor
    row0: int = 0
    col0: int = 0
    fill: Optional[float] = None
    scale: Optional[float] = None
    clip: Optional[Tuple[float, float]] = None


def window_cut(planes: Sequence[Plane], offsets, out_size: Tuple[int, int], scene_shape: Optional[Tuple[int, int]] = None):
    """``sc_window_cut``: cut ``len(offsets)`` windows of ``out_size`` = (height, width) at ``offsets`` = [(row_off, col_off)]
    out of the planes -> dense device tensor (n_win, P, height, width) in the planes' dtype (one dtype of 1, 2 or 4 bytes per
    call; scale / clip need float32).  ``scene_shape``: the grid the offsets refer to (default: the hull of the planes)."""
    planes = list(planes)
    if not planes:
        raise ValueError("window_cut: no planes")
    dt, dev = planes[0].data.dtype, planes[0].data.device
    if any(p.data.dtype != dt or p.data.device != dev or p.data.dim() != 2 for p in planes):
        raise ValueError("window_cut: all planes of a call are 2-D and share one dtype and device")
    nd = torch.empty(0, dtype=dt).numpy().dtype
    if nd.kind not in "fiu" or nd.itemsize not in (1, 2, 4):
        raise ValueError(f"window_cut: dtype {dt} is not supported (1-, 2- or 4-byte integers and float32)")
    if any(p.scale is not None or p.clip is not None for p in planes) and dt != torch.float32:
        raise ValueError(f"window_cut: scale / clip need float32 planes, got {dt}")
    _lib.require_device(planes[0].data)
    lib = _lib.load()
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1, 2))
    if off.shape[0] == 0:
        raise ValueError("window_cut: no windows")
    if np.abs(off).max() >= 2 ** 31:
        raise ValueError("window_cut: window offsets leave the int32 range")
    off = off.astype(np.int32)
    off_d = torch.from_numpy(off).to(dev)
    oh, ow = int(out_size[0]), int(out_size[1])
    if scene_shape is None:
        scene_shape = (max(p.row0 + p.data.shape[0] for p in planes), max(p.col0 + p.data.shape[1] for p in planes))
    n = off.shape[0]
    data = [p.data for p in planes]
    outs = []
    for p0, count in chunks(len(planes), NOUT_MAX):
        out = torch.empty((n, count, oh, ow), dtype=dt, device=dev)
        a = sc_wcut_args()
        a.scene_rows, a.scene_cols, a.out_h, a.out_w = int(scene_shape[0]), int(scene_shape[1]), oh, ow
        a.P, a.elem_bytes, a.n_win = count, nd.itemsize, n
        a.win_off, a.win_off_host = off_d.data_ptr(), off.ctypes.data
        set_planes(a, data, p0, rows=a.rows, cols=a.cols)
        for k, p in enumerate(planes[p0:p0 + count]):
            a.row0[k], a.col0[k] = int(p.row0), int(p.col0)
            set_plane_ops(a, k, match_bits(p.fill, nd) if p.fill is not None else None, p.scale, p.clip)
        a.out = out.data_ptr()
        check(lib.sc_window_cut(a, stream()))
        outs.append(out)
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


# ------------------------------------------------------------------------------------------------ the dataset
def _no_gs(path):
    if str(path).startswith("gs://"):
        raise NotImplementedError(f"{path}: reading from / writing to Google Cloud Storage is not supported")


class WindowDataset:
    """sampling_dataset.py:182-386.  ``dataframe``: one row per sample with ``folder`` (the flight-line folder), ``window`` and
    -- for the acquisition-date factor -- ``datetime`` and ``solar_altitude`` (degrees) unless ``toa_correction_factor`` =
    {folder: factor} is given; the first row of a folder decides its factor, as the reference caches it per folder (:275-279).
    ``products``: names read from ``{folder}/{name}.tif``.  ``wavelengths`` (nm): for each, the band of the flight line whose
    centre is closest, under the key ``"{w:.0f}nm"``; the bands come from ``{folder}/{band_index}.tif`` with the centres of
    ``{folder}/metadata.json`` when that file exists, else from the ENVI radiance ``{folder}/{name}_img``.  ``output_size``:
    windows are padded to it (``pad_window_to_size``); a window that is larger raises ValueError.  Items are dicts of numpy
    arrays (bands, height, width); the georeferencing travels as GeoTIFF tags in ``cache``.  With
    ``normalize_by_acquisition_date`` and a product that needs the factor (S2*, WV*, numeric names, ``wavelengths``) but neither
    source for it, the constructor raises ValueError before any file is touched."""

    def __init__(self, dataframe, products: List[str], read_label_path: bool = False, read_rgb_path: bool = False,
                 wavelengths: Optional[List[float]] = None, output_size: Optional[Tuple[int, int]] = None,
                 normalize_by_acquisition_date: bool = True, proposed_mask: bool = True,
                 toa_correction_factor: Optional[Dict[str, float]] = None, device=None, memory_budget: int = MEMORY_BUDGET):
        if read_label_path or read_rgb_path:
            raise NotImplementedError("read_label_path / read_rgb_path are deprecated in the reference (labels come from "
                                      "label_rgba.tif) and are not supported")
        self.dataframe = dataframe.copy()
        self.products = list(products)
        self.proposed_mask = proposed_mask
        if proposed_mask and not {"label_rgba", "mag1c"} <= set(self.products):
            raise ValueError("proposed_mask=True needs the products 'label_rgba' and 'mag1c'")
        self.normalize_by_acquisition_date = normalize_by_acquisition_date
        self.wavelengths = np.array(wavelengths, dtype=np.float64) if wavelengths is not None else None
        self.wavelengths_names = [f"{w:.0f}nm" for w in self.wavelengths] if wavelengths is not None else []
        self.output_size = (int(output_size[-2]), int(output_size[-1])) if output_size is not None else None
        self.device = torch.device(device if device is not None else "cuda")
        self.memory_budget = int(memory_budget)
        self.folders = [str(f) for f in self.dataframe["folder"]]
        for f in self.folders:
            _no_gs(f)
        wins = [_rchw(w) for w in self.dataframe["window"]]
        if self.output_size is not None:
            wins = [pad_window_to_size(w, self.output_size) for w in wins]
            for w in wins:
                if (w[2], w[3]) != self.output_size:
                    raise ValueError(f"window {w} is larger than output_size {self.output_size}")
        if any(w[2] < 1 or w[3] < 1 for w in wins):
            raise ValueError("windows need a positive height and width")
        self.windows = wins
        self.dataframe["window"] = wins
        self.toa_correction_factor: Dict[str, float] = {}
        needs = normalize_by_acquisition_date and (self.wavelengths is not None or any(_is_toa(p) or p.isnumeric() for p in self.products))
        if needs:
            given = dict(toa_correction_factor or {})
            has_alt = "solar_altitude" in self.dataframe.columns and "datetime" in self.dataframe.columns
            for pos, f in enumerate(self.folders):
                if f in self.toa_correction_factor:
                    continue
                if f in given:
                    self.toa_correction_factor[f] = float(given[f])
                elif has_alt:
                    row = self.dataframe.iloc[pos]
                    when = row["datetime"]
                    when = when.to_pydatetime() if hasattr(when, "to_pydatetime") else when
                    self.toa_correction_factor[f] = float(aviris.observation_date_correction_factor(when, float(row["solar_altitude"])))
                else:
                    raise ValueError(f"normalize_by_acquisition_date=True needs the acquisition-date factor of {f}: pass "
                                     "toa_correction_factor={folder: factor} or give the table a 'solar_altitude' column (degrees) "
                                     "next to 'datetime' (aviris.observation_date_correction_factor)")
        self._sources: Dict[str, Dict[str, Any]] = {}

    def __len__(self):
        return len(self.folders)

    # -------------------------------------------------------------------------------------------- sources of a flight line
    def _folder_sources(self, folder: str) -> Dict[str, Any]:
        """what is read in ``folder``: entries (key, path_name, kind, ...) in the reference's order (:259-260), the grid of the
        flight line and the bytes one of its rows takes on the device.  Raises FileNotFoundError for a missing product."""
        if folder in self._sources:
            return self._sources[folder]
        entries = []

        def tif(key, path_name):
            path = os.path.join(folder, f"{path_name}.tif")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{folder}: missing {path_name}.tif")
            info = io.tiff_info(path)
            if info.dtype.itemsize not in (1, 2, 4):
                raise NotImplementedError(f"{path}: {info.dtype} samples are not supported (1-, 2- or 4-byte samples)")
            entries.append({"key": key, "path_name": path_name, "kind": "tif", "path": path, "info": info, "geo": info,
                            "shape": (info.height, info.width), "fill": _nodata(info),
                            "row_bytes": info.width * info.bands * info.dtype.itemsize})
        for name in self.products:
            tif(name, name)
        if self.wavelengths is not None:
            meta_path = os.path.join(folder, "metadata.json")
            if os.path.exists(meta_path):                                    # one file per band (:249-257)
                with open(meta_path) as fh:
                    centres = np.array(json.load(fh)["wavelengths"], dtype=np.float64)
                for key, b in zip(self.wavelengths_names, np.argmin(np.abs(self.wavelengths[:, None] - centres), axis=1)):
                    tif(key, f"{b}")
            else:                                                            # the ENVI radiance cube of steps 1-2
                name = os.path.basename(folder.rstrip("/"))
                path = os.path.join(folder, f"{name}_img")
                if not os.path.exists(path):
                    raise FileNotFoundError(f"{folder}: neither metadata.json nor the ENVI radiance {name}_img")
                cube, meta = io.open_envi(path)
                if meta["wavelengths"] is None:
                    raise ValueError(f"{path}: the ENVI header has no wavelengths")
                if cube.dtype.itemsize != 4 or cube.dtype.kind != "f":
                    raise NotImplementedError(f"{path}: {cube.dtype} radiance is not supported (float32)")
                ignore = meta["header"].get("data ignore value")
                geo = io.envi_geo_tags(meta["header"])
                bands = np.argmin(np.abs(self.wavelengths[:, None] - meta["wavelengths"]), axis=1)
                for key, b in zip(self.wavelengths_names, bands):
                    entries.append({"key": key, "path_name": f"{b}", "kind": "envi", "path": path, "band": int(b), "geo": geo,
                                    "shape": tuple(cube.shape[:2]), "fill": float(ignore) if ignore is not None else None,
                                    "row_bytes": 0})
                if len(bands):
                    entries[-1]["row_bytes"] = int(cube.shape[1] * cube.shape[2] * 4)       # the cube is uploaded once
        src = {"entries": entries, "shape": (max(e["shape"][0] for e in entries), max(e["shape"][1] for e in entries)),
               "row_bytes": sum(e["row_bytes"] for e in entries)}
        self._sources[folder] = src
        return src

    def _load_band(self, folder: str, band: Tuple[int, int], keep: list):
        """decode every source of ``folder`` once for the rows ``band`` of the flight line and upload them through pinned memory
        -> [(entry, [Plane per band of the product])]"""
        src = self._folder_sources(folder)
        factor = self.toa_correction_factor.get(folder)
        cubes: Dict[str, torch.Tensor] = {}

        def upload(a):
            t = torch.from_numpy(np.ascontiguousarray(a))
            if self.device.type == "cuda":
                t = t.pin_memory()
                keep.append(t)
            return t.to(self.device, non_blocking=True)
        loaded = []
        for e in src["entries"]:
            H, W = e["shape"]
            b0 = min(band[0], H - 1)
            b1 = min(max(band[1], b0 + 1), H)
            scale, clip = product_ops(e["path_name"], self.normalize_by_acquisition_date, factor)
            if e["kind"] == "tif":
                a = io.read_tiff(e["path"], window=(b0, 0, b1 - b0, W), info=e["info"])
                if (scale is not None or clip is not None) and a.dtype != np.float32:
                    raise ValueError(f"{e['path']}: scaling / clipping needs float32 samples, got {a.dtype}")
                t = upload(a)
                views = [t[k] for k in range(t.shape[0])]
            else:
                if e["path"] not in cubes:
                    cube, _ = io.open_envi(e["path"])
                    cubes[e["path"]] = upload(np.array(cube[b0:b1], dtype=np.float32))       # only the row band, all bands
                views = [cubes[e["path"]][:, :, e["band"]]]                 # a strided plane of the pixel-interleaved cube
            loaded.append((e, [Plane(v, b0, 0, e["fill"], scale, clip) for v in views]))
        return loaded

    def _cut(self, folder: str, rows: Sequence[int], band: Tuple[int, int]) -> List[Dict[str, np.ndarray]]:
        """the items of the table rows ``rows`` (all in ``folder``) whose windows lie in the rows ``band`` of the flight line"""
        src = self._folder_sources(folder)
        keep: list = []
        loaded = self._load_band(folder, band, keep)
        items: List[Dict[str, np.ndarray]] = [dict() for _ in rows]
        by_shape: Dict[Tuple[int, int], List[int]] = {}
        for k, i in enumerate(rows):
            by_shape.setdefault(self.windows[i][2:], []).append(k)
        by_dtype: Dict[torch.dtype, List[int]] = {}
        for j, (_, planes) in enumerate(loaded):
            by_dtype.setdefault(planes[0].data.dtype, []).append(j)
        for shape, ks in by_shape.items():
            offsets = [self.windows[rows[k]][:2] for k in ks]
            dev_out: Dict[str, torch.Tensor] = {}
            for js in by_dtype.values():                                     # one launch per element type
                planes = [p for j in js for p in loaded[j][1]]
                out = window_cut(planes, offsets, shape, scene_shape=src["shape"])
                p0 = 0
                for j in js:
                    nb = len(loaded[j][1])
                    dev_out[loaded[j][0]["key"]] = out[:, p0:p0 + nb]
                    p0 += nb
            if self.proposed_mask:
                dev_out["labelbinary"] = mask_creation.proposed_mask(dev_out["label_rgba"], dev_out["mag1c"]).to(torch.uint8)[:, None]
            host = {key: v.cpu().numpy() for key, v in dev_out.items()}
            for n, k in enumerate(ks):
                for e, _ in loaded:
                    items[k][e["key"]] = host[e["key"]][n]
                if self.proposed_mask:
                    items[k]["labelbinary"] = host["labelbinary"][n]
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()              # the pinned staging buffers may be released now
        return items

    def __getitem__(self, idx: int) -> Dict[str, np.ndarray]:
        folder = self.folders[idx]
        src = self._folder_sources(folder)
        chunk = plan_chunks([folder], [self.windows[idx]], {folder: src["shape"][0]}, {folder: src["row_bytes"]})[0]
        return self._cut(folder, [idx], chunk["band"])[0]

    # -------------------------------------------------------------------------------------------- writing
    def _geo(self, folder: str, key: str):
        src = self._folder_sources(folder)
        for e in src["entries"]:
            if e["key"] == key:
                return e["geo"]
        raise KeyError(key)

    def _write_item(self, idx: int, item: Dict[str, np.ndarray], folder_idx_path: str, overwrite: bool):
        folder = self.folders[idx]
        r, c = self.windows[idx][:2]
        for k, v in item.items():
            k_save = save_name(k, self.normalize_by_acquisition_date)
            path_save = os.path.join(folder_idx_path, f"{k_save}.tif")
            if not overwrite and os.path.exists(path_save):
                continue
            tags = io.window_geo_tags(self._geo(folder, "mag1c" if k == "labelbinary" else k), r, c)
            tags.update(io.gdal_metadata_tag({}, ["r", "g", "b", "a"] if k == "label_rgba" else [k_save]))
            if k != "labelbinary":
                tags[42113] = (2, ("0",))                                    # fill_value_default = 0 (:271); labelbinary: None
            io.write_tiff(path_save, v, blocksize=128, extra_tags=tags)

    def cache_item(self, idx: int, output_path: str, overwrite: bool = False):
        _no_gs(output_path)
        folder_idx_path = os.path.join(output_path, str(self.dataframe.index[idx]))
        os.makedirs(folder_idx_path, exist_ok=True)
        self._write_item(idx, self[idx], folder_idx_path, overwrite)

    def _missing(self, idx: int, folder_idx_path: str) -> bool:
        keys = [e["key"] for e in self._folder_sources(self.folders[idx])["entries"]] + (["labelbinary"] if self.proposed_mask else [])
        return any(not os.path.exists(os.path.join(folder_idx_path, f"{save_name(k, self.normalize_by_acquisition_date)}.tif")) for k in keys)

    def cache(self, output_path: str, dataframe_name: str, overwrite: bool = False):
        """sampling_dataset.py:358-386: ``{output_path}/{index}/{k_save}.tif`` for every row and product (tiled 128 x 128, the
        source's georeferencing moved to the window, band descriptions, GDAL_NODATA 0 except for labelbinary), then
        ``{dataframe_name}_sampled_data.csv`` (the table as sampled) and ``{dataframe_name}.csv`` (``folder`` = the sample
        folders, window columns = (0, 0, output_size)), both without the ``window`` column.  Files and tables that exist are
        left alone unless ``overwrite``.  Every source is looked up before anything is written (FileNotFoundError)."""
        _no_gs(output_path)
        for f in dict.fromkeys(self.folders):
            self._folder_sources(f)
        os.makedirs(output_path, exist_ok=True)
        out_dirs = [os.path.join(output_path, str(i)) for i in self.dataframe.index]
        todo = [i for i in range(len(self)) if overwrite or not os.path.isdir(out_dirs[i]) or self._missing(i, out_dirs[i])]
        shapes = {f: self._sources[f]["shape"][0] for f in self.folders}
        row_bytes = {f: self._sources[f]["row_bytes"] for f in self.folders}
        for chunk in plan_chunks([self.folders[i] for i in todo], [self.windows[i] for i in todo], shapes, row_bytes, self.memory_budget):
            rows = [todo[k] for k in chunk["rows"]]
            for i, item in zip(rows, self._cut(chunk["folder"], rows, chunk["band"])):
                os.makedirs(out_dirs[i], exist_ok=True)
                self._write_item(i, item, out_dirs[i], overwrite)
        columns_copy = [c for c in self.dataframe.columns if c != "window"]
        csv_original_path = os.path.join(output_path, f"{dataframe_name}_sampled_data.csv")
        if overwrite or not os.path.exists(csv_original_path):
            self.dataframe[columns_copy].to_csv(csv_original_path, index=True)
        dataframe_new = self.dataframe.copy()
        dataframe_new["folder"] = out_dirs
        dataframe_new["window_col_off"] = 0
        dataframe_new["window_row_off"] = 0
        dataframe_new["window_width"] = [w[3] for w in self.windows]
        dataframe_new["window_height"] = [w[2] for w in self.windows]
        csv_path = os.path.join(output_path, f"{dataframe_name}.csv")
        if overwrite or not os.path.exists(csv_path):
            dataframe_new[columns_copy].to_csv(csv_path, index=True)
