"""Which 512 x 512 windows of a flight line become samples: mag1c window statistics and the no-plume window sampling.

Mirrors the reference's last dataset-production step:
  ``window_stats`` / ``stats_mag1c``   scripts/preprocessing/stats_mag1c.py:24-70: ten statistics of the valid, non-negative mag1c
                                       values (clipped at 10 000) of every 512 x 512 window at overlap 256 -> ``stats_mag1c.csv``
  ``mag1c_stats_dataframe``            starcop/data/sampling_dataset.py:112-179 ``permian_mag1c_stats_dataframe`` with the two tables
                                       passed in instead of read from a bucket
  ``windows_intersect``                ``rasterio.windows.intersect`` of two windows (third-party, absent: restated -- two windows
                                       intersect iff their extents overlap with positive area; sharing an edge is not enough)
  ``select_non_overlapping``           sampling_dataset.py:19-41
  ``sampling_no_plumes``               sampling_dataset.py:408-439, same draws (``np.random.seed``, one permutation per flight line)

The statistics run on the device (``sc_window_stats``: all windows of a scene in one call, the scene read in place); the table
logic is host code on pandas, as in the reference.  A window is a ``(row_off, col_off, height, width)`` tuple, or any object with
those four attributes.
"""
import os
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

from . import _lib
from ._lib import check, ptr, stream
from .datamodule import create_windows

STATS_COLUMNS = ["window_col_off", "window_row_off", "window_width", "window_height", "max", "min", "mean", "percentile01",
                 "percentile05", "median", "percentile95", "percentile99", "sum", "count"]

# sampling_dataset.py:109
TEST_DATES = ["2019-10-25", "2019-10-21", "2019-10-18"]
# sampling_dataset.py:135-150: windows of the Permian campaign that hold a plume without a label
PERMIAN_UNLABELED_PLUMES = [
    "ang20191018t183859_r2304_c0_w512_h512", "ang20191018t183859_r2560_c0_w512_h512", "ang20191021t190136_r4096_c0_w512_h512",
    "ang20191018t141549_r2560_c0_w512_h512", "ang20190926t172904_r512_c0_w512_h512", "ang20190926t184029_r6144_c256_w512_h512",
    "ang20190927t164322_r3328_c0_w512_h512", "ang20190923t185208_r4608_c0_w512_h512", "ang20190926t172904_r768_c0_w512_h512",
    "ang20190926t184029_r6400_c256_w512_h512", "ang20190927t153023_r8192_c0_w512_h512", "ang20191005t215301_r5120_c0_w512_h512",
    "ang20191007t195115_r768_c0_w512_h512", "ang20191012t162223_r3072_c0_w512_h512", "ang20191005t215301_r4864_c0_w512_h512"]


def __getattr__(name):
    # sampling_dataset.py:182-386 lives in window_dataset.py (which imports this module): resolved on first use
    if name == "WindowDataset":
        from .window_dataset import WindowDataset
        return WindowDataset
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _rchw(w) -> Tuple[int, int, int, int]:
    if hasattr(w, "row_off"):
        return int(w.row_off), int(w.col_off), int(w.height), int(w.width)
    r, c, h, wd = w
    return int(r), int(c), int(h), int(wd)


def windows_intersect(a, b) -> bool:
    """True iff the extents of the two windows overlap with positive area (``rasterio.windows.intersect`` for two windows)."""
    ar, ac, ah, aw = _rchw(a)
    br, bc, bh, bw = _rchw(b)
    return min(ar + ah, br + bh) > max(ar, br) and min(ac + aw, bc + bw) > max(ac, bc)


def window_stats(mag1c, fill_value: Optional[float] = None, window_size: Tuple[int, int] = (512, 512),
                 overlap: Tuple[int, int] = (256, 256), clip: float = 10_000., include_incomplete: bool = True,
                 windows: Optional[Sequence[Any]] = None) -> pd.DataFrame:
    """The table of stats_mag1c.py:41-63 for one scene: one row per window that holds at least one value of
    ``V = {min(v, clip) : v != fill_value, v >= 0}``, columns ``STATS_COLUMNS``.

    ``mag1c``: (H, W) or (1, H, W) float32 device tensor (any row stride, unit column stride) or numpy array (uploaded).
    ``fill_value`` None masks nothing.  max / min / percentiles are float32 and equal ``np.max`` / ``np.min`` /
    ``np.percentile`` / ``np.median`` of the float32 values (numpy >= 2.0 arithmetic); ``sum`` and ``mean`` are accumulated in
    float64, where the reference stores numpy's float32 pairwise results.

    Windows come from ``datamodule.create_windows`` unless given.  The reference calls ``georeader.slices.create_windows(reader,
    window_size=(512, 512), overlap=(256, 256))``; georeader is not part of the reference tree, so whether its default keeps the
    incomplete windows at the lower / right edge could not be checked: ``include_incomplete=True`` (edge windows trimmed to the
    scene) is this function's default, pass False to drop them.
    """
    if isinstance(mag1c, np.ndarray):
        mag1c = torch.from_numpy(np.ascontiguousarray(mag1c, dtype=np.float32)).to("cuda")
    _lib.require_device(mag1c)
    lib = _lib.load()
    if mag1c.dim() == 3 and mag1c.shape[0] == 1:
        mag1c = mag1c[0]
    if mag1c.dim() != 2 or mag1c.dtype != torch.float32:
        raise ValueError(f"window_stats: expected a (H, W) or (1, H, W) float32 scene, got {tuple(mag1c.shape)} {mag1c.dtype}")
    if mag1c.shape[1] > 1 and mag1c.stride(1) != 1 or mag1c.shape[0] > 1 and mag1c.stride(0) < mag1c.shape[1]:
        mag1c = mag1c.contiguous()
    H, W = mag1c.shape
    if windows is None:
        windows = create_windows((H, W), tuple(window_size), tuple(overlap), include_incomplete=include_incomplete)
    wins = np.array([_rchw(w) for w in windows], dtype=np.int32).reshape(-1, 4)
    n = wins.shape[0]
    if n == 0:
        return pd.DataFrame(columns=STATS_COLUMNS)
    dev = mag1c.device
    wins_d = torch.from_numpy(wins).to(dev)
    count = torch.empty((n,), dtype=torch.int64, device=dev)
    sum_mean = torch.empty((n, 2), dtype=torch.float64, device=dev)
    stats = torch.empty((n, 7), dtype=torch.float32, device=dev)
    wb = lib.sc_window_stats_workspace_bytes(n)
    work = torch.empty((wb,), dtype=torch.uint8, device=dev)
    a = _lib.sc_winstats_args()
    a.x, a.row_stride, a.H, a.W = mag1c.data_ptr(), (mag1c.stride(0) if H > 1 else W), H, W
    a.has_fill, a.fill = (0, 0.0) if fill_value is None else (1, float(fill_value))
    a.clip_max, a.n_win = float(clip), n
    a.windows, a.windows_host = wins_d.data_ptr(), wins.ctypes.data
    a.count, a.sum_mean, a.stats = count.data_ptr(), sum_mean.data_ptr(), stats.data_ptr()
    check(lib.sc_window_stats(a, ptr(work), wb, stream()))
    count, sum_mean, stats = count.cpu().numpy(), sum_mean.cpu().numpy(), stats.cpu().numpy()
    keep = count > 0                                    # stats_mag1c.py:50-51
    table = pd.DataFrame({
        "window_col_off": wins[:, 1].astype(np.int64), "window_row_off": wins[:, 0].astype(np.int64),
        "window_width": wins[:, 3].astype(np.int64), "window_height": wins[:, 2].astype(np.int64),
        "max": stats[:, 0], "min": stats[:, 1], "mean": sum_mean[:, 1], "percentile01": stats[:, 2], "percentile05": stats[:, 3],
        "median": stats[:, 4], "percentile95": stats[:, 5], "percentile99": stats[:, 6], "sum": sum_mean[:, 0], "count": count},
        columns=STATS_COLUMNS)
    return table[keep].reset_index(drop=True)


def _nodata(info) -> Optional[float]:
    nod = info.tags.get(42113)          # GDAL_NODATA
    if not nod:
        return None
    try:
        return float(str(nod[1][0]).strip().strip("\0"))
    except (ValueError, IndexError):
        return None


def stats_mag1c(folders: Sequence[str], filename_full_out: Optional[str] = None, overwrite: bool = True) -> pd.DataFrame:
    """stats_mag1c.py:24-70 for local folders: for every ``{folder}/mag1c.tif`` write ``{folder}/stats_mag1c.csv`` (the
    ``window_stats`` table plus the ``folder`` column after ``window_height``, as the reference orders it), or read the existing
    one when ``overwrite`` is False; returns the concatenation and writes it to ``filename_full_out`` if given.  The nodata value
    is the file's GDAL_NODATA tag; a file without one masks nothing."""
    from . import io_formats as io
    folders = [str(f) for f in folders]
    for p in folders + ([str(filename_full_out)] if filename_full_out is not None else []):
        if p.startswith("gs://"):
            raise NotImplementedError(f"{p}: reading from / writing to Google Cloud Storage is not supported")
    data_out = []
    for folder in folders:
        file_out = os.path.join(folder, "stats_mag1c.csv")
        if not overwrite and os.path.exists(file_out):
            data_out.append(pd.read_csv(file_out))
            continue
        path = os.path.join(folder, "mag1c.tif")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{folder}: missing mag1c.tif")
        info = io.tiff_info(path)
        scene = io.read_tiff(path, info=info)[0].astype(np.float32, copy=False)
        table = window_stats(scene, fill_value=_nodata(info))
        table.insert(4, "folder", folder)
        table.to_csv(file_out, index=False)
        data_out.append(table)
    data_out = pd.concat(data_out, ignore_index=True) if data_out else pd.DataFrame(columns=STATS_COLUMNS)
    if filename_full_out is not None:
        data_out.to_csv(filename_full_out, index=False)
    return data_out


def _overlaps_any(boxes: np.ndarray, others: np.ndarray) -> np.ndarray:
    """boxes (n, 4), others (m, 4), rows (row_off, col_off, height, width) -> bool (n,): overlaps one of ``others`` with
    positive area (the rule of ``windows_intersect``, all pairs at once)"""
    if others.shape[0] == 0:
        return np.zeros(boxes.shape[0], dtype=bool)
    top = np.maximum(boxes[:, None, 0], others[None, :, 0])
    left = np.maximum(boxes[:, None, 1], others[None, :, 1])
    bottom = np.minimum(boxes[:, None, 0] + boxes[:, None, 2], others[None, :, 0] + others[None, :, 2])
    right = np.minimum(boxes[:, None, 1] + boxes[:, None, 3], others[None, :, 1] + others[None, :, 3])
    return ((bottom > top) & (right > left)).any(axis=1)


def mag1c_stats_dataframe(mag1c_stats: pd.DataFrame, plumes_dataframe: pd.DataFrame,
                          unlabeled_plume_ids: Sequence[str] = PERMIAN_UNLABELED_PLUMES,
                          test_dates: Sequence[str] = TEST_DATES) -> pd.DataFrame:
    """The candidate windows of every flight line (what sampling_dataset.py:112-179 builds, with the two tables passed in).
    ``mag1c_stats``: the concatenated ``stats_mag1c`` table; ``plumes_dataframe``: the labelled plumes with ``folder`` and
    ``window`` columns.  Rows with a negative ``window_col_off`` are dropped and ``folder`` gets its trailing slash.  Added, in
    this order: ``name`` (last folder component), ``datetime`` (UTC, from ``ang%Y%m%dt%H%M%S``), ``date``, the ``id`` index
    ``{name}_r{row}_c{col}_w{w}_h{h}``, ``percentage_valids`` = count / (width * height), ``has_plume``, ``window`` =
    (row_off, col_off, height, width) and ``subset`` ("test" on ``test_dates``, else "train").  A window has a plume if its id is
    in ``unlabeled_plume_ids`` or if it intersects a labelled plume or a listed window of the same folder.  Listed ids that are
    not in the table are skipped (the reference's ``.loc`` assignment would create empty rows for them)."""
    table = mag1c_stats.loc[mag1c_stats["window_col_off"] >= 0].copy()
    folder = table["folder"].astype(str)
    table["folder"] = folder.where(folder.str.endswith("/"), folder + "/")
    table["name"] = table["folder"].str.rstrip("/").str.rsplit("/", n=1).str[-1]
    table["datetime"] = pd.to_datetime(table["name"], format="ang%Y%m%dt%H%M%S", utc=True)
    table["date"] = table["datetime"].dt.tz_localize(None).dt.normalize()
    geometry = table[["window_row_off", "window_col_off", "window_height", "window_width"]].to_numpy(dtype=np.int64)
    table.index = pd.Index([f"{name}_r{r}_c{c}_w{w}_h{h}" for name, (r, c, h, w) in zip(table["name"], geometry)], name="id")
    table["percentage_valids"] = table["count"] / (table["window_width"] * table["window_height"])
    listed = table.index.isin(list(unlabeled_plume_ids))
    has_plume = listed.copy()
    plume_folders = plumes_dataframe["folder"].to_numpy()
    plume_boxes = np.array([_rchw(w) for w in plumes_dataframe["window"]], dtype=np.int64).reshape(-1, 4)
    folders = table["folder"].to_numpy()
    for f in pd.unique(folders):
        rows = np.flatnonzero(folders == f)
        plumes = np.concatenate([plume_boxes[plume_folders == f], geometry[rows][listed[rows]]])
        has_plume[rows] |= _overlaps_any(geometry[rows], plumes)
    table["has_plume"] = has_plume
    table["window"] = [tuple(int(v) for v in g) for g in geometry]
    on_test_date = table["date"].dt.strftime("%Y-%m-%d").isin(list(test_dates))
    table["subset"] = np.where(on_test_date, "test", "train")
    return table


def select_non_overlapping(data: pd.DataFrame, n: int = 2, idxs: Optional[List[Any]] = None) -> List[Any]:
    """Greedy choice of mutually non-intersecting windows (the behaviour of sampling_dataset.py:19-41): walk ``data`` in its order
    and keep the index of every row whose ``window`` intersects none of the kept ones, until ``n`` are kept.  ``idxs``: indices of
    ``data`` that are already kept.  As in the reference, the first row of an empty selection is taken without looking at ``n``
    and the count is only checked after a later row, so ``n = 1`` returns two indices when the second row is free."""
    if n < 1:
        raise AssertionError(f"select_non_overlapping: n must be at least 1, got {n}")
    kept = list(idxs) if idxs is not None else []
    if len(kept) >= n:
        raise AssertionError(f"select_non_overlapping: {len(kept)} windows are already kept, n = {n} leaves nothing to select")
    boxes = [_rchw(data.at[i, "window"]) for i in kept]
    for index, window in zip(data.index, data["window"]):
        box = _rchw(window)
        if not kept:
            kept.append(index)
            boxes.append(box)
            continue
        if not any(windows_intersect(other, box) for other in boxes):
            kept.append(index)
            boxes.append(box)
        if len(kept) >= n:
            break
    return kept


def sampling_no_plumes(no_plumes: pd.DataFrame, n_hard: int, n_random: int, percentage_valids: float = .8, seed: int = 42) -> pd.DataFrame:
    """The no-plume samples of every flight line (the behaviour of sampling_dataset.py:408-439).  Per ``name``, in ``unique()``
    order, among the windows with at least ``percentage_valids`` valid pixels: the ``n_hard`` non-overlapping ones with the
    highest mean mag1c (the confounders, ``difficulty`` "hard"), then up to ``n_random`` more that overlap none of them, taken in
    the order of one ``np.random.permutation`` of the same rows ("random").  ``np.random.seed(seed)`` is set once, so the draws
    are the reference's.  Also adds ``qplume`` 0, ``candidate_id`` "" and ``label_path`` ""."""
    np.random.seed(seed)
    chosen, difficulty = [], []
    for line in no_plumes["name"].unique():
        usable = no_plumes[(no_plumes["name"] == line) & (no_plumes["percentage_valids"] >= percentage_valids)]
        ranked = usable.sort_values(by="mean", ascending=False)
        hard = select_non_overlapping(ranked, n=n_hard)
        shuffled = ranked.iloc[np.random.permutation(len(ranked))]
        both = select_non_overlapping(shuffled, n=n_hard + n_random, idxs=hard)
        chosen += both
        difficulty += ["hard"] * len(hard) + ["random"] * (len(both) - len(hard))
    selected = no_plumes.loc[chosen].copy()
    selected["difficulty"] = difficulty
    selected["qplume"] = 0
    selected["candidate_id"] = ""
    selected["label_path"] = ""
    return selected
