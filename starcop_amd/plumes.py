"""Plume catalogue: from a plume mask to a table of plumes.

``component_stats`` reduces value planes per labelled component in libstarcop_hip.so (include/starcop_hip.h: sc_component_stats);
``plume_table`` labels a mask (``mask_creation.connected_components``), reduces mag1c / probability / a second mask per
component in one call and returns one pandas row per plume; ``match_plumes`` counts detected, spurious and missed plumes between
a predicted and a labelled mask; ``write_plumes`` writes a table as CSV or GeoJSON.
"""
import json

import numpy as np
import torch

from . import _lib, metrics
from ._lib import check, ptr, stream
from .mask_creation import _planes, connected_components

MAX_PLANES = _lib.CSTATS_MAX_PLANES
COMPONENT_FIELDS = ("area", "row_min", "row_max", "col_min", "col_max", "sum_row", "sum_col", "first_pixel", "n_other")
PLANE_FIELDS = ("n_finite", "sum", "max", "min", "argmax")
_DTYPES = {"row_min": torch.int32, "row_max": torch.int32, "col_min": torch.int32, "col_max": torch.int32,
           "sum": torch.float64, "max": torch.float32, "min": torch.float32}


def _as_batch(t, what):
    if t.dim() not in (2, 3):
        raise ValueError(f"{what}: expected an (H, W) or (N, H, W) array, got {tuple(t.shape)}")
    return t[None] if t.dim() == 2 else t


def component_stats(labels, counts, planes=(), other=None, M=None):
    """Per-component statistics of a label image in one ``sc_component_stats`` call.

    ``labels``: device int32 (H, W) or (N, H, W); component k of image n is the set of pixels with value k, 1 <= k <= counts[n]
    (as ``connected_components`` returns them, but any label image will do: values need not be connected, values outside
    [0, counts[n]] are ignored).  ``counts``: device int32 (N,), or an int for one image.  ``planes``: up to 8 float32 tensors of
    the shape of ``labels``; views whose H x W planes are dense (a channel of an (N, C, H, W) tensor) are read in place.
    ``other``: an optional mask of that shape (uint8 is read in place).  ``M``: rows per image; the default reads ``counts`` back
    once and takes its maximum.

    Returns a dict of device tensors: ``area``, ``sum_row``, ``sum_col``, ``first_pixel``, ``n_other`` (int64), ``row_min``,
    ``row_max``, ``col_min``, ``col_max`` (int32, inclusive), all (N, M); and over the finite values of each plane ``n_finite``
    (int64), ``sum`` (float64), ``max``, ``min`` (float32), ``argmax`` (int64, the first raster index of the maximum; -1 and NaN
    where a component has no finite value), all (N, M, P).  Rows at or above counts[n] are zero.  Repeated calls, and an image
    alone or in a batch, give identical bits."""
    planes = list(planes)
    if len(planes) > MAX_PLANES:
        raise ValueError(f"component_stats: {len(planes)} planes, at most {MAX_PLANES} per call")
    if not isinstance(labels, torch.Tensor):
        raise ValueError("component_stats: labels must be a device tensor (plume_table takes numpy masks)")
    lab = _as_batch(labels, "component_stats: labels")
    N, H, W = lab.shape
    planes = [_as_batch(p, f"component_stats: plane {i}") for i, p in enumerate(planes)]
    for i, p in enumerate(planes):
        if tuple(p.shape) != (N, H, W):
            raise ValueError(f"component_stats: plane {i} has shape {tuple(p.shape)}, labels {(N, H, W)}")
    if other is not None:
        other = _as_batch(other, "component_stats: other")
        if tuple(other.shape) != (N, H, W):
            raise ValueError(f"component_stats: other has shape {tuple(other.shape)}, labels {(N, H, W)}")
    if isinstance(counts, int):
        counts = torch.tensor([counts], dtype=torch.int32, device=lab.device)
    counts = counts.reshape(-1)
    if counts.numel() != N:
        raise ValueError(f"component_stats: {counts.numel()} counts for {N} images")
    _lib.require_device(lab)
    lib = _lib.load()
    if lab.dtype != torch.int32:
        lab = lab.to(torch.int32)
    lab = lab.contiguous()
    counts = counts.to(device=lab.device, dtype=torch.int32).contiguous()
    if M is None:
        M = max(int(counts.max().item()), 0)
    M, P = int(M), len(planes)
    a = _lib.sc_cstats_args()
    a.labels, a.counts, a.N, a.H, a.W, a.M, a.P = lab.data_ptr(), counts.data_ptr(), N, H, W, M, P
    ops, oth = _operands(planes, other)          # holds the tensors the pointers belong to until the call is enqueued
    for i, (p, stride) in enumerate(ops):
        _lib.require_device(p)
        a.plane[i], a.plane_stride[i] = p.data_ptr(), stride
    if oth is not None:
        _lib.require_device(oth[0])
        a.other, a.other_stride = oth[0].data_ptr(), oth[1]
    out = {}
    for f in COMPONENT_FIELDS:
        out[f] = torch.empty((N, M), dtype=_DTYPES.get(f, torch.int64), device=lab.device)
    for f in PLANE_FIELDS:
        out[f] = torch.empty((N, M, P), dtype=_DTYPES.get(f, torch.int64), device=lab.device)
    for f, t in out.items():
        setattr(a, f, t.data_ptr() if t.numel() else None)
    wb = lib.sc_component_stats_workspace_bytes(N, H, W, M, P)          # 0 for bad dims: the call then raises with the message
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=lab.device)
    check(lib.sc_component_stats(a, ptr(work), wb, stream()))
    return out


def _operands(planes, other):
    """(N, H, W) planes and mask -> [(tensor, elements between images)], (tensor, bytes between images) or None: float32 / uint8
    views with dense H x W planes are used in place, anything else is converted or copied"""
    ops = [_planes(p if p.dtype == torch.float32 else p.float()) for p in planes]
    oth = None if other is None else _planes(other if other.dtype == torch.uint8 else (other != 0).to(torch.uint8))
    return ops, oth


def table_from_stats(stats, counts, width, plane_names=(), with_other=False, min_area=1, geotransform=None, pixel_area_m2=None):
    """The DataFrame of ``plume_table`` from host copies of the ``component_stats`` columns (numpy, (N, M) and (N, M, P)),
    ``counts`` (N,) and the image width (for the row / column of ``argmax``).  ``plane_names``: which of ``"mag1c"``, ``"prob"``
    the P planes are, in order.  No device involved."""
    import pandas as pd
    counts = np.asarray(counts).reshape(-1)
    area = np.asarray(stats["area"])
    N, M = area.shape
    item, k = np.nonzero((np.arange(M)[None, :] < np.minimum(counts, M)[:, None]) & (area >= max(int(min_area), 1)))
    a = area[item, k].astype(np.float64)
    cols = {"item": item, "plume_id": k + 1, "area_px": area[item, k]}
    for f in ("row_min", "row_max", "col_min", "col_max"):
        cols[f] = np.asarray(stats[f])[item, k]
    cols = {c: np.asarray(v, dtype=np.int64) for c, v in cols.items()}
    cols["centroid_row"] = np.asarray(stats["sum_row"])[item, k].astype(np.float64) / a
    cols["centroid_col"] = np.asarray(stats["sum_col"])[item, k].astype(np.float64) / a
    for q, name in enumerate(plane_names):
        nf = np.asarray(stats["n_finite"])[item, k, q]
        s = np.asarray(stats["sum"])[item, k, q].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(nf > 0, s / np.maximum(nf, 1), np.nan)
        mx = np.asarray(stats["max"])[item, k, q].astype(np.float64)
        if name == "mag1c":
            am = np.asarray(stats["argmax"])[item, k, q].astype(np.int64)
            cols.update(mag1c_sum=s, mag1c_mean=mean, mag1c_max=mx, mag1c_max_row=np.where(am >= 0, am // width, -1),
                        mag1c_max_col=np.where(am >= 0, am % width, -1))
            if pixel_area_m2 is not None:
                cols["ime_ppmm_m2"] = s * float(pixel_area_m2)
        elif name == "prob":
            cols.update(prob_mean=mean, prob_max=mx)
        else:
            raise ValueError(f"table_from_stats: unknown plane {name!r}")
    if with_other:
        cols["overlap_px"] = np.asarray(stats["n_other"])[item, k].astype(np.int64)
    if geotransform is not None:
        gt = [float(v) for v in np.asarray(geotransform, dtype=np.float64).ravel()]
        if len(gt) != 6:
            raise ValueError(f"plume_table: geotransform must have 6 numbers, got {len(gt)}")
        if gt[2] != 0.0 or gt[4] != 0.0:
            raise NotImplementedError(f"plume_table: rotated geotransform (terms {gt[2]}, {gt[4]}) is not supported")
        cols["x"] = gt[0] + (cols["centroid_col"] + 0.5) * gt[1]
        cols["y"] = gt[3] + (cols["centroid_row"] + 0.5) * gt[5]
    return pd.DataFrame(cols)


def _to_device(a, dev=None):
    if isinstance(a, np.ndarray):
        _lib.require_device()
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev if dev is not None else "cuda")
    return a


def plume_table(mask, mag1c=None, prob=None, label_mask=None, connectivity=2, min_area=1, geotransform=None, pixel_area_m2=None):
    """One row per plume of ``mask != 0``: an (H, W) or (N, H, W) mask, numpy or device.  Labels the mask on the device
    (``connectivity`` 1 or 2 as ``connected_components``), reduces every component in one ``sc_component_stats`` call and reads
    the rows back once.  Components of fewer than ``min_area`` pixels are dropped.  Columns:

    ``item`` (index of the image), ``plume_id`` (the component's label), ``area_px``, ``row_min``, ``row_max``, ``col_min``,
    ``col_max`` (inclusive), ``centroid_row``, ``centroid_col`` (float64 means of the pixel indices);
    with ``mag1c``: ``mag1c_sum``, ``mag1c_mean``, ``mag1c_max`` over the component's finite pixels, ``mag1c_max_row`` /
    ``mag1c_max_col`` of the first maximum in raster order, and with ``pixel_area_m2`` the integrated enhancement
    ``ime_ppmm_m2 = mag1c_sum * pixel_area_m2`` (ppm m x m2; turning it into a mass needs a constant the caller supplies);
    with ``prob``: ``prob_mean``, ``prob_max``;  with ``label_mask``: ``overlap_px``, the component's pixels inside it;
    with ``geotransform`` (GDAL 6-tuple, north up): ``x``, ``y`` of the centroid, pixel centres at +0.5."""
    shape = tuple(mask.shape)
    for name, p in (("mag1c", mag1c), ("prob", prob), ("label_mask", label_mask)):
        if p is not None and tuple(p.shape) != shape:
            raise ValueError(f"plume_table: {name} has shape {tuple(p.shape)}, the mask {shape}")
    if len(shape) not in (2, 3):
        raise ValueError(f"plume_table: expected an (H, W) or (N, H, W) mask, got {shape}")
    m = _to_device(mask)
    labels, counts = connected_components(m, connectivity=connectivity)
    names = [n for n, p in (("mag1c", mag1c), ("prob", prob)) if p is not None]
    planes = [_to_device(p, m.device) for p in (mag1c, prob) if p is not None]
    other = _to_device(label_mask, m.device) if label_mask is not None else None
    counts_h = np.array([counts]) if isinstance(counts, int) else counts.cpu().numpy()      # the one read-back of the counts
    st = component_stats(labels, counts, planes, other, M=max(int(counts_h.max()), 0))
    counts = counts_h
    host = _read_back(st)
    return table_from_stats(host, counts, shape[-1], names, other is not None, min_area, geotransform, pixel_area_m2)


def _read_back(st):
    """every column of a ``component_stats`` dict in ONE device-to-host copy -> numpy arrays"""
    N, M = st["area"].shape
    P = st["sum"].shape[-1]
    parts, layout = [], []
    for f in COMPONENT_FIELDS + PLANE_FIELDS:
        t = st[f]
        if t.dtype == torch.float64:
            t = t.view(torch.int64)
        elif t.dtype == torch.float32:
            t = t.view(torch.int32)
        parts.append(t.reshape(N, -1).to(torch.int64))
        layout.append((f, st[f].dtype, st[f].shape))
    flat = torch.cat(parts, 1).cpu().numpy() if M else np.zeros((N, 0), dtype=np.int64)
    out, at = {}, 0
    for f, dt, shp in layout:
        n = int(np.prod(shp[1:]))
        a = np.ascontiguousarray(flat[:, at:at + n]) if M else np.zeros((N, n), dtype=np.int64)
        at += n
        if dt == torch.float64:
            a = a.view(np.float64)
        elif dt == torch.float32:
            a = a.astype(np.int32).view(np.float32)
        elif dt == torch.int32:
            a = a.astype(np.int32)
        out[f] = a.reshape(tuple(shp))
    return out


def match_plumes(pred_mask, label_mask, connectivity=2, min_overlap_px=1, min_area=1):
    """Object-level detection score of a predicted against a labelled plume mask (same shape, numpy or device).  Both masks are
    labelled and each is reduced against the other: a predicted plume is a true positive when at least ``min_overlap_px`` of its
    pixels are labelled, a false positive otherwise; a labelled plume with fewer than ``min_overlap_px`` predicted pixels is a
    false negative.  Returns ``{"pred": table, "label": table, "tp", "fp", "fn", "precision", "recall"}``, the tables as
    ``plume_table`` gives them (with ``overlap_px``), the ratios from ``starcop_amd.metrics`` on [[0, fp], [fn, tp]]."""
    pred = plume_table(pred_mask, label_mask=label_mask, connectivity=connectivity, min_area=min_area)
    lab = plume_table(label_mask, label_mask=pred_mask, connectivity=connectivity, min_area=min_area)
    tp = int((pred["overlap_px"] >= min_overlap_px).sum())
    fp = len(pred) - tp
    fn = int((lab["overlap_px"] < min_overlap_px).sum())
    cm = torch.tensor([[0, fp], [fn, tp]], dtype=torch.float64)
    return {"pred": pred, "label": lab, "tp": tp, "fp": fp, "fn": fn,
            "precision": float(metrics.precision(cm)), "recall": float(metrics.recall(cm))}


def write_plumes(table, path):
    """``.csv``: the table as it is (no index column).  ``.geojson``: one Point feature per plume at (``x``, ``y``) -- the table
    must carry them, i.e. come from ``plume_table(..., geotransform=...)`` -- with every other column as a property and the
    bounding box as ``bbox_px`` = [row_min, col_min, row_max, col_max]."""
    path = str(path)
    if path.startswith("gs://"):
        raise NotImplementedError(f"{path}: writing to Google Cloud Storage is not supported")
    if path.endswith(".csv"):
        table.to_csv(path, index=False)
        return path
    if not path.endswith(".geojson"):
        raise ValueError(f"write_plumes: {path}: expected a .csv or .geojson path")
    if "x" not in table.columns or "y" not in table.columns:
        raise ValueError("write_plumes: a .geojson needs the x / y columns (plume_table(..., geotransform=...))")
    feats = []
    for row in table.to_dict("records"):
        props = {}
        for c, v in row.items():
            if c in ("x", "y"):
                continue
            v = v.item() if hasattr(v, "item") else v
            props[c] = None if isinstance(v, float) and not np.isfinite(v) else v
        props["bbox_px"] = [int(row["row_min"]), int(row["col_min"]), int(row["row_max"]), int(row["col_max"])]
        feats.append({"type": "Feature", "geometry": {"type": "Point", "coordinates": [float(row["x"]), float(row["y"])]},
                      "properties": props})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": feats}, f)
    return path
