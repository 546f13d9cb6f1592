"""Plume catalogue: from a plume mask to a table of plumes.

``component_stats`` reduces value planes per labelled component in libstarcop_hip.so (include/starcop_hip.h: sc_component_stats);
``plume_table`` labels a mask (``mask_creation.connected_components``), reduces mag1c / probability / a second mask per
component in one call and returns one pandas row per plume; ``match_plumes`` counts detected, spurious and missed plumes between
a predicted and a labelled mask; ``component_outlines`` traces the polygon rings of every component (sc_component_outlines),
``plume_outlines`` turns a mask into closed (x, y) rings per plume; ``component_radial`` (sc_component_radial) gives the radial
profile, extent and second moments of every component, from which ``plume_table(quantify=...)`` / ``fetch_profiles`` derive shape,
mass and emission rates (starcop_amd/quantify.py); ``write_plumes`` writes a table as CSV or GeoJSON (Points, or
Polygons with the outlines).  The other way: ``read_plumes`` reads such a GeoJSON back, ``rasterize_polygons`` burns polygons
into a label image on the raster grid (sc_rasterize_polygons), ``match_plumes_polygons`` scores a mask against polygons.
"""
import json

import numpy as np
import torch

from . import _lib, metrics, stacks
from ._lib import check, stream
from .mask_creation import connected_components

MAX_PLANES = _lib.CSTATS_MAX_PLANES
COMPONENT_FIELDS = ("area", "row_min", "row_max", "col_min", "col_max", "sum_row", "sum_col", "first_pixel", "n_other")
PLANE_FIELDS = ("n_finite", "sum", "max", "min", "argmax")
_DTYPES = {"row_min": torch.int32, "row_max": torch.int32, "col_min": torch.int32, "col_max": torch.int32,
           "sum": torch.float64, "max": torch.float32, "min": torch.float32}
_COLUMNS = [(f, _DTYPES.get(f, torch.int64), f in PLANE_FIELDS) for f in COMPONENT_FIELDS + PLANE_FIELDS]      # (field, dtype, per plane)


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
    who = "component_stats"
    planes = list(planes)
    if len(planes) > MAX_PLANES:
        raise ValueError(f"{who}: {len(planes)} planes, at most {MAX_PLANES} per call")
    if not isinstance(labels, torch.Tensor):
        raise ValueError("component_stats: labels must be a device tensor (plume_table takes numpy masks)")
    lab = stacks.stack3(labels, "component_stats: labels")[0]
    shape = N, H, W = lab.shape
    planes = [stacks.stack_like(p, shape, f"component_stats: plane {i}") for i, p in enumerate(planes)]
    if other is not None:
        other = stacks.stack_like(other, shape, "component_stats: other")
    counts = stacks.counts_i32(counts, N, lab.device, who)
    lab = stacks.labels_i32(lab)
    lib = _lib.load()
    if M is None:
        M = max(int(counts.max().item()), 0)
    M, P = int(M), len(planes)
    a = _lib.sc_cstats_args()
    a.labels, a.counts, a.N, a.H, a.W, a.M, a.P = lab.data_ptr(), counts.data_ptr(), N, H, W, M, P
    ops = [stacks.plane_operand(p, torch.float32) for p in planes]      # holds the tensors the pointers belong to until the call is enqueued
    for i, (p, stride) in enumerate(ops):
        _lib.require_device(p)
        a.plane[i], a.plane_stride[i] = p.data_ptr(), stride
    if other is not None:
        other, a.other_stride = stacks.plane_operand(other, torch.uint8)
        _lib.require_device(other)
        a.other = other.data_ptr()
    out = stacks.output_columns(a, [(f, dt, (N, M, P) if per_plane else (N, M)) for f, dt, per_plane in _COLUMNS], lab.device)
    wb = lib.sc_component_stats_workspace_bytes(N, H, W, M, P)          # 0 for bad dims: the call then raises with the message
    stacks.call_with_workspace(lib.sc_component_stats, a, wb, lab.device)
    return out


MAX_QUANTILES = _lib.CQUANT_MAX_Q
BACKGROUND_STATS = ("mean", "median")
MAD_TO_SIGMA = 1.4826          # sigma of a normal distribution = 1.4826 * its median absolute deviation


def quantile_fractions(q, who):
    """the ``q`` of ``component_quantiles`` -> the float32 fractions the kernel takes: ``float32(q_j) / float32(100)``, the quantile
    numpy >= 2.0 forms for float32 data, and -1 for ``"median"``.  ValueError for an empty ``q``, more than 8 entries, a number
    outside [0, 100] or NaN, or any other string.  No device involved."""
    if isinstance(q, (str, bytes)) or not hasattr(q, "__len__"):
        raise ValueError(f"{who}: q {q!r} must be a sequence of percentages in [0, 100] and / or \"median\"")
    if not 1 <= len(q) <= MAX_QUANTILES:
        raise ValueError(f"{who}: {len(q)} quantiles, 1 to {MAX_QUANTILES} per call")
    out = []
    for v in q:
        if isinstance(v, str):
            if v != "median":
                raise ValueError(f"{who}: q entry {v!r} (a percentage in [0, 100] or \"median\")")
            out.append(np.float32(-1.0))
            continue
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: q entry {v!r} (a percentage in [0, 100] or \"median\")") from None
        if not 0.0 <= f <= 100.0:                      # NaN fails both comparisons
            raise ValueError(f"{who}: q entry {v!r} is outside [0, 100]")
        out.append(np.float32(f) / np.float32(100))
    return out


def quantile_names(q, prefix="mag1c"):
    """column names of the ``percentiles=`` of ``plume_table``: ``f"{prefix}_p{q:g}"``, ``f"{prefix}_median"`` for ``"median"``"""
    return [f"{prefix}_median" if isinstance(v, str) else f"{prefix}_p{float(v):g}" for v in q]


def component_quantiles(labels, counts, plane, q=("median",), center=None, M=None):
    """Exact order statistics of one plane per labelled component in one ``sc_component_quantiles`` call.

    ``labels``, ``counts``, ``M`` as ``component_stats`` takes them (they need not come from that call: the ring labels of
    ``background_rings`` are an ordinary input).  ``plane``: one float32 tensor of the shape of ``labels``, read in place where its
    H x W planes are dense.  ``q``: 1 to 8 entries, each a percentage in [0, 100] or the string ``"median"``.  ``center``: an optional
    device float32 (N, M); with it the value of a pixel of component k is ``|v - center[n, k-1]|`` (rounded once to float32), which
    makes the median of the result the median absolute deviation about ``center``.  A bad ``q``, a shape mismatch or a non-tensor
    ``labels`` is a ValueError before the device is required.

    Over the pixels of each component whose value is finite (NaN and +-inf are dropped, and every pixel of a row whose centre is
    not finite) returns ``{"n_finite": (N, M) int64, "quantile": (N, M, Q) float32}`` on the device: what ``np.percentile(values,
    q_j)`` and ``np.median(values)`` of numpy >= 2.0 give for the float32 values, bit for bit (the sign of a zero aside); NaN and
    0 for a component without such a pixel and for rows at or above ``counts[n]``.  Exact selection with integer atomics only:
    repeated calls, and an image alone or in a batch, give identical bytes."""
    who = "component_quantiles"
    fr = quantile_fractions(q, who)
    if not isinstance(labels, torch.Tensor) or not isinstance(plane, torch.Tensor):
        raise ValueError(f"{who}: labels and plane must be device tensors (plume_table takes numpy masks)")
    lab = stacks.stack3(labels, "component_quantiles: labels")[0]
    shape = N, H, W = lab.shape
    pl = stacks.stack_like(plane, shape, "component_quantiles: plane")
    counts = stacks.counts_i32(counts, N, lab.device, who)
    if center is not None:
        if not isinstance(center, torch.Tensor) or center.dim() != 2 or center.shape[0] != N or center.dtype != torch.float32:
            raise ValueError(f"{who}: center must be a float32 tensor of shape ({N}, M)")
        if M is not None and center.shape[1] != int(M):
            raise ValueError(f"{who}: center has shape {tuple(center.shape)}, expected {(N, int(M))}")
        M = center.shape[1]
    lab = stacks.labels_i32(lab)
    lib = _lib.load()
    if M is None:
        M = max(int(counts.max().item()), 0)
    M, Q = int(M), len(fr)
    op, stride = stacks.plane_operand(pl, torch.float32)      # holds the tensor the pointer belongs to until the call is enqueued
    _lib.require_device(op)
    a = _lib.sc_cquant_args()
    a.labels, a.counts, a.N, a.H, a.W, a.M, a.Q = lab.data_ptr(), counts.data_ptr(), N, H, W, M, Q
    a.plane, a.plane_stride = op.data_ptr(), stride
    if center is not None:
        center = center.to(lab.device).contiguous()
        _lib.require_device(center)
        a.center = center.data_ptr() if center.numel() else None
    for j, f in enumerate(fr):
        a.q[j] = float(f)
    out = stacks.output_columns(a, [("n_finite", torch.int64, (N, M)), ("quantile", torch.float32, (N, M, Q))], lab.device)
    wb = lib.sc_component_quantiles_workspace_bytes(N, H, W, M, Q)      # 0 for bad dims: the call then raises with the message
    stacks.call_with_workspace(lib.sc_component_quantiles, a, wb, lab.device)
    return out


def component_median_mad(labels, counts, plane, M=None):
    """Median and median absolute deviation of one plane per labelled component: ``component_quantiles`` twice, the second call
    with the medians of the first as ``center``; nothing is read back in between (with ``M`` given, nothing at all).  Returns
    ``{"n_finite": (N, M) int64, "median": (N, M) float32, "mad": (N, M) float32}`` on the device: ``np.median(v)`` and
    ``np.median(np.abs(v - np.median(v)))`` over the finite values v of each component, NaN where there is none.  (A component
    whose values overflow float32 in ``v - median`` loses those pixels from the MAD, as numpy's ``isfinite`` filter would.)"""
    first = component_quantiles(labels, counts, plane, ("median",), M=M)
    med = first["quantile"][..., 0].contiguous()
    second = component_quantiles(labels, counts, plane, ("median",), center=med, M=med.shape[1])
    return {"n_finite": first["n_finite"], "median": med, "mad": second["quantile"][..., 0].contiguous()}


RADIAL_FIELDS = ("bin_count", "bin_sum", "d2_max", "sum_rr", "sum_cc", "sum_rc")
MAX_RADII = _lib.CRADIAL_MAX_BINS


def origins_from_argmax(stats, width, plane=0):
    """The origin of every plume at the first maximum of one plane: the ``argmax`` column of a ``component_stats`` dict (the raster
    index r * width + c) -> device int32 (N, M, 2) of (row, col), (-1, -1) where ``argmax`` is -1 (no finite value, or no such
    component), which ``component_radial`` skips.  Device arithmetic only: nothing is read back."""
    am = stats["argmax"]
    if am.dim() != 3 or not 0 <= int(plane) < am.shape[-1]:
        raise ValueError(f"origins_from_argmax: plane {plane!r} of an argmax column of shape {tuple(am.shape)}")
    width = int(width)
    if width <= 0:
        raise ValueError(f"origins_from_argmax: width {width!r}")
    am = am[..., int(plane)]
    ok = am >= 0
    row = torch.where(ok, torch.div(am, width, rounding_mode="floor"), -1)
    col = torch.where(ok, am - torch.div(am, width, rounding_mode="floor") * width, -1)
    return torch.stack([row, col], -1).to(torch.int32)


def component_radial(labels, counts, stats, origins, radii_px, plane, M=None):
    """Radial profile, extent and second moments of every component in one ``sc_component_radial`` call.

    ``labels``, ``counts``, ``M`` as ``component_stats`` takes them; ``stats``: the dict that call returned for the same labels (its
    ``row_min`` .. ``col_max`` columns are the boxes that are walked; they are not recomputed); ``origins``: device int32 (N, M, 2)
    of (row, col), a negative row skips the plume (``origins_from_argmax``); ``plane``: one float32 tensor of the shape of
    ``labels``, read in place where its H x W planes are dense.  ``radii_px``: 1 to 64 positive radii in pixels; the squared bin
    edges are ``edge2[j] = floor(radii_px[j]^2)`` in float64 with no epsilon (as ``morphology.dilate`` and ``background_rings`` take
    a radius), which must increase strictly and stay below 2^31 - 2: a ValueError otherwise, before the device is used.

    With ``d2 = (r - r0)^2 + (c - c0)^2`` of a pixel from its component's origin, in integers, returns a dict of device tensors:
    ``bin_count`` (int64) and ``bin_sum`` (float64), (N, M, K+1), over the component's pixels with a finite plane value -- bin j is the
    smallest j with ``d2 <= edge2[j]``, bin K lies beyond the last edge; ``d2_max`` (int64, (N, M)), over all its pixels, -1 for a
    component without pixels or a skipped one; ``sum_rr``, ``sum_cc``, ``sum_rc`` (int64, (N, M)), the sums of r^2, c^2 and r c over all
    its pixels.  Rows at or above counts[n], rows without pixels and skipped rows are zero.  Repeated calls, and an image alone or
    in a batch, give identical bits."""
    from .quantify import squared_edges
    who = "component_radial"
    edges = squared_edges(radii_px, who, _lib.EDT_FAR - 1)
    if not isinstance(labels, torch.Tensor) or not isinstance(plane, torch.Tensor) or not isinstance(origins, torch.Tensor):
        raise ValueError(f"{who}: labels, origins and plane must be device tensors (plume_table takes numpy masks)")
    lab = stacks.stack3(labels, "component_radial: labels")[0]
    shape = N, H, W = lab.shape
    pl = stacks.stack_like(plane, shape, "component_radial: plane")
    if H >_lib.CRADIAL_MAX_SIDE or W > _lib.CRADIAL_MAX_SIDE:
        raise ValueError(f"{who}: image of {H} x {W}; a side may have at most {_lib.CRADIAL_MAX_SIDE} pixels")
    counts = stacks.counts_i32(counts, N, lab.device, who)
    boxes =[stats[f] for f in ("row_min", "row_max", "col_min", "col_max")]
    if M is None:
        M = boxes[0].shape[-1]
    M, K = int(M), len(edges)
    for f, t in zip(("row_min", "row_max", "col_min", "col_max"), boxes):
        if tuple(t.shape) != (N, M) or t.dtype != torch.int32:
            raise ValueError(f"{who}: stats[{f!r}] is {t.dtype} {tuple(t.shape)}, expected int32 {(N, M)}")
    if tuple(origins.shape) != (N, M, 2) or origins.dtype != torch.int32:
        raise ValueError(f"{who}: origins is {origins.dtype} {tuple(origins.shape)}, expected int32 {(N, M, 2)}")
    for t in [lab, pl, origins] + boxes:
        if not t.is_cuda:
            raise ValueError(f"{who}: labels, stats, origins and plane must be device tensors, got one on {t.device}")
    lab = stacks.labels_i32(lab)
    lib = _lib.load()
    boxes = [t.contiguous() for t in boxes]
    origins = origins.contiguous()
    op, stride = stacks.plane_operand(pl, torch.float32)      # holds the tensor the pointer belongs to until the call is enqueued
    a = _lib.sc_cradial_args()
    a.labels, a.counts, a.N, a.H, a.W, a.M, a.K = lab.data_ptr(), counts.data_ptr(), N, H, W, M, K
    a.row_min, a.row_max, a.col_min, a.col_max = (t.data_ptr() if t.numel() else None for t in boxes)
    a.origin = origins.data_ptr() if origins.numel() else None
    a.plane, a.plane_stride = op.data_ptr(), stride
    for j, e in enumerate(edges):
        a.edge2[j] = e
    out = stacks.output_columns(a, [("bin_count", torch.int64, (N, M, K + 1)), ("bin_sum", torch.float64, (N, M, K + 1))]
                                + [(f, torch.int64, (N, M)) for f in RADIAL_FIELDS[2:]], lab.device)
    wb = lib.sc_component_radial_workspace_bytes(N, H, W, M, K)         # 0 for bad dims: the call then raises with the message
    stacks.call_with_workspace(lib.sc_component_radial, a, wb, lab.device)
    return out


def table_from_stats(stats, counts, width, plane_names=(), with_other=False, min_area=1, geotransform=None, pixel_area_m2=None,
                     ring_stats=None, quantify=None, ring_quantiles=None, plume_quantiles=None):
    """The DataFrame of ``plume_table`` from host copies of the ``component_stats`` columns (numpy, (N, M) and (N, M, P)),
    ``counts`` (N,) and the image width (for the row / column of ``argmax``).  ``plane_names``: which of ``"mag1c"``, ``"prob"``
    the P planes are, in order.  ``ring_stats``: the same columns reduced over the background-ring labels (``background_rings``)
    with mag1c as plane 0, for the ring columns of ``plume_table``; it needs ``"mag1c"`` among the planes.  ``quantify``: for the
    quantification columns of ``plume_table``, a dict with ``settings`` (the checked ``quantify=`` dict), ``radii_m``,
    ``pixel_size_m`` and ``radial`` (host copies of the ``component_radial`` columns and ``origin``, (N, M, ..)); the per-plume
    curves of ``fetch_profiles`` are left under its key ``curves``.  It needs mag1c as well.  ``ring_quantiles``: for
    ``background_stat="median"``, host copies of the ``component_median_mad`` columns of mag1c over the ring labels (``median``,
    ``mad``, (N, M)); it needs ``ring_stats``, and the median then is the background that is subtracted.  ``plume_quantiles``: for
    ``percentiles=``, a dict with ``q`` (the sequence) and ``quantile`` (the host copy of that ``component_quantiles`` column of
    mag1c over the plume labels, (N, M, Q)); it needs mag1c.  No device involved."""
    import pandas as pd
    if ring_stats is not None and "mag1c" not in plane_names:
        raise ValueError("table_from_stats: ring_stats needs the mag1c plane")
    if ring_quantiles is not None and ring_stats is None:
        raise ValueError("table_from_stats: ring_quantiles needs ring_stats")
    if plume_quantiles is not None and "mag1c" not in plane_names:
        raise ValueError("table_from_stats: plume_quantiles needs the mag1c plane")
    if quantify is not None and "mag1c" not in plane_names:
        raise ValueError("table_from_stats: quantify needs the mag1c plane")
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
            if ring_stats is not None:
                bg_n = np.asarray(ring_stats["n_finite"])[item, k, 0].astype(np.int64)
                bg_s = np.asarray(ring_stats["sum"])[item, k, 0].astype(np.float64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    bg_mean = np.where(bg_n > 0, bg_s / np.maximum(bg_n, 1), np.nan)
                bg = bg_mean
                if ring_quantiles is not None:             # float32 results, kept as float64 columns
                    bg = np.asarray(ring_quantiles["median"])[item, k].astype(np.float64)
                cols.update(bg_px=bg_n, mag1c_bg_mean=bg_mean, mag1c_sum_bgsub=s - bg * nf.astype(np.float64))
                if pixel_area_m2 is not None:
                    cols["ime_bgsub_ppmm_m2"] = cols["mag1c_sum_bgsub"] * float(pixel_area_m2)
                if ring_quantiles is not None:
                    mad = np.asarray(ring_quantiles["mad"])[item, k].astype(np.float64)
                    noise = MAD_TO_SIGMA * mad * np.sqrt(nf.astype(np.float64))      # of the sum over n pixels of independent noise
                    cols.update(mag1c_bg_median=bg, mag1c_bg_mad=mad, mag1c_bg_sigma=MAD_TO_SIGMA * mad)
                    if pixel_area_m2 is not None:
                        cols["ime_sigma_ppmm_m2"] = noise * float(pixel_area_m2)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        cols["snr"] = np.where(noise > 0, cols["mag1c_sum_bgsub"] / np.where(noise > 0, noise, 1.0), np.nan)
            if plume_quantiles is not None:
                pq = np.asarray(plume_quantiles["quantile"])
                for j, cname in enumerate(quantile_names(plume_quantiles["q"])):
                    cols[cname] = pq[item, k, j].astype(np.float64)
        elif name == "prob":
            cols.update(prob_mean=mean, prob_max=mx)
        else:
            raise ValueError(f"table_from_stats: unknown plane {name!r}")
    if with_other:
        cols["overlap_px"] = np.asarray(stats["n_other"])[item, k].astype(np.int64)
    if geotransform is not None:
        gt = _gt6(geotransform, "plume_table")
        cols["x"] = gt[0] + (cols["centroid_col"] + 0.5) * gt[1]
        cols["y"] = gt[3] + (cols["centroid_row"] + 0.5) * gt[5]
    if quantify is not None:
        from .quantify import quantify_columns
        q = list(plane_names).index("mag1c")
        settings, rad = quantify["settings"], quantify["radial"]
        wind = np.asarray(settings["wind_speed_m_s"], dtype=np.float64)
        if wind.ndim:                                 # one per plume, in the order of the rows before the min_area filter
            rank = np.concatenate([[0], np.cumsum(np.minimum(np.maximum(counts, 0), M))])[item] + k
            wind = wind.reshape(-1)[rank]
        qcols, curves = quantify_columns(
            settings, quantify["radii_m"], quantify["pixel_size_m"], area[item, k], np.asarray(stats["sum_row"])[item, k],
            np.asarray(stats["sum_col"])[item, k], cols["mag1c_sum"], np.asarray(stats["n_finite"])[item, k, q],
            {f: np.asarray(v)[item, k] for f, v in rad.items()},
            None if ring_stats is None else cols["mag1c_bg_mean" if ring_quantiles is None else "mag1c_bg_median"],
            wind if wind.ndim else None)
        cols.update(qcols)
        quantify["curves"] = curves
    return pd.DataFrame(cols)


def _ring_caps(ring_px, gap_px, who):
    """(floor(ring_px^2), floor(gap_px^2)), both radii >= 0, the ring at least a pixel wide and within the int32 range of d2"""
    ring, gap = float(ring_px), float(gap_px)
    if not ring >= 1.0 or not gap >= 0.0 or not gap < ring or not ring * ring < _lib.EDT_FAR - 1:
        raise ValueError(f"{who}: ring_px {ring_px!r} and gap_px {gap_px!r}: need 0 <= gap_px < ring_px, 1 <= ring_px < 2^15.5")
    return int(np.floor(ring * ring)), int(np.floor(gap * gap))


def _rings(lab, ring2, gap2):
    """``background_rings`` of a contiguous device int32 (N, H, W) label image and the two squared radii"""
    from . import morphology as mo
    _, d2, (near,) = mo._nearest((lab != 0).to(torch.uint8), False, ring2, dist2=True, planes=[lab])
    return torch.where((lab == 0) & (d2 > gap2) & (d2 <= ring2), near, 0)


def background_rings(labels, ring_px, gap_px=0.0):
    """The local-background ring of every plume of an integer label image (0 the background; (H, W) or (N, H, W), numpy or
    device) -> int32 ring labels: pixel p gets k when ``labels[p] == 0``, its squared distance d2 to the nearest labelled pixel
    has ``floor(gap_px^2) < d2 <= floor(ring_px^2)``, and that nearest pixel (``morphology.nearest_index``'s tie rule) carries k;
    every other pixel 0.  With several plumes each ring pixel belongs to the nearest one, so rings never overlap.  One
    ``sc_edt_nearest`` call (squared distance and the gathered label plane) and one select."""
    who = "background_rings"
    ring2, gap2 = _ring_caps(ring_px, gap_px, who)
    lab, single, host = stacks.device_labels(labels, who, integers=True)
    return stacks.finish(_rings(lab, ring2, gap2), single, host)


def plume_table(mask, mag1c=None, prob=None, label_mask=None, connectivity=2, min_area=1, geotransform=None, pixel_area_m2=None,
                background_ring_px=None, background_gap_px=0.0, quantify=None, background_stat="mean", percentiles=None):
    """One row per plume of ``mask != 0``: an (H, W) or (N, H, W) mask, numpy or device.  Labels the mask on the device
    (``connectivity`` 1 or 2 as ``connected_components``), reduces every component in one ``sc_component_stats`` call and reads
    back twice whatever the options: the component counts, which size the rows, and then every column of every option below in one
    copy (``stacks.read_back``).  Components of fewer than ``min_area`` pixels are dropped.  Columns:

    ``item`` (index of the image), ``plume_id`` (the component's label), ``area_px``, ``row_min``, ``row_max``, ``col_min``,
    ``col_max`` (inclusive), ``centroid_row``, ``centroid_col`` (float64 means of the pixel indices);
    with ``mag1c``: ``mag1c_sum``, ``mag1c_mean``, ``mag1c_max`` over the component's finite pixels, ``mag1c_max_row`` /
    ``mag1c_max_col`` of the first maximum in raster order, and with ``pixel_area_m2`` the integrated enhancement
    ``ime_ppmm_m2 = mag1c_sum * pixel_area_m2`` (ppm m x m2; ``quantify`` below turns it into a mass and emission rates);
    with ``prob``: ``prob_mean``, ``prob_max``;  with ``label_mask``: ``overlap_px``, the component's pixels inside it;
    with ``geotransform`` (GDAL 6-tuple, north up): ``x``, ``y`` of the centroid, pixel centres at +0.5;
    with ``background_ring_px`` (needs ``mag1c``): the local background of every plume, taken over its ring of
    ``background_rings(labels, background_ring_px, background_gap_px)`` in one more ``component_stats`` call: ``bg_px`` (ring pixels
    with finite mag1c), ``mag1c_bg_mean`` (NaN when ``bg_px`` is 0), ``mag1c_sum_bgsub = mag1c_sum - mag1c_bg_mean * n`` with n the
    plume's finite pixels, and with ``pixel_area_m2`` ``ime_bgsub_ppmm_m2``.  None leaves the table as it is without.

    ``quantify`` (needs ``mag1c`` and ``pixel_area_m2``, square pixels of ``pixel_size_m = sqrt(pixel_area_m2)``; a geotransform
    with ``|gt1| != |gt5|`` is a ValueError) adds shape, mass and emission rates from one ``component_radial`` call, read back with
    the other columns.  A dict with the keys (anything else is a ValueError):
    ``wind_speed_m_s`` (required): the EFFECTIVE wind speed, used as given -- a number, or one per plume; no U10 model is applied;
    ``radii_m`` (up to 64 increasing radii) or ``max_fetch_m`` (default 150 m, the AVIRIS-NG survey's choice): without ``radii_m`` the
    circles are ``r_j = j * pixel_size_m`` for j = 1 .. min(64, floor(max_fetch_m / pixel_size_m)); no radius at all is a ValueError;
    ``origin``: ``"max"`` (default), the plume's first mag1c maximum (``mag1c_max_row`` / ``mag1c_max_col``), or an (R, 2) array of
    (row, col) -- floats are floored -- or, with ``origin_xy=True`` and a geotransform, of (x, y); a row that is negative or not
    finite leaves that plume without the columns that need an origin (NaN);
    ``min_fetch_m`` (default 0), ``temperature_k`` / ``pressure_pa`` (defaults 288.15 K, 101325 Pa) or ``kg_per_ppmm_m2`` in their
    place (``quantify.kg_per_ppmm_m2``).
    Arrays with one entry per plume (``origin``, ``wind_speed_m_s``) are aligned with the rows the table has BEFORE the ``min_area``
    filter, i.e. with ``min_area=1``: image after image, ``plume_id`` ascending, R = the number of components of all images.
    Columns: ``origin_row``, ``origin_col``; ``fetch_max_m``, the distance of the farthest pixel from the origin;
    ``major_axis_m``, ``minor_axis_m``, ``orientation_rad`` (``quantify.shape_from_moments``); ``ime_kg = mag1c_sum * pixel_area_m2 *
    kg_per_ppmm_m2``; ``q_sqrt_area_kg_h``, ``q_fetch_kg_h``, ``q_fetch_std_kg_h``, ``q_fetch_n`` (``quantify.emission_rates`` on the
    cumulative profile inside the circles).  With ``background_ring_px`` the profile and ``ime_kg`` are taken above
    ``mag1c_bg_mean``, and a plume whose ``bg_px`` is 0 gets NaN rates.  None leaves columns and bytes as they are without.

    ``background_stat``: ``"mean"`` (default: every column and byte as above) or ``"median"``, which needs ``background_ring_px`` (a
    ValueError otherwise, as is any other string).  The ring is reduced once more, by ``component_median_mad`` (exact order statistics
    of the ring pixels with finite mag1c), and the background that ``mag1c_sum_bgsub``, ``ime_bgsub_ppmm_m2`` and ``quantify``
    (``ime_kg``, the fetch profile, the NaN rule for a plume without ring pixels) subtract is the ring MEDIAN; ``bg_px`` and
    ``mag1c_bg_mean`` stay as they are.  Added columns: ``mag1c_bg_median``, ``mag1c_bg_mad`` (the median of ``|v - median|`` over the
    ring; both float32 results kept as float64), ``mag1c_bg_sigma = 1.4826 * mag1c_bg_mad`` (the standard deviation of a normal
    distribution with that MAD), with ``pixel_area_m2`` ``ime_sigma_ppmm_m2 = mag1c_bg_sigma * sqrt(n) * pixel_area_m2``, and ``snr =
    mag1c_sum_bgsub / (mag1c_bg_sigma * sqrt(n))``, n the plume's finite pixels.  Both ASSUME that the noise of the n pixels is
    uncorrelated and as large as in the ring; mag1c noise is spatially correlated, so they flatter the plume.  ``snr`` is NaN where
    sigma is 0 or there is no ring.
    ``percentiles``: a sequence as the ``q`` of ``component_quantiles``, e.g. ``(5, "median", 95)``; it needs ``mag1c`` and adds, over
    the plume's own finite pixels and from one more ``component_quantiles`` call, ``mag1c_p5``, ``mag1c_median``, ``mag1c_p95`` (names
    ``f"mag1c_p{q:g}"``).  None adds nothing."""
    return _plume_table(mask, mag1c, prob, label_mask, connectivity, min_area, geotransform, pixel_area_m2, background_ring_px,
                        background_gap_px, quantify, background_stat, percentiles)[0]


def fetch_profiles(mask, mag1c, quantify, prob=None, label_mask=None, connectivity=2, min_area=1, geotransform=None,
                   pixel_area_m2=None, background_ring_px=None, background_gap_px=0.0, background_stat="mean", percentiles=None):
    """``plume_table(..., quantify=quantify)`` and the curves behind its rates, for plotting -> ``(table, curves)``: ``curves`` a
    dict with ``radii_m`` (K,) and, one row per row of the table, ``n_px`` (pixels with finite mag1c inside circle j), ``ime_kg``
    (IME_j, above the background with ``background_ring_px``), ``q_kg_h`` (``3600 U IME_j / r_j``) and ``used`` (bool: the radii
    that enter ``q_fetch_kg_h``), all (rows, K).  ``background_stat`` and ``percentiles`` are passed through: with ``"median"`` the
    curves are taken above the ring median.  The same device work as ``plume_table``."""
    if quantify is None:
        raise ValueError("fetch_profiles: quantify is required (a dict with wind_speed_m_s)")
    return _plume_table(mask, mag1c, prob, label_mask, connectivity, min_area, geotransform, pixel_area_m2, background_ring_px,
                        background_gap_px, quantify, background_stat, percentiles)


def _quantify_plan(quantify, mag1c, geotransform, pixel_area_m2):
    """what ``plume_table`` can settle about ``quantify`` before the device is used -> None or {settings, radii_m, radii_px,
    pixel_size_m}"""
    from . import quantify as qf
    settings = qf.check_quantify(quantify, "plume_table")
    if settings is None:
        return None
    if mag1c is None:
        raise ValueError("plume_table: quantify needs mag1c")
    if pixel_area_m2 is None:
        raise ValueError("plume_table: quantify needs pixel_area_m2, the area of a pixel on a metric grid; a longitude / latitude "
                         "grid has none (the scene calls put their products on one with crs=\"utm\")")
    area = float(pixel_area_m2)
    if not area > 0.0 or not np.isfinite(area):
        raise ValueError(f"plume_table: pixel_area_m2 {pixel_area_m2!r} must be positive and finite")
    if geotransform is not None:
        gt = _gt6(geotransform, "plume_table")
        if abs(gt[1]) != abs(gt[5]):
            raise ValueError(f"plume_table: quantify needs square pixels, the geotransform has {abs(gt[1])} x {abs(gt[5])}")
    elif settings.get("origin_xy"):
        raise ValueError("plume_table: origin_xy=True needs a geotransform")
    px = float(np.sqrt(area))
    radii_m, radii_px = qf.radii_for(settings, px)
    qf.squared_edges(radii_px, "plume_table: quantify", _lib.EDT_FAR - 1)
    return {"settings": settings, "radii_m": radii_m, "radii_px": radii_px, "pixel_size_m": px}


def _origins_from_rows(settings, counts, M, geotransform):
    """the (R, 2) ``origin`` array of a quantify dict -> host int32 (N, M, 2) of (row, col), (-1, -1) for rows to skip"""
    o = np.asarray(settings["origin"], dtype=np.float64)
    per = np.minimum(np.maximum(np.asarray(counts).reshape(-1), 0), M)
    if o.shape[0] != int(per.sum()):
        raise ValueError(f"plume_table: quantify origin has {o.shape[0]} rows, the mask {int(per.sum())} plumes (before min_area)")
    if settings.get("origin_xy"):
        gt = _gt6(geotransform, "plume_table")
        with np.errstate(invalid="ignore", divide="ignore"):
            o = np.stack([(o[:, 1] - gt[3]) / gt[5], (o[:, 0] - gt[0]) / gt[1]], 1)
    ok = np.isfinite(o).all(1)
    o = np.clip(np.floor(np.where(ok[:, None], o, -1.0)), -1.0, 2.0 ** 30)
    o[o[:, 0] < 0] = -1.0
    out = np.full((per.size, M, 2), -1, dtype=np.int32)
    at = 0
    for n, c in enumerate(per):
        out[n, :c] = o[at:at + c].astype(np.int32)
        at += c
    return out


def _plume_table(mask, mag1c, prob, label_mask, connectivity, min_area, geotransform, pixel_area_m2, background_ring_px,
                 background_gap_px, quantify, background_stat="mean", percentiles=None):
    """``plume_table`` -> (table, the curves of ``fetch_profiles`` or None)"""
    shape = tuple(mask.shape)
    if background_stat not in BACKGROUND_STATS:
        raise ValueError(f"plume_table: background_stat {background_stat!r} (one of {BACKGROUND_STATS})")
    if background_stat == "median" and background_ring_px is None:
        raise ValueError("plume_table: background_stat=\"median\" needs background_ring_px")
    if percentiles is not None:
        if mag1c is None:
            raise ValueError("plume_table: percentiles needs mag1c")
        quantile_fractions(percentiles, "plume_table: percentiles")
    qplan = _quantify_plan(quantify, mag1c, geotransform, pixel_area_m2)
    if background_ring_px is not None:
        if mag1c is None:
            raise ValueError("plume_table: background_ring_px needs mag1c")
        ring2, gap2 = _ring_caps(background_ring_px, background_gap_px, "plume_table")
    for name, p in (("mag1c", mag1c), ("prob", prob), ("label_mask", label_mask)):
        if p is not None and tuple(p.shape) != shape:
            raise ValueError(f"plume_table: {name} has shape {tuple(p.shape)}, the mask {shape}")
    stacks.check_stack(mask, "plume_table", "mask")
    m = stacks.upload(mask)
    labels, counts = connected_components(m, connectivity=connectivity)
    names = [n for n, p in (("mag1c", mag1c), ("prob", prob)) if p is not None]
    planes = [stacks.upload(p, m.device) for p in (mag1c, prob) if p is not None]
    other = stacks.upload(label_mask, m.device) if label_mask is not None else None
    counts_h = np.array([counts]) if isinstance(counts, int) else counts.cpu().numpy()      # the first read-back: the counts size M
    M = max(int(counts_h.max()), 0)
    dev = {"stats": component_stats(labels, counts, planes, other, M=M)}      # {group: {column: device tensor}}, read back together
    if background_ring_px is not None:
        rings = _rings(stacks.device_labels(labels, "plume_table")[0], ring2, gap2)
        dev["ring"] = component_stats(rings, counts, planes[:1], M=M)
        if background_stat == "median":
            ring_q = component_median_mad(rings, counts, planes[0], M=M)
            dev["ring_q"] = {f: ring_q[f] for f in ("median", "mad")}
    if percentiles is not None:
        dev["plume_q"] = {"quantile": component_quantiles(labels, counts, planes[0], percentiles, M=M)["quantile"]}
    if qplan is not None:
        settings = qplan["settings"]
        if np.ndim(settings["wind_speed_m_s"]) and np.size(settings["wind_speed_m_s"]) != int(np.minimum(counts_h, M).sum()):
            raise ValueError(f"plume_table: {np.size(settings['wind_speed_m_s'])} wind speeds for {int(np.minimum(counts_h, M).sum())} "
                             "plumes (before min_area)")
        if isinstance(settings.get("origin", "max"), str):
            origins = origins_from_argmax(dev["stats"], shape[-1], names.index("mag1c"))
        else:
            origins = torch.from_numpy(_origins_from_rows(settings, counts_h, M, geotransform)).to(m.device)
        rad = component_radial(labels, counts, dev["stats"], origins, qplan["radii_px"], planes[names.index("mag1c")], M=M)
        dev["radial"] = {**rad, "origin": origins}
    flat = stacks.read_back({(g, f): t for g, cols in dev.items() for f, t in cols.items()})      # the second read-back: everything else
    host = {g: {f: flat[g, f] for f in cols} for g, cols in dev.items()}
    if qplan is not None:
        qplan["radial"] = host["radial"]
    plume_q = {"q": tuple(percentiles), **host["plume_q"]} if percentiles is not None else None
    table = table_from_stats(host["stats"], counts_h, shape[-1], names, other is not None, min_area, geotransform, pixel_area_m2,
                             host.get("ring"), qplan, host.get("ring_q"), plume_q)
    return table, (qplan["curves"] if qplan is not None else None)


def _score(pred, lab, min_overlap_px):
    """the dict ``match_plumes`` returns, from the two tables with their ``overlap_px`` columns"""
    tp = int((pred["overlap_px"] >= min_overlap_px).sum())
    fp = len(pred) - tp
    fn = int((lab["overlap_px"] < min_overlap_px).sum())
    cm = torch.tensor([[0, fp], [fn, tp]], dtype=torch.float64)
    return {"pred": pred, "label": lab, "tp": tp, "fp": fp, "fn": fn,
            "precision": float(metrics.precision(cm)), "recall": float(metrics.recall(cm))}


def match_plumes(pred_mask, label_mask, connectivity=2, min_overlap_px=1, min_area=1, tolerance_px=0.0):
    """Object-level detection score of a predicted against a labelled plume mask (same shape, numpy or device).  Both masks are
    labelled and each is reduced against the other: a predicted plume is a true positive when at least ``min_overlap_px`` of its
    pixels are labelled, a false positive otherwise; a labelled plume with fewer than ``min_overlap_px`` predicted pixels is a
    false negative.  Returns ``{"pred": table, "label": table, "tp", "fp", "fn", "precision", "recall"}``, the tables as
    ``plume_table`` gives them (with ``overlap_px``), the ratios from ``starcop_amd.metrics`` on [[0, fp], [fn, tp]].

    ``tolerance_px`` > 0 matches with a tolerance: each side is reduced against the OTHER mask dilated by the disc of that radius
    (``morphology.dilate``), so ``overlap_px`` counts the pixels of a plume that lie within ``tolerance_px`` of a pixel of the other
    mask.  0 is the plain overlap, with no extra launch."""
    near_label, near_pred = _dilated_others(pred_mask, label_mask, tolerance_px, "match_plumes")
    pred = plume_table(pred_mask, label_mask=near_label, connectivity=connectivity, min_area=min_area)
    lab = plume_table(label_mask, label_mask=near_pred, connectivity=connectivity, min_area=min_area)
    return _score(pred, lab, min_overlap_px)


def _dilated_others(pred_mask, label_mask, tolerance_px, who):
    """(label mask, predicted mask) as the other side of a match sees them: dilated by ``tolerance_px``, or as they are at 0"""
    tol = float(tolerance_px)
    if not tol >= 0.0:
        raise ValueError(f"{who}: tolerance_px {tolerance_px!r} must be >= 0")
    if tol == 0.0:
        return label_mask, pred_mask
    from .morphology import dilate
    return dilate(label_mask, tol), dilate(pred_mask, tol)


OUTLINE_FIELDS = ("vertices", "ring_offsets", "ring_label", "ring_area2")


def _empty_outlines(dev):
    return {"vertices": torch.zeros((0, 2), dtype=torch.int32, device=dev), "ring_offsets": torch.zeros(1, dtype=torch.int64, device=dev),
            "ring_label": torch.zeros(0, dtype=torch.int32, device=dev), "ring_area2": torch.zeros(0, dtype=torch.int64, device=dev)}


def _outlines_one(lab, connectivity, collinear):
    """the stages of ``sc_component_outlines`` on one (H, W) int32 image, the scans and the sort of the ring keys between them"""
    lib = _lib.load()
    dev = lab.device
    H, W = lab.shape

    def i32(n):
        return torch.empty(n, dtype=torch.int32, device=dev)

    def i64(n):
        return torch.empty(n, dtype=torch.int64, device=dev)
    a = _lib.sc_outline_args()
    a.labels, a.H, a.W, a.connectivity = lab.data_ptr(), H, W, int(connectivity)
    if 4 * H * W >= 2 ** 31 or H * W == 0:                       # refused before anything is allocated: the call has the message
        check(lib.sc_component_outlines(a, _lib.OUTLINE_COUNT, stream()))
    cnt = i32(H * W)
    a.cnt = cnt.data_ptr()
    check(lib.sc_component_outlines(a, _lib.OUTLINE_COUNT, stream()))
    prefix = torch.cumsum(cnt, 0, dtype=torch.int32)
    E = int(prefix[-1].item())                                   # read-back: sizes every buffer below
    if E == 0:
        return _empty_outlines(dev)
    wb = lib.sc_component_outlines_workspace_bytes(H, W, E)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    keys, stats = i64(E), i32(2)
    a.E, a.prefix, a.work, a.work_bytes, a.keys, a.stats = E, prefix.data_ptr(), work.data_ptr(), wb, keys.data_ptr(), stats.data_ptr()
    check(lib.sc_component_outlines(a, _lib.OUTLINE_TRACE, stream()))
    R, V = (int(v) for v in stats.cpu().tolist())                # read-back: rings and corner vertices
    skeys = torch.sort(keys).values[:R].contiguous()
    out = {"ring_label": i32(R), "ring_area2": i64(R)}
    ring_len, ring_start = i64(R), torch.zeros(R + 1, dtype=torch.int64, device=dev)
    a.R, a.sorted_keys, a.ring_len = R, skeys.data_ptr(), ring_len.data_ptr()
    a.ring_label, a.ring_area2 = out["ring_label"].data_ptr(), out["ring_area2"].data_ptr()
    check(lib.sc_component_outlines(a, _lib.OUTLINE_RINGS, stream()))
    torch.cumsum(ring_len, 0, out=ring_start[1:])
    ordered, okeep = torch.empty((E, 2), dtype=torch.int32, device=dev), i32(E)
    a.ring_start, a.ordered, a.ordered_keep = ring_start.data_ptr(), ordered.data_ptr(), okeep.data_ptr()
    check(lib.sc_component_outlines(a, _lib.OUTLINE_SCATTER, stream()))
    if collinear:
        out.update(vertices=ordered, ring_offsets=ring_start)
        return out
    kprefix = torch.cumsum(okeep, 0, dtype=torch.int32)
    out.update(vertices=torch.empty((V, 2), dtype=torch.int32, device=dev), ring_offsets=i64(R + 1))
    a.V, a.keep_prefix, a.vertices, a.ring_offsets = V, kprefix.data_ptr(), out["vertices"].data_ptr(), out["ring_offsets"].data_ptr()
    check(lib.sc_component_outlines(a, _lib.OUTLINE_COMPACT, stream()))
    return out


def component_outlines(labels, counts=None, connectivity=2, collinear=False):
    """Polygon rings of every component of a label image (``sc_component_outlines``; include/starcop_hip.h has the edge
    numbering and the turning rule).

    ``labels``: device int32 (H, W) or (N, H, W) as ``connected_components`` returns them: 0 background, component k the pixels of
    value k.  ``counts`` (an int, an (N,) tensor or None) is accepted as ``component_stats`` accepts it and only checked for its
    length: every positive value has its outline traced.  ``connectivity`` must be the one the image was labelled with: at a
    corner where two pixels of a component meet diagonally, 2 passes to the diagonal pixel, 1 stays on its own.

    Returns, per image (a dict for (H, W), a list of dicts for (N, H, W)), device tensors ``vertices`` (V, 2) int32 (row, column)
    of pixel CORNERS (corner (r, c) is the upper-left corner of pixel (r, c)), ``ring_offsets`` (R+1,) int64 (ring i is
    ``vertices[ring_offsets[i]:ring_offsets[i+1]]``, not closed), ``ring_label`` (R,) int32 and ``ring_area2`` (R,) int64, the
    signed doubled area sum(col_i * row_{i+1} - col_{i+1} * row_i): positive for an exterior, negative for a hole.  A ring has
    its component on the right of the direction of travel (row axis down).  Rings are ordered by label, the exterior first,
    then by their first edge in raster order.  ``collinear=False`` drops every vertex that lies on a straight run; the ring then
    starts at the first corner at or after its first edge.  A ring may touch itself at a corner where two pixels of the component
    meet diagonally: with connectivity 2 the ring around both passes through that corner twice, with connectivity 1 a hole
    ring whose background is pinched there does.  That is how GDAL's polygonize leaves such rings too; they are not repaired.
    Integers throughout: two calls give identical bytes."""
    if not isinstance(labels, torch.Tensor):
        raise ValueError("component_outlines: labels must be a device tensor (plume_outlines takes numpy masks)")
    if connectivity not in (1, 2):
        raise ValueError(f"component_outlines: connectivity {connectivity!r} (1 or 2)")
    lab, single = stacks.stack3(labels, "component_outlines: labels")
    if counts is not None:
        stacks.counts_i32(counts, lab.shape[0], None, "component_outlines")
    lab = stacks.labels_i32(lab)
    res = [_outlines_one(lab[n], connectivity, bool(collinear)) for n in range(lab.shape[0])]
    return res[0] if single else res


def _gt6(geotransform, who):
    gt = [float(v) for v in np.asarray(geotransform, dtype=np.float64).ravel()]
    if len(gt) != 6:
        raise ValueError(f"{who}: geotransform must have 6 numbers, got {len(gt)}")
    if gt[2] != 0.0 or gt[4] != 0.0:
        raise NotImplementedError(f"{who}: rotated geotransform (terms {gt[2]}, {gt[4]}) is not supported")
    return gt


def polygons_from_rings(vertices, ring_offsets, ring_label, ring_area2, geotransform=None, min_area=1, item=0):
    """The host half of ``plume_outlines``: the four arrays of ``component_outlines`` (numpy) -> ``{(item, label): [ring, ...]}``,
    every ring a closed (n+1, 2) float64 array of (x, y), the exterior first, then the holes.  x = gt0 + col * gt1 and
    y = gt3 + row * gt5 (corners: no + 0.5); without a geotransform (x, y) = (col, row).  Components of fewer than ``min_area``
    pixels (half the sum of their rings' ``ring_area2``) are left out.  No device involved."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64)
    lab = np.asarray(ring_label, dtype=np.int64)
    a2 = np.asarray(ring_area2, dtype=np.int64)
    if geotransform is not None:
        gt = _gt6(geotransform, "plume_outlines")
        xy = np.stack([gt[0] + v[:, 1] * gt[1], gt[3] + v[:, 0] * gt[5]], 1)
    else:
        xy = np.stack([v[:, 1], v[:, 0]], 1)
    out = {}
    i, R = 0, lab.size
    while i < R:
        j = i
        while j < R and lab[j] == lab[i]:
            j += 1
        if a2[i] <= 0:
            raise ValueError(f"polygons_from_rings: the first ring of label {lab[i]} is not an exterior")
        if int(a2[i:j].sum()) // 2 >= max(int(min_area), 1):
            out[(int(item), int(lab[i]))] = [np.concatenate([xy[off[q]:off[q + 1]], xy[off[q]:off[q] + 1]]) for q in range(i, j)]
        i = j
    return out


def plume_outlines(mask, connectivity=2, min_area=1, geotransform=None):
    """Polygons of the plumes of ``mask != 0``, an (H, W) or (N, H, W) mask, numpy or device: labels the mask as ``plume_table``
    does (same ``plume_id``), traces every component on the device (``component_outlines``, corners only) and reads the rings
    back in one copy.  Returns ``{(item, plume_id): [ring, ...]}`` as ``polygons_from_rings`` gives them."""
    stacks.check_stack(mask, "plume_outlines", "mask")
    if geotransform is not None:
        _gt6(geotransform, "plume_outlines")
    m = stacks.upload(mask)
    labels, counts = connected_components(m, connectivity=connectivity)
    res = component_outlines(labels, counts, connectivity=connectivity, collinear=False)
    res = [res] if isinstance(res, dict) else res
    host = stacks.read_back({(n, f): r[f] for n, r in enumerate(res) for f in OUTLINE_FIELDS})      # the one read-back
    out = {}
    for n in range(len(res)):           # polygons_from_rings takes the int32 columns as they are: it widens them itself
        out.update(polygons_from_rings(*(host[n, f] for f in OUTLINE_FIELDS), geotransform=geotransform, min_area=min_area, item=n))
    return out


def _shoelace(ring):
    """signed doubled area of a closed (n+1, 2) ring of (x, y), taken about its first vertex"""
    x, y = ring[:, 0] - ring[0, 0], ring[:, 1] - ring[0, 1]
    return float(np.sum(x[:-1] * y[1:] - x[1:] * y[:-1]))


def _properties(row):
    props = {}
    for c, v in row.items():
        if c in ("x", "y"):
            continue
        v = v.item() if hasattr(v, "item") else v
        props[c] = None if isinstance(v, float) and not np.isfinite(v) else v
    props["bbox_px"] = [int(row["row_min"]), int(row["col_min"]), int(row["row_max"]), int(row["col_max"])]
    return props


def write_plumes(table, path, outlines=None):
    """``.csv``: the table as it is (no index column; ``outlines`` is ignored).  ``.geojson``: one Point feature per plume at
    (``x``, ``y``) -- the table must carry them, i.e. come from ``plume_table(..., geotransform=...)`` -- with every other column
    as a property and the bounding box as ``bbox_px`` = [row_min, col_min, row_max, col_max].  With ``outlines`` (the dict of
    ``plume_outlines`` of the same mask) every feature is a Polygon instead, looked up by (``item``, ``plume_id``), with the same
    properties; a row without an outline is a ValueError.  Rings are wound as RFC 7946 asks, the exterior counter-clockwise
    and the holes clockwise in (x, y) -- reversed where the geotransform flips an axis (north up) -- and the coordinates stay in
    the raster's reference system."""
    path = str(path)
    if path.startswith("gs://"):
        raise NotImplementedError(f"{path}: writing to Google Cloud Storage is not supported")
    if path.endswith(".csv"):
        table.to_csv(path, index=False)
        return path
    if not path.endswith(".geojson"):
        raise ValueError(f"write_plumes: {path}: expected a .csv or .geojson path")
    if outlines is None and ("x" not in table.columns or "y" not in table.columns):
        raise ValueError("write_plumes: a .geojson needs the x / y columns (plume_table(..., geotransform=...))")
    feats = []
    for row in table.to_dict("records"):
        if outlines is None:
            geom = {"type": "Point", "coordinates": [float(row["x"]), float(row["y"])]}
        else:
            key = (int(row["item"]), int(row["plume_id"]))
            if key not in outlines:
                raise ValueError(f"write_plumes: no outline for item {key[0]}, plume {key[1]}")
            rings = []
            for q, ring in enumerate(outlines[key]):
                ring = np.asarray(ring, dtype=np.float64)
                if (_shoelace(ring) < 0) == (q == 0):            # exterior clockwise, or a hole counter-clockwise
                    ring = ring[::-1]
                rings.append(ring.tolist())
            geom = {"type": "Polygon", "coordinates": rings}
        feats.append({"type": "Feature", "geometry": geom, "properties": _properties(row)})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": feats}, f)
    return path


def read_plumes(path):
    """The inverse of ``write_plumes`` for a ``.geojson`` FeatureCollection -> ``(table, polygons)``: ``table`` a DataFrame of the
    features' properties, one row per feature in file order; ``polygons`` a list aligned with the rows, for a ``Polygon`` its rings
    and for a ``MultiPolygon`` the rings of all its parts in one list (float64 (n, 2) arrays of (x, y), closed as the file has
    them), ``None`` for a ``Point``.  Any other geometry is a ValueError.  The coordinates are taken as the raster's reference
    system: nothing is reprojected.  ``rasterize_polygons`` takes the list as it is (``None`` burns nothing)."""
    import pandas as pd
    path = str(path)
    if path.startswith("gs://"):
        raise NotImplementedError(f"{path}: reading from Google Cloud Storage is not supported")
    if not path.endswith(".geojson"):
        raise ValueError(f"read_plumes: {path}: expected a .geojson path")
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("type") != "FeatureCollection":
        raise ValueError(f"read_plumes: {path}: not a GeoJSON FeatureCollection")
    props, polygons = [], []
    for k, feat in enumerate(doc.get("features", [])):
        geom = feat.get("geometry") or {}
        kind = geom.get("type")
        if kind == "Point":
            polygons.append(None)
        elif kind == "Polygon":
            polygons.append([np.asarray(r, dtype=np.float64)[:, :2] for r in geom["coordinates"]])
        elif kind == "MultiPolygon":
            polygons.append([np.asarray(r, dtype=np.float64)[:, :2] for part in geom["coordinates"] for r in part])
        else:
            raise ValueError(f"read_plumes: {path}: feature {k} has geometry {kind!r} (Point, Polygon or MultiPolygon)")
        props.append(dict(feat.get("properties") or {}))
    return pd.DataFrame(props), polygons


RAST_COORD_LIMIT = 2.0 ** 31


def _polygon_list(polygons, item=0):
    """a sequence of ring lists, or the dict of ``plume_outlines`` -> (list of ring lists, their default burn values)"""
    if isinstance(polygons, dict):
        keys = [k for k in polygons if int(k[0]) == int(item)]
        return [polygons[k] for k in keys], [int(k[1]) for k in keys]
    polys = list(polygons)
    return polys, list(range(1, len(polys) + 1))


def polygon_edges(polygons, shape, geotransform=None):
    """The host half of ``rasterize_polygons``: a list of ring lists -> ``(edges, table)`` as ``sc_rasterize_polygons`` takes
    them.  ``edges``: float64 (E, 4), (x0, y0, x1, y1) in pixel coordinates, every ring closed (the closing edge is added when the
    last vertex differs from the first).  ``table``: int32 (P, 8), per polygon its edge range, the clipped box rows [r0, r1) and
    columns [c0, c1) -- every pixel the polygon can toggle, a pixel to spare on each side -- and the first job index
    (include/starcop_hip.h: sc_rast_poly).  With ``geotransform`` the rings are (x, y) and become col = (x - gt0) / gt1,
    row = (y - gt3) / gt5 in float64; without, they are (col, row).  An entry that is ``None`` has no edges.  ValueError for
    coordinates that are not finite or reach 2^31 in magnitude, rings of fewer than 3 distinct positions and H * W >= 2^31;
    NotImplementedError for a rotated geotransform.  No device involved."""
    H, W = (int(v) for v in shape)
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError(f"rasterize_polygons: bad shape {(H, W)} (positive, H * W < 2^31)")
    gt = _gt6(geotransform, "rasterize_polygons") if geotransform is not None else None
    if gt is not None and (gt[1] == 0.0 or gt[5] == 0.0):
        raise ValueError(f"rasterize_polygons: geotransform with a zero pixel size ({gt[1]}, {gt[5]})")
    # every ring of every polygon in one (N, 2) array: the checks, the closing edges and the boxes are whole-array operations
    rings, ring_poly = [], []
    for i, poly in enumerate(polygons):
        for q, ring in enumerate(poly if poly is not None else ()):
            a = np.asarray(ring, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != 2:
                raise ValueError(f"rasterize_polygons: polygon {i}, ring {q}: expected an (n, 2) array, got {a.shape}")
            if len(a) < 3:
                raise ValueError(f"rasterize_polygons: polygon {i}, ring {q}: fewer than 3 distinct positions")
            rings.append(a)
            ring_poly.append(i)
    P = len(polygons)
    table = np.zeros((P, 8), dtype=np.int32)
    if not rings:
        return np.zeros((0, 4), dtype=np.float64), table
    ring_poly = np.asarray(ring_poly, dtype=np.int64)
    n = np.array([len(a) for a in rings], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(n)])
    A = np.concatenate(rings)
    rid = np.repeat(np.arange(len(rings)), n)

    def refuse(bad_vertex, what):
        k = int(rid[np.nonzero(bad_vertex)[0][0]])
        i = int(ring_poly[k])
        raise ValueError(f"rasterize_polygons: polygon {i}, ring {k - int(np.searchsorted(ring_poly, i))}: {what}")
    finite = np.isfinite(A).all(1)
    if gt is not None and finite.all():
        A = np.stack([(A[:, 0] - gt[0]) / gt[1], (A[:, 1] - gt[3]) / gt[5]], 1)
    ok = np.isfinite(A).all(1) & (np.abs(A) < RAST_COORD_LIMIT).all(1)
    if not ok.all():
        refuse(~ok, "coordinates must be finite and below 2^31 in magnitude (pixel units)")
    # at least 3 distinct positions: some vertex differs from the first one and from the first that differs from it
    idx = np.arange(len(A))
    off0 = (A != A[start[:-1]][rid]).any(1)
    second = np.minimum.reduceat(np.where(off0, idx, len(A)), start[:-1])
    off1 = off0 & (A != A[np.minimum(second, len(A) - 1)][rid]).any(1)
    enough = np.logical_or.reduceat(off1, start[:-1])
    if not enough.all():
        refuse(~enough[rid], "fewer than 3 distinct positions")
    # vertex j -> its successor in the ring, the last one back to the first; a ring that is closed already has no such edge
    nxt = idx + 1
    last = start[1:] - 1
    nxt[last] = start[:-1]
    keep = np.ones(len(A), dtype=bool)
    keep[last] = (A[last] != A[start[:-1]]).any(1)
    edges = np.ascontiguousarray(np.concatenate([A, A[nxt]], 1)[keep])
    ring_edges = n - 1 + keep[last]
    first_ring = np.searchsorted(ring_poly, np.arange(P + 1))              # ring_poly is non-decreasing
    e_at = np.concatenate([[0], np.cumsum(ring_edges)])
    table[:, 0], table[:, 1] = e_at[first_ring[:-1]], e_at[first_ring[1:]]
    has = first_ring[1:] > first_ring[:-1]
    lo = np.minimum.reduceat(A, start[first_ring[:-1][has]])
    hi = np.maximum.reduceat(A, start[first_ring[:-1][has]])
    # rows whose scanline an edge can cross and columns a crossing can land in, one to spare: a box that is too large costs time
    # only, the rule is applied per edge on the device
    r0, r1 = np.clip(np.floor(lo[:, 1] - 0.5), 0, H), np.clip(np.ceil(hi[:, 1] - 0.5) + 1, 0, H)
    c0, c1 = np.clip(np.floor(lo[:, 0] - 0.5) - 1, 0, W), np.clip(np.ceil(hi[:, 0] - 0.5) + 2, 0, W)
    box = np.stack([r0, r1, c0, c1], 1).astype(np.int32)
    box[(r1 <= r0) | (c1 <= c0)] = 0
    table[has, 2:6] = box
    rows = (table[:, 3] - table[:, 2]).astype(np.int64)
    job0 = np.concatenate([[0], np.cumsum(rows)])
    E, jobs = len(edges), int(job0[-1])
    if E >= 2 ** 31 or jobs >= 2 ** 31:
        raise ValueError(f"rasterize_polygons: {E} edges, {jobs} (polygon, row) jobs: both must stay below 2^31")
    table[:, 6] = job0[:-1]
    return edges, table


def _align256(n):
    return (int(n) + 255) // 256 * 256


def rasterize_upload(edges, table, values=None, device="cuda"):
    """``polygon_edges`` output (and int32 ``values``, or None for 1..P) -> the operands of ``rasterize_launch``: edges, table and
    values packed into one buffer and uploaded in ONE copy"""
    E, P = len(edges), len(table)
    off_t = _align256(E * 32)
    off_v = off_t + _align256(P * 32)
    buf = np.zeros(off_v + _align256(P * 4) + 256, dtype=np.uint8)
    buf[:E * 32] = edges.view(np.uint8).reshape(-1)
    buf[off_t:off_t + P * 32] = table.view(np.uint8).reshape(-1)
    if values is not None:
        buf[off_v:off_v + P * 4] = np.ascontiguousarray(values, dtype=np.int32).view(np.uint8)
    _lib.require_device()
    return {"buffer": torch.from_numpy(buf).to(device), "table": table, "E": E, "off_table": off_t,
            "off_values": off_v if values is not None else None}


def rasterize_launch(ops, shape, out=None):
    """one ``sc_rasterize_polygons`` call on uploaded operands -> device int32 (H, W)"""
    H, W = (int(v) for v in shape)
    buf, table = ops["buffer"], ops["table"]
    if out is None:
        out = torch.empty((H, W), dtype=torch.int32, device=buf.device)
    a = _lib.sc_rast_args()
    base = buf.data_ptr()
    a.edges, a.polys, a.polys_host = base, base + ops["off_table"], table.ctypes.data
    a.values = base + ops["off_values"] if ops["off_values"] is not None else None
    a.out, a.E, a.P, a.H, a.W = out.data_ptr(), ops["E"], len(table), H, W
    check(_lib.load().sc_rasterize_polygons(a, stream()))
    return out


def rasterize_polygons(polygons, shape, geotransform=None, values=None, item=0):
    """Burn polygons into a label image on the device, the inverse of ``plume_outlines`` (``sc_rasterize_polygons``;
    include/starcop_hip.h has the rule): -> device int32 (H, W), 0 where no polygon covers the pixel.

    ``polygons``: a sequence of ring lists (every ring an (n, 2) array, n >= 3, closed or not, any winding; ``None`` burns
    nothing), or the dict ``{(item, plume_id): [ring, ...]}`` of ``plume_outlines``, iterated in its order, of which only the keys
    of ``item`` are burnt.  With ``geotransform`` (GDAL 6-tuple, north up; a rotated one is a NotImplementedError) the rings are
    (x, y) and are converted on the host in float64, col = (x - gt0) / gt1 and row = (y - gt3) / gt5; without, they are (col, row):
    pixel (r, c) covers [c, c+1) x [r, r+1).  Coverage is even-odd over all rings of a polygon (exterior and holes, the parts of a
    MultiPolygon), a pixel belongs to a polygon when its centre is inside, centres on the outline by a top-left rule.  Polygon i
    burns ``values[i]`` (int32; default i + 1, for the dict its ``plume_id``); where polygons overlap the later one wins.
    Vertices may lie anywhere outside the raster.  Two calls give identical bytes."""
    polys, default = _polygon_list(polygons, item)
    H, W = (int(v) for v in shape)
    edges, table = polygon_edges(polys, (H, W), geotransform)
    P = len(polys)
    vals = np.asarray(default if values is None else values).reshape(-1)
    if vals.size != P:
        raise ValueError(f"rasterize_polygons: {vals.size} values for {P} polygons")
    if P and (vals.dtype.kind not in "iu" or vals.min() < -2 ** 31 or vals.max() >= 2 ** 31):
        raise ValueError("rasterize_polygons: values must be integers in the int32 range")
    _lib.require_device()
    if P == 0 or not (table[:, 3] > table[:, 2]).any():
        return torch.zeros((H, W), dtype=torch.int32, device="cuda")
    identity = np.array_equal(vals, np.arange(1, P + 1))
    return rasterize_launch(rasterize_upload(edges, table, None if identity else vals.astype(np.int32)), (H, W))


def burn_and_match(pred_mask, polygons, geotransform=None, connectivity=2, min_overlap_px=1, min_area=1, tolerance_px=0.0):
    """The polygons burnt with values 1..P on the grid of ``pred_mask`` and that image scored against the mask -> (burnt, device
    int32 (H, W); the dict ``match_plumes_polygons`` returns) -- for callers that keep the burnt image as a label mask.
    ``tolerance_px`` as in ``match_plumes``."""
    polys, _ = _polygon_list(polygons)
    P = len(polys)
    burnt = rasterize_polygons(polys, tuple(pred_mask.shape), geotransform=geotransform)
    other = stacks.upload(pred_mask, burnt.device)
    near_label, other = _dilated_others(other, (burnt != 0).to(torch.uint8), tolerance_px, "burn_and_match")
    pred = plume_table(pred_mask, label_mask=near_label, connectivity=connectivity, min_area=min_area)
    st = component_stats(burnt, P, other=other, M=P)
    lab = table_from_stats(stacks.read_back(st), [P], burnt.shape[-1], with_other=True, min_area=min_area)
    return burnt, _score(pred, lab, min_overlap_px)


def match_plumes_polygons(pred_mask, polygons, geotransform=None, connectivity=2, min_overlap_px=1, min_area=1, tolerance_px=0.0):
    """``match_plumes`` against labelled POLYGONS (a sequence of ring lists or the dict of ``plume_outlines``, as
    ``rasterize_polygons`` takes them; with ``geotransform`` in its coordinates): the polygons are burnt with values 1..P on the
    grid of ``pred_mask`` ((H, W), numpy or device) and the labelled objects are the polygons themselves, not the connected
    components of their union -- two polygons that share an edge stay two.  The ``label`` table is ``component_stats`` of the burnt
    image against ``pred_mask``, one row per polygon that burnt at least ``min_area`` pixels (``plume_id`` = its position + 1);
    the ``pred`` table is ``plume_table(pred_mask, label_mask=burnt != 0)``.  ``tolerance_px`` as in ``match_plumes``: each side is
    reduced against the other dilated by that radius.  Returns the dict ``match_plumes`` returns."""
    if len(pred_mask.shape) != 2:
        raise ValueError(f"match_plumes_polygons: expected an (H, W) mask, got {tuple(pred_mask.shape)}")
    return burn_and_match(pred_mask, polygons, geotransform, connectivity, min_overlap_px, min_area, tolerance_px)[1]
