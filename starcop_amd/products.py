"""What a scene run leaves behind: the raster files of a prediction dict and its plume annotations, for
``pipeline.emit_granule_predict``, ``pipeline.aviris_scene_predict`` / ``aviris_scene_mag1c`` and ``sentinel2.cloud_mask_file``.

Host side only.  Which files a run writes is data (``Raster`` rows), which of them are written and with which tags is decided by
``plan_rasters`` without a device, and every file goes through ``write_raster``: ``io_formats.write_tiff`` of the host copy, or
(the only place that imports :mod:`starcop_amd.cog`) a Cloud-Optimized GeoTIFF straight from the device tensor."""
import os
import warnings
from typing import NamedTuple

import numpy as np
import torch

from . import io_formats as io


class Raster(NamedTuple):
    name: str               # file name in the output folder
    key: str                # key of the image in the prediction dict
    bands: tuple            # band descriptions
    nodata: bool            # carries GDAL_NODATA (and hands the value to the COG writer)
    mag1c_tags: bool        # carries the dataset tags of the matched filter: wavelengths, mag1c=...
    uint8: bool             # stored as uint8 whatever the dtype in the dict


MAG1C = Raster("mag1c.tif", "mf", ("CH4 Absorption (ppm x m)",), True, True, False)
ALBEDO = Raster("albedo.tif", "albedo", ("Albedo",), True, True, False)
PRED = Raster("pred.tif", "prediction", ("Plume probability",), True, False, False)
PREDBINARY = Raster("predbinary.tif", "pred_binary", ("Plume mask",), False, False, True)
RGB = Raster("rgb.tif", "rgb", ("Red (640 nm)", "Green (550 nm)", "Blue (460 nm)"), True, False, False)
LABEL = Raster("label.tif", "label_mask", ("Plume label",), False, False, True)
EMIT_RASTERS = (MAG1C, ALBEDO, PRED, PREDBINARY, RGB)
AVIRIS_RASTERS = (PRED, PREDBINARY)


def nodata_text(v):
    return f"{float(v):.9g}"


def raster_tags(row, geo_tags, nodata=None, mag1c_md=None, extra_tags=None):
    """the tags of one file, in the order they are laid out in it: georeferencing, GDAL_NODATA, ``extra_tags``, GDAL_METADATA"""
    tags = {**(geo_tags or {}), **({42113: (2, (nodata_text(nodata),))} if row.nodata else {}), **(extra_tags or {})}
    return {**tags, **io.gdal_metadata_tag(mag1c_md if row.mag1c_tags else {}, list(row.bands))}


def plan_rasters(table, folder, overwrite=False, geo_tags=None, nodata=None, mag1c_md=None, no_geo_warning=None):
    """The files of ``table`` a run will write into ``folder`` -- all with ``overwrite``, else those that do not exist -- in table
    order: [(path, key, tags, nodata for the COG writer)].  ``no_geo_warning``: issued once when something will be written and
    ``geo_tags`` is empty.  Touches the file system with ``os.path.exists`` only."""
    plan = []
    for row in table:
        path = os.path.join(folder, row.name)
        if overwrite or not os.path.exists(path):
            plan.append((path, row.key, raster_tags(row, geo_tags, nodata, mag1c_md), nodata if row.nodata else None))
    if plan and not geo_tags and no_geo_warning:
        warnings.warn(no_geo_warning)
    return plan


def write_raster(path, image, tags, cog=False, nodata=None):
    """one raster product, BLOCKSIZE 128, from a device tensor or a numpy array: ``write_tiff`` of the host copy, or with ``cog``
    (True, or a dict of ``cog.write_cog`` keyword arguments) a Cloud-Optimized GeoTIFF -- tiles and overviews are made on the
    device, float32 products averaged, uint8 ones by mode, and only the tiles that are stored cross to the host"""
    if not cog:
        io.write_tiff(path, image.cpu().numpy() if isinstance(image, torch.Tensor) else image, blocksize=128, extra_tags=tags)
        return
    from .cog import write_cog
    write_cog(path, image, nodata=nodata, extra_tags=tags, **{"blocksize": 128, **(cog if isinstance(cog, dict) else {})})


def write_rasters(out, table, folder, overwrite=False, geo_tags=None, nodata=None, mag1c_md=None, cog=False, no_geo_warning=None):
    """the plan of ``plan_rasters`` carried out on the images of ``out``; the folder is created when something is written into it.
    An image that is not uint8 yet is cast where it lives: on the host for the plain file, on the device for the COG.
    Returns the paths written, in table order."""
    plan = plan_rasters(table, folder, overwrite, geo_tags, nodata, mag1c_md, no_geo_warning)
    if plan:
        os.makedirs(folder, exist_ok=True)
    as_uint8 = {row.key for row in table if row.uint8}
    for path, key, tags, cog_nodata in plan:
        image = out[key]
        if key in as_uint8 and image.dtype != torch.uint8:
            image = image.to(torch.uint8) if cog else image.cpu().numpy().astype(np.uint8)
        write_raster(path, image, tags, cog, cog_nodata)
    return [p[0] for p in plan]


REGRID_KEYS = ("mf", "albedo", "prediction", "ratio", "rgb", "pred_binary", "label_mask")


MASK_RESAMPLING = ("nearest", "mode", "max", "min")


def regrid(out, src_gt, src_crs, dst_crs, resolution=None, resampling="nearest", nodata=None, keys=REGRID_KEYS,
           mask_resampling="nearest", min_coverage=0.5):
    """The raster keys of a prediction dict put on another grid, in place: every ``out[key]`` of ``keys`` that is there -- (H, W) or
    (bands, H, W) device tensors on the grid ``(src_gt, src_crs)`` -- is warped (``warp.reproject``) onto the north-up
    ``warp.suggest_grid`` of ``dst_crs`` at ``resolution``.  Integer images (masks) are resampled with ``mask_resampling``
    (``nearest``, or on a coarser grid the footprint modes ``mode`` / ``max`` / ``min``) and no-data 0; floating-point ones with
    ``resampling`` -- one mode of ``warp.reproject`` but ``mode``, or {key: mode} with ``nearest`` for the keys it leaves out -- and
    ``nodata`` (a value, or {key: value}).  ``min_coverage`` is the footprint rule of the footprint modes (``warp.reproject``).
    Images that share dtype, mode and no-data go through one launch, so the coordinates of a pixel are computed once for all of
    them.  -> (geotransform of the new grid, its CRS, the area of a pixel in m2 -- None unless the CRS
    is a UTM zone)"""
    from . import warp
    if mask_resampling not in MASK_RESAMPLING:
        raise ValueError(f"regrid: mask_resampling {mask_resampling!r}; expected one of {MASK_RESAMPLING}")
    for m in (resampling.values() if isinstance(resampling, dict) else [resampling]):
        if m not in warp.RESAMPLING or m == "mode":
            raise ValueError(f"regrid: resampling {m!r} for floating-point images; expected one of {sorted(set(warp.RESAMPLING) - {'mode'})}")
    if not 0.0 <= float(min_coverage) <= 1.0:
        raise ValueError(f"regrid: min_coverage {min_coverage!r} outside [0, 1]")
    have = [k for k in keys if out.get(k) is not None]
    if not have:
        raise ValueError(f"regrid: none of {keys} in the prediction dict")
    shape = tuple(out[have[0]].shape[-2:])
    dst_shape, dst_gt = warp.suggest_grid(shape, src_gt, src_crs, dst_crs, resolution)
    groups = {}
    for k in have:
        t = out[k]
        if tuple(t.shape[-2:]) != shape:
            raise ValueError(f"regrid: {k} is {tuple(t.shape)}, {have[0]} {tuple(out[have[0]].shape)}: one grid per call")
        if t.dtype.is_floating_point:
            mode = resampling.get(k, "nearest") if isinstance(resampling, dict) else resampling
            fill = nodata.get(k) if isinstance(nodata, dict) else nodata
        else:
            mode, fill = mask_resampling, 0
        groups.setdefault((t.dtype, mode, 0 if fill is None else fill), []).append(k)
    for (_, mode, fill), ks in groups.items():
        planes = [p for k in ks for p in ([out[k]] if out[k].dim() == 2 else out[k].unbind(0))]
        res = warp.reproject(planes, src_gt, src_crs, dst_gt, dst_crs, dst_shape, mode, fill, min_coverage)
        i = 0
        for k in ks:
            n = 1 if out[k].dim() == 2 else out[k].shape[0]
            out[k] = res[i] if out[k].dim() == 2 else res[i:i + n]
            i += n
    metric = dst_crs is not None and warp.crs_kind(dst_crs)[0] == 2
    return dst_gt, dst_crs, (abs(dst_gt[1] * dst_gt[5]) if metric else None)


SOURCE = Raster("source.tif", "source", ("Source scene",), True, False, True)
SOURCE_NONE = 255           # in source.tif: no scene has a valid pixel here


def mosaic(outs, dst_crs=None, resolution=None, rule="max", key="prediction", resampling="nearest", nodata=None, keys=REGRID_KEYS,
           grids=None):
    """N prediction dicts -- as ``pipeline.emit_granule_predict(..., georeferenced=True)`` / ``aviris_scene_predict`` return them,
    each with ``geotransform`` and ``crs``, or with ``grids=[(gt, crs), ...]`` -- composed into ONE new dict on the
    ``mosaic.union_grid`` of their grids in ``dst_crs`` (default: the CRS of the first) at ``resolution``; the inputs stay untouched.

    The float32 raster keys of ``keys`` that every input carries go through one ``mosaic.mosaic`` launch with ``rule`` and the
    plane ``key`` as key (None: the footprint alone), ``resampling`` and ``nodata`` (a value, or {key: value}; default 0); the
    integer keys (``pred_binary``, ``label_mask``) follow by rule ``"index"`` with the index of that launch, so mask, probability
    and mag1c of a pixel come from the same scene.  With ``rule="mean"`` there is no winner: the masks go by ``"first"`` over the
    footprint.  Added: ``geotransform``, ``crs``, ``source_index`` (int32: the scene of every pixel, -1 for none) and
    ``source_count`` (int32: scenes with a valid pixel).  ``annotate`` works on the result as it is, so plume tables, outlines and
    label polygons over a mosaic count each plume once."""
    from . import mosaic as mz
    outs = list(outs)
    if grids is None:
        grids = [(o.get("geotransform"), o.get("crs")) for o in outs]
    grids = list(grids)
    if len(grids) != len(outs) or any(g[0] is None for g in grids):
        raise ValueError("mosaic: every input needs a geotransform: `geotransform` / `crs` in the dict, or grids=[(gt, crs), ...]")
    if not 1 <= len(outs) <= mz.MAX_SOURCES:
        raise ValueError(f"mosaic: {len(outs)} inputs; one call takes 1 to {mz.MAX_SOURCES}")
    dst_crs = grids[0][1] if dst_crs is None else dst_crs
    have = [k for k in keys if all(o.get(k) is not None for o in outs)]
    floats = [k for k in have if outs[0][k].dtype.is_floating_point]
    ints = [k for k in have if k not in floats]
    if not floats or (key is not None and key not in floats):
        raise ValueError(f"mosaic: the key {key!r} must be a floating-point raster every input carries; common rasters: {have}")
    shapes = [tuple(o[have[0]].shape[-2:]) for o in outs]
    for o, shape in zip(outs, shapes):
        if any(tuple(o[k].shape[-2:]) != shape for k in have):
            raise ValueError("mosaic: the rasters of one input share one grid")
    dst_shape, dst_gt = mz.union_grid([(s, g, c) for s, (g, c) in zip(shapes, grids)], dst_crs, resolution)

    def planes(o, ks):
        return [p for k in ks for p in ([o[k]] if o[k].dim() == 2 else o[k].unbind(0))]

    def split(res, ks, new):
        i = 0
        for k in ks:
            n = 1 if outs[0][k].dim() == 2 else outs[0][k].shape[0]
            new[k] = res[i] if outs[0][k].dim() == 2 else res[i:i + n]
            i += n

    fills, kidx = [], -1
    for k in floats:
        n = 1 if outs[0][k].dim() == 2 else outs[0][k].shape[0]
        kidx = len(fills) if k == key else kidx
        v = nodata.get(k) if isinstance(nodata, dict) else nodata
        fills += [0 if v is None else v] * n
    srcs = [(planes(o, floats), g, c) for o, (g, c) in zip(outs, grids)]
    new = {}
    if rule == "mean":
        res, count = mz.mosaic(srcs, dst_gt, dst_crs, dst_shape, rule, kidx, resampling, fills, return_count=True)
        index = None
    else:
        res, index, count = mz.mosaic(srcs, dst_gt, dst_crs, dst_shape, rule, kidx, resampling, fills, return_index=True, return_count=True)
    split(res, floats, new)
    groups = {}
    for k in ints:
        groups.setdefault(outs[0][k].dtype, []).append(k)
    if index is None:                             # mean: the first scene whose footprint holds the pixel
        index = mz.mosaic([(o[floats[0]] if o[floats[0]].dim() == 2 else o[floats[0]][0], g, c) for o, (g, c) in zip(outs, grids)],
                          dst_gt, dst_crs, dst_shape, "first", -1, return_index=True)[1]
    for ks in groups.values():
        split(mz.mosaic([(planes(o, ks), g, c) for o, (g, c) in zip(outs, grids)], dst_gt, dst_crs, dst_shape, "index", -1,
                        nodata=0, select=index), ks, new)
    new.update(geotransform=dst_gt, crs=dst_crs, source_index=index, source_count=count)
    return new


CLEAN_KEYS = ("open_radius", "min_area", "exclude", "exclude_buffer_px", "connectivity")


def check_clean(clean, who):
    """the ``clean=`` argument of the pipeline calls: None or a dict of ``clean`` keyword arguments (no device involved)"""
    if clean is None:
        return
    if not isinstance(clean, dict) or set(clean) - set(CLEAN_KEYS):
        raise ValueError(f"{who}: clean must be a dict with keys from {CLEAN_KEYS}, got {clean!r}")


def clean(out, open_radius=0.0, min_area=1, exclude=None, exclude_buffer_px=0.0, connectivity=2):
    """Clean the mask of a prediction dict in place, before ``annotate`` and the writers, so that ``predbinary.tif``, the plume
    table, the outlines and the match all describe the same plumes.  ``out["pred_binary"]`` ((H, W), device) is rewritten, in
    this order: ``morphology.opening`` by the disc of ``open_radius`` pixels; ``morphology.remove_small_objects`` below ``min_area``
    pixels (``connectivity`` as ``connected_components``); cleared wherever ``exclude != 0`` dilated by ``exclude_buffer_px`` is set.
    ``exclude``: an (H, W) array or device tensor on the grid of the mask (clouds, water, flares), or the path of a single-band
    GeoTIFF of exactly that shape -- a mask on another grid goes through ``warp.reproject_like`` first.  The defaults do nothing.
    ``prediction`` and ``mf`` are left alone.  ``out["clean"]`` records the pixels each step removed, ``{"opened_px", "sieved_px",
    "excluded_px"}``: the four pixel counts come back in one copy (the sieve, when it runs, reads the number of components back on
    its own to size its table).  -> ``out``"""
    from . import morphology as mo
    mask = out["pred_binary"]
    if mask.dim() != 2:
        raise ValueError(f"clean: pred_binary must be (H, W), got {tuple(mask.shape)}")
    if not float(open_radius) >= 0.0 or not float(exclude_buffer_px) >= 0.0:
        raise ValueError(f"clean: open_radius {open_radius!r} and exclude_buffer_px {exclude_buffer_px!r} must be >= 0")
    if connectivity not in (1, 2):
        raise ValueError(f"clean: connectivity {connectivity!r} (1 or 2)")
    if isinstance(exclude, (str, os.PathLike)):
        exclude = io.read_tiff(str(exclude))
        if exclude.ndim == 3 and exclude.shape[0] == 1:
            exclude = exclude[0]
    if exclude is not None and tuple(exclude.shape) != tuple(mask.shape):
        raise ValueError(f"clean: exclude has shape {tuple(exclude.shape)}, the mask {tuple(mask.shape)}: put it on the product grid "
                         "first (warp.reproject_like)")
    m0 = mo.dilate(mask, 0)                                  # the mask as 0 / 1
    m1 = mo.opening(m0, open_radius) if float(open_radius) > 0.0 else m0
    m2 = mo.remove_small_objects(m1, min_area, connectivity) if int(min_area) > 1 else m1
    m3 = m2
    if exclude is not None:
        if isinstance(exclude, np.ndarray):
            exclude = torch.from_numpy(np.ascontiguousarray(exclude != 0).view(np.uint8)).to(mask.device)
        m3 = m2 & (mo.dilate(exclude, exclude_buffer_px) ^ 1)
    n = torch.stack([m.sum(dtype=torch.int64) for m in (m0, m1, m2, m3)]).cpu().tolist()      # the one read-back
    out["pred_binary"] = m3.to(mask.dtype)
    out["clean"] = {"opened_px": n[0] - n[1], "sieved_px": n[1] - n[2], "excluded_px": n[2] - n[3]}
    return out


BACKGROUND_KEYS = ("ring_px", "gap_px", "stat")


def check_plume_background(plume_background, who):
    """the ``plume_background=`` argument of ``annotate`` and the pipeline calls: None, or a dict with ``ring_px`` and optionally
    ``gap_px`` and ``stat`` (``"mean"`` or ``"median"``, the ``background_stat`` of ``plumes.plume_table``; no device involved) -> the
    keyword arguments of ``plumes.plume_table``; ``background_stat`` is among them when ``stat`` is given"""
    if plume_background is None:
        return {}
    if not isinstance(plume_background, dict) or set(plume_background) - set(BACKGROUND_KEYS) or "ring_px" not in plume_background:
        raise ValueError(f"{who}: plume_background must be a dict with ring_px and keys from {BACKGROUND_KEYS}, got {plume_background!r}")
    kw = {"background_ring_px": plume_background["ring_px"], "background_gap_px": plume_background.get("gap_px", 0.0)}
    if "stat" in plume_background:
        from .plumes import BACKGROUND_STATS
        if plume_background["stat"] not in BACKGROUND_STATS:
            raise ValueError(f"{who}: plume_background stat {plume_background['stat']!r} (one of {BACKGROUND_STATS})")
        kw["background_stat"] = plume_background["stat"]
    return kw


def check_plume_quantify(plume_quantify, who):
    """the ``plume_quantify=`` argument of ``annotate`` and the pipeline calls: None, or the ``quantify=`` dict of
    ``plumes.plume_table`` -- ``wind_speed_m_s`` and keys from ``quantify.QUANTIFY_KEYS`` (``quantify.check_quantify``; no device
    involved) -> the keyword arguments of ``plumes.plume_table``"""
    from .quantify import check_quantify
    if plume_quantify is None:
        return {}
    return {"quantify": check_quantify(plume_quantify, who)}


def annotate(out, mask, mf, prob, geotransform=None, pixel_area_m2=None, plumes=False, plume_outlines=False, label_polygons=None,
             match_tolerance_px=0.0, plume_background=None, plume_quantify=None):
    """The plume annotations of a prediction dict, as asked for: ``plumes`` (``plumes.plume_table`` of ``mask`` with ``mf`` as mag1c
    and ``prob`` as probability), ``plume_outlines`` of the same mask in the same coordinates, and for ``label_polygons`` (a
    ``.geojson`` path or polygons) ``label_mask``, the polygons burnt into the grid of ``mask`` (device uint8), and ``plume_match``,
    the same burnt image scored against the mask, with ``match_tolerance_px`` as the ``tolerance_px`` of ``plumes.burn_and_match``.
    ``plume_background``: ``{"ring_px": .., "gap_px": .., "stat": "mean" | "median"}`` adds the background-ring columns of ``plumes.plume_table`` to the table
    (and so to ``plumes.csv`` and the GeoJSON properties), with ``stat="median"`` those of its ``background_stat="median"``; it needs
    ``mf``.  ``plume_quantify``: the ``quantify=`` dict of
    ``plumes.plume_table`` (``wind_speed_m_s``, ...) adds its shape, mass and emission-rate columns the same way; it needs ``mf`` and
    ``pixel_area_m2``, i.e. a metric grid: on a longitude / latitude grid it is a ValueError (the scene calls take ``crs="utm"``)."""
    from . import plumes as pl
    ring = check_plume_background(plume_background, "annotate")
    ring.update(check_plume_quantify(plume_quantify, "annotate"))
    if plumes:
        if plume_quantify is not None and pixel_area_m2 is None:
            raise ValueError("annotate: plume_quantify needs a metric grid (pixel_area_m2): this one has none -- a longitude / latitude "
                             "grid is put on a UTM zone with crs=\"utm\"")
        out["plumes"] = pl.plume_table(mask, mag1c=mf, prob=prob, geotransform=geotransform, pixel_area_m2=pixel_area_m2, **ring)
        if plume_outlines:
            out["plume_outlines"] = pl.plume_outlines(mask, geotransform=geotransform)
    if label_polygons is not None:
        if isinstance(label_polygons, (str, os.PathLike)):
            label_polygons = pl.read_plumes(label_polygons)[1]
        burnt, match = pl.burn_and_match(mask, label_polygons, geotransform, tolerance_px=match_tolerance_px)
        out["label_mask"], out["plume_match"] = (burnt != 0).to(torch.uint8), match


def write_annotations(out, folder, overwrite=False, geo_tags=None, cog=False):
    """what ``annotate`` added, as files: ``label.tif`` like ``predbinary.tif``, ``plumes.csv`` and, with outlines,
    ``plumes.geojson`` (one Polygon per row of the table) -> the paths written"""
    from .plumes import write_plumes
    files = write_rasters(out, (LABEL,), folder, overwrite, geo_tags, cog=cog) if "label_mask" in out else []
    todo = [("plumes.csv", None)] if "plumes" in out else []
    todo += [("plumes.geojson", out["plume_outlines"])] if "plume_outlines" in out else []
    for name, outlines in todo:
        path = os.path.join(folder, name)
        if overwrite or not os.path.exists(path):
            os.makedirs(folder, exist_ok=True)
            files.append(write_plumes(out["plumes"], path, outlines=outlines))
    return files
