"""End-to-end scene inference on the GPU: radiance cube -> mag1c -> network input -> plume mask.

The reference spreads this over its drivers and notebooks; the steps and their order are
  * EMIT (BASELINE configs[4]): ``mag1c_emit`` (starcop/models/mag1c_emit.py:16-90: bands in [2122, 2488] nm, float64
    filter on blocks of ``column_step`` columns) -> RGB = nearest bands to 640/550/460 nm -> range rescale of
    starcop/emit_tools/emit_dataset.py:62-106 -> ``model(x)`` -> sigmoid > 0.5;
    optionally orthorectified through the granule's GLT and written as GeoTIFFs (``georeferenced=True``, ``out_folder``);
  * AVIRIS-NG (configs[2]): ``run_mag1c`` (starcop/process_aviris.py:189-219: per detector column, alpha = 0) and the
    pre-computed RGB products -> ``padded_predict``; here ``aviris_scene_predict`` goes from the ENVI flight line to ``pred.tif`` /
    ``predbinary.tif`` / the plume table in one call (``aviris_scene_mag1c`` when there is no ``mag1c.tif``, the RGB bands read
    from the radiance cube, ``ModelModule.predict_scene`` for lines that do not fit as one image).
Everything stays on the device between the stages; with ``torch.distributed`` initialised the column blocks of the
matched filter and the scenes are independent work items (``column_range`` / ``parallel.sharded_map``): no collective on
the data path.
"""
import numpy as np
import torch

from . import mag1c, products
from .features import emit_to_aviris_input
from .model_module import masks_from_logits
from .products import nodata_text
from .scene import RECEPTIVE_HALO       # noqa: F401  (re-exported: the halo of scene_tiles / tiled_logits too)

EMIT_MAG1C_RANGE_NM = (2122.0, 2488.0)          # mag1c_emit.py:40-43
RGB_NM = (640.0, 550.0, 460.0)


def _upload_pinned(array, device):
    """host array -> device tensor through pinned memory, without waiting for the copy"""
    h = torch.from_numpy(array)
    return (h.pin_memory() if torch.cuda.is_available() else h).to(device, non_blocking=True)


def nearest_bands(wavelengths, targets=RGB_NM):
    w = np.asarray(wavelengths, dtype=np.float64)
    return [int(np.argmin(np.abs(w - t))) for t in targets]


def scene_tiles(H, W, tile=512, halo=RECEPTIVE_HALO, strips=False):
    """Partition an (H, W) scene into ``tile`` x ``tile`` cores and their halo-extended windows, clipped to the scene (so the
    convolutions' zero padding falls on the true border, as in the whole-scene forward).  ``strips``: full-width row strips of
    ``tile`` rows with a vertical halo only -- (tile + 2 halo) / tile times the scene's work instead of ((tile + 2 halo) / tile)^2
    (2.25x instead of 5x at 512 / 320).  Returns an int64 tensor (n, 8): core y0, y1, x0, x1 and window y0, y1, x0, x1.  H, W, tile
    and halo must be multiples of 32 (encoder stride): only shifts by multiples of 32 commute with the network."""
    for v, name in ((H, "H"), (W, "W"), (tile, "tile"), (halo, "halo")):
        if v % 32 or (v <= 0 and name != "halo"):
            raise ValueError(f"scene_tiles: {name}={v} must be a positive multiple of 32")
    rows = []
    tw = W if strips else tile
    for y0 in range(0, H, tile):
        for x0 in range(0, W, tw):
            y1, x1 = min(y0 + tile, H), min(x0 + tw, W)
            rows.append((y0, y1, x0, x1, max(0, y0 - halo), min(H, y1 + halo), max(0, x0 - halo), min(W, x1 + halo)))
    return torch.tensor(rows, dtype=torch.int64)


def stitch(cores, rects, H, W):
    """cores: (n, tile, tile | W) per-tile core values (zero-padded at the right / bottom scene edge) -> (H, W)"""
    out = torch.empty((H, W), dtype=cores.dtype, device=cores.device)
    for c, (y0, y1, x0, x1) in zip(cores, rects[:, :4].tolist()):
        out[y0:y1, x0:x1] = c[:y1 - y0, :x1 - x0]
    return out


@torch.no_grad()
def tiled_logits(model, x, tile=512, halo=RECEPTIVE_HALO, batch=8, group=None, shard=None, strips=False):
    """Sliding-window inference of a (C, H, W) device scene (H, W multiples of 32): the tiles are independent work items, so with
    ``torch.distributed`` initialised they are partitioned over the ranks (``parallel.sharded_map``: no collective on the data
    path, one all_gather of the core logits at the end) -- the tile-sharded mode of BASELINE configs[4].  Windows of equal
    shape are stacked into batches of up to ``batch``.  Returns (H, W) logits on every rank.
    ``shard``: None = shard whenever a process group is initialised; False = this rank infers ALL tiles of ITS scene and no
    collective is entered (one scene per rank: ranks may hold different scenes with different tile counts)."""
    from .parallel import sharded_map
    C_, H, W = x.shape
    rects = scene_tiles(H, W, tile, halo, strips)

    def run(my):
        cores = torch.zeros((my.shape[0], tile, W if strips else tile), dtype=torch.float32, device=x.device)
        by_shape = {}
        for i, r in enumerate(my.tolist()):
            by_shape.setdefault((r[5] - r[4], r[7] - r[6]), []).append((i, r))
        for items in by_shape.values():
            for k in range(0, len(items), batch):
                chunk = items[k:k + batch]
                xb = torch.stack([x[:, r[4]:r[5], r[6]:r[7]] for _, r in chunk]).contiguous()
                lg = model(xb)
                for j, (i, r) in enumerate(chunk):
                    cores[i, :r[1] - r[0], :r[3] - r[2]] = lg[j, 0, r[0] - r[4]:r[1] - r[4], r[2] - r[6]:r[3] - r[6]]
        return cores

    cores = run(rects) if shard is False else sharded_map(run, rects, group=group)
    return stitch(cores, rects, H, W)


def _merge_column_shards(t, c0, c1, group=None):
    """every rank filtered the column blocks [c0, c1) it owns: merged by OWNERSHIP -- a rank zeroes the columns it does not own
    and the ranks SUM, so the result does not depend on how the values compare with the fill value (x + 0 + ... + 0 == x
    exactly, fill pixels inside an owned block stay fill)"""
    import torch.distributed as dist
    t[:, :c0] = 0
    t[:, c1:] = 0
    if dist.get_backend(group) == "gloo" and t.is_cuda:
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


@torch.no_grad()
def emit_scene_predict(model, raw, wavelengths, template, fill_value=-9999.0, column_step=2, num_iter=30,
                       covariance_lerp_alpha=1e-4, column_range=None, tile=None, halo=RECEPTIVE_HALO, ratio_bands=None,
                       distributed=None, group=None, strips=True, georeferenced=False, glt_x=None, glt_y=None):
    """``raw``: (rows, cols, S) float32 EMIT L1B radiance (device or host), ``wavelengths``: (S,) nm, ``template``: unit CH4
    absorption for the bands inside [2122, 2488] nm (``mag1c.generate_template_from_bands``; (K,) or (K, 2)).
    Returns a dict of device tensors: ``mf`` (rows, cols) ppm*m, ``albedo``, ``input`` (4, H', W') in the AVIRIS value range,
    ``prediction`` (H', W') plume probability and ``pred_binary`` (int64) -- H', W' = rows, cols cropped to multiples of 32
    (emit_dataset.py:80-93).

    ``tile``: None = one whole-scene forward (the reference's only mode); an int = sliding-window inference with ``halo``
    (:func:`tiled_logits`): full-width strips of ``tile`` rows (``strips=True``, the throughput mode: (tile + 2 halo) / tile of the
    scene's work -- 2.25x at 512 / 320 against 5x for square cores, measured 2.6x vs 6.8x wall time on 1280 x 1248) or
    ``tile`` x ``tile`` cores.  ``ratio_bands=(2350, 2310)`` additionally returns ``ratio``, the
    on-the-fly two-band ratio of feature_extration.py:42-56 on the nearest bands (absorbing, reference).
    With ``torch.distributed`` initialised (``distributed=None`` -> automatic) the column blocks of the matched filter and the
    inference tiles are partitioned over the ranks; the per-rank mf / albedo columns are merged (one all_reduce) before the
    network input is built, so every rank returns the full-scene result.  ``column_range=(c0, c1)`` (explicit manual shard,
    c0 / c1 on column_step boundaries) returns ONLY ``mf`` and ``albedo`` of that shard: a network input built from a partial
    mf would be wrong for the whole scene.
    ``georeferenced=True`` (with the granule's ``glt_x`` / ``glt_y``) orthorectifies the products: see
    :func:`georeference_products`."""
    if georeferenced and (glt_x is None or glt_y is None):
        raise ValueError("emit_scene_predict: georeferenced=True needs glt_x and glt_y")
    raw = torch.as_tensor(raw)
    dev = raw.device if raw.is_cuda else model.device
    raw = raw.to(dev).float()
    w = np.asarray(wavelengths, dtype=np.float64)
    keep = np.nonzero((w >= EMIT_MAG1C_RANGE_NM[0]) & (w <= EMIT_MAG1C_RANGE_NM[1]))[0]
    assert keep.size and np.all(np.diff(keep) == 1), "the mag1c bands must be contiguous"
    sub = raw[..., int(keep[0]):int(keep[-1]) + 1].contiguous()
    rgb = raw[..., nearest_bands(w)].permute(2, 0, 1).contiguous()
    ratio = None
    if ratio_bands is not None:
        ia, ir = nearest_bands(w, ratio_bands)
        ratio = (raw[..., ia].contiguous(), raw[..., ir].contiguous())
    out = _emit_predict_parts(model, sub, rgb, ratio, template, fill_value, column_step, num_iter, covariance_lerp_alpha, column_range,
                              tile, halo, distributed, group, strips)
    return georeference_products(out, glt_x, glt_y, fill_value) if georeferenced else out


ORTHO_PRODUCTS = ("mf", "albedo", "prediction", "ratio", "pred_binary")


def georeference_products(out, glt_x, glt_y, fill_value=-9999.0):
    """Orthorectifies the 2-D products of an EMIT prediction dict through the granule's GLT (what ``georreferenced=True`` does to
    the outputs of the reference's ``mag1c_emit``, mag1c_emit.py:86-88, extended to everything the notebook plots): ``mf``,
    ``albedo``, ``prediction``, ``ratio`` and the three RGB planes of the network input (read in place from ``input[1:4]``, new key
    ``rgb``) go through ONE ``sc_glt_ortho`` call (float32, no-data = ``fill_value``), ``pred_binary`` (int64, no-data = 0: not a
    plume) through a second one -- one call per dtype, the GLT uploaded once.  The network output covers the swath cropped to
    multiples of 32; GLT entries beyond it are no-data.  The sensor-geometry tensors stay in the dict under ``<key>_raw``;
    ``input`` stays in sensor geometry."""
    from .ortho import georeference
    swath = tuple(out["mf"].shape)
    dev = out["mf"].device
    gx = torch.from_numpy(np.ascontiguousarray(glt_x, dtype=np.int32)).to(dev) if not isinstance(glt_x, torch.Tensor) else glt_x
    gy = torch.from_numpy(np.ascontiguousarray(glt_y, dtype=np.int32)).to(dev) if not isinstance(glt_y, torch.Tensor) else glt_y
    by_dtype = {}
    for k in ORTHO_PRODUCTS:
        if out.get(k) is not None:
            by_dtype.setdefault(out[k].dtype, []).append(k)
    res = dict(out)
    for dt, keys in by_dtype.items():
        planes = [out[k] for k in keys]
        rgb = dt == torch.float32 and out.get("input") is not None
        if rgb:
            planes += list(out["input"][1:4].unbind(0))
        fill = 0 if dt == torch.int64 else fill_value
        geo = georeference(planes, gx, gy, fill_value_default=fill, shape=swath)
        for i, k in enumerate(keys):
            res[k + "_raw"], res[k] = out[k], geo[i]
        if rgb:
            res["rgb"] = geo[len(keys):]
    return res


def _emit_predict_parts(model, sub, rgb, ratio, template, fill_value, column_step, num_iter, covariance_lerp_alpha, column_range, tile, halo,
                        distributed, group, strips=True):
    """``sub``: (rows, cols, K) device float32 radiance of the mag1c bands, ``rgb``: (3, rows, cols), ``ratio``: None or the
    (absorbing, reference) band planes -- the pieces of the cube the scene pipeline touches"""
    import torch.distributed as dist
    t = np.asarray(template, dtype=np.float64)
    t = t[:, 1] if t.ndim == 2 else t
    if t.size != sub.shape[-1]:
        raise ValueError(f"template has {t.size} bands, the cube has {sub.shape[-1]} inside {EMIT_MAG1C_RANGE_NM} nm")
    if distributed is None:
        distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    cols = sub.shape[1]
    step = int(column_step or cols)
    if column_range is not None:
        mf, alb = mag1c.mag1c_columns(sub, t, fill_value, column_step=column_step, num_iter=num_iter,
                                      covariance_lerp_alpha=covariance_lerp_alpha, column_range=column_range)
        return {"mf": mf, "albedo": alb}
    if distributed:
        from .parallel import shard_range
        nblk = -(-cols // step)
        lo, hi = shard_range(nblk, dist.get_rank(group), dist.get_world_size(group))
        c0, c1 = lo * step, min(hi * step, cols)
        mf, alb = mag1c.mag1c_columns(sub, t, fill_value, column_step=column_step, num_iter=num_iter,
                                      covariance_lerp_alpha=covariance_lerp_alpha, column_range=(c0, c1))
        mf, alb = _merge_column_shards(mf, c0, c1, group), _merge_column_shards(alb, c0, c1, group)
    else:
        mf, alb = mag1c.mag1c_columns(sub, t, fill_value, column_step=column_step, num_iter=num_iter,
                                      covariance_lerp_alpha=covariance_lerp_alpha)
    x = emit_to_aviris_input(mf, rgb)
    out = {"mf": mf, "albedo": alb, "input": x}
    if ratio is not None:
        from .features import ratio_2c_match_c_from_sums_outlier
        out["ratio"] = ratio_2c_match_c_from_sums_outlier(ratio[0], ratio[1])
    was = model.training
    model.eval()
    try:
        logits = model(x[None]) if tile is None else tiled_logits(model, x, tile, halo, group=group, shard=bool(distributed), strips=strips)[None, None]
        masks = masks_from_logits(logits.contiguous())
    finally:
        model.train(was)
    out["prediction"], out["pred_binary"] = masks["prediction"][0, 0], masks["pred_binary"][0, 0]
    return out


@torch.no_grad()
def emit_granule_predict(model, nc_path, column_step=2, num_iter=30, covariance_lerp_alpha=1e-4, tile=None, halo=RECEPTIVE_HALO,
                         ratio_bands=None, distributed=None, group=None, rows=None, threads=8, strips=True, georeferenced=False,
                         out_folder=None, geotransform=None, overwrite=False, plumes=False, plume_outlines=False,
                         label_polygons=None, cog=False, crs=None, resolution=None, resampling="nearest", label_crs=None,
                         mask_resampling="nearest", clean=None, match_tolerance_px=0.0,
                         plume_background=None, plume_quantify=None):
    """The notebook path of the reference end to end FROM THE FILE (notebooks/inference_on_raw_EMIT_nc_file.ipynb cells 8-19:
    ``EMITImage(path)`` -> ``mag1c_emit`` -> RGB bands -> rescale -> ``model`` -> threshold): opens the EMIT L1B radiance granule
    (NetCDF-4) with :mod:`starcop_amd.hdf5_reader`, reads ONLY what the pipeline touches -- the contiguous band slice inside
    [2122, 2488] nm chunk-wise, the three RGB band planes, the two ratio bands if asked for: ~0.35 GB of the 1.8 GB cube -- builds the
    CH4 target from the file's band centres / widths (shipped look-up table) and runs :func:`emit_scene_predict`'s device pipeline.
    ``rows``: optional slice of downtrack lines.  Returns its dict plus ``wavelengths``, ``fwhm`` (the mag1c bands) and ``glt_x`` /
    ``glt_y`` (host arrays, or None).

    ``georeferenced=True`` orthorectifies the products through that GLT on the device (:func:`georeference_products`: the
    sensor-geometry tensors move to ``<key>_raw``, ``rgb`` is added); the file must carry a GLT and ``rows`` must be None (the
    GLT indexes the whole granule).  With ``out_folder`` (only with ``georeferenced=True``) the orthorectified products are
    written as tiled GeoTIFFs (BLOCKSIZE 128): ``mag1c.tif``, ``albedo.tif``, ``pred.tif`` (float32, GDAL_NODATA = the fill
    value), ``predbinary.tif`` (uint8) and ``rgb.tif`` (3 bands, the RGB planes of the network input), with band descriptions
    and the georeferencing of :func:`starcop_amd.ortho.emit_geo_tags` from the file's root attributes ``geotransform`` /
    ``spatial_ref`` -- ``geotransform=`` overrides the attribute; with neither, the files carry no georeferencing and one warning
    is issued.  Existing files are skipped unless ``overwrite=True``; the paths written are returned under ``files``.

    ``plumes=True`` adds ``plumes``, the :func:`starcop_amd.plumes.plume_table` of ``pred_binary`` with ``mf`` as mag1c and
    ``prediction`` as probability -- on the orthorectified products (with ``x`` / ``y`` from the geotransform, when there is one)
    if ``georeferenced=True``, on the sensor-geometry ones otherwise; pixels that carry the fill value or are not finite do not
    count.  With ``out_folder`` the table is also written as ``plumes.csv`` (same ``overwrite`` rule) and listed in ``files``.
    ``plume_outlines=True`` (with ``plumes=True``) adds ``plume_outlines``, the :func:`starcop_amd.plumes.plume_outlines` of the same
    mask in the same coordinates, and with ``out_folder`` writes ``plumes.geojson``, one Polygon per row of the table.

    ``label_polygons`` (a ``.geojson`` path for :func:`starcop_amd.plumes.read_plumes`, or polygons as
    :func:`starcop_amd.plumes.rasterize_polygons` takes them, in the coordinates of the geotransform; needs ``georeferenced=True``,
    there is no grid to burn into otherwise) adds ``label_mask``, the polygons burnt into the product grid (device uint8), and
    ``plume_match``, :func:`starcop_amd.plumes.match_plumes_polygons` of ``pred_binary`` against them; with ``out_folder`` the
    mask is written as ``label.tif`` like ``predbinary.tif``.

    ``cog=True`` (or a dict of :func:`starcop_amd.cog.write_cog` keyword arguments) writes every raster as a Cloud-Optimized
    GeoTIFF -- tiled, with an overview pyramid, empty tiles left out -- straight from the device tensors; the default leaves the
    files as they were.

    ``crs`` (with ``georeferenced=True``; ``"utm"`` = the WGS-84 UTM zone of the centre of the orthorectified grid, or an EPSG
    code: 326zz / 327zz / 4326) warps the orthorectified products from the granule's longitude / latitude grid onto the north-up
    :func:`starcop_amd.warp.suggest_grid` of that CRS at ``resolution`` (its units; default: the pixel count along the diagonal is
    kept) through :func:`starcop_amd.products.regrid`: ``pred_binary`` by ``mask_resampling`` (``"nearest"``, or ``"mode"`` / ``"max"``
    / ``"min"`` over the pixel's footprint), the float32 products by ``resampling`` (``"nearest"`` / ``"bilinear"``, for a
    ``resolution`` coarser than the granule's ``"average"`` / ``"max"`` / ``"min"`` over the footprint, or {key: mode}), no-data =
    the fill value.  The files then carry the tags of that grid
    (:func:`starcop_amd.warp.geo_tags`), ``plumes`` has ``x`` / ``y`` in its units and -- for a UTM zone -- ``ime_ppmm_m2`` with
    the pixel area ``resolution ** 2``; ``geotransform`` and ``crs`` of the new grid are added to the dict.  ``label_polygons``
    are taken in the output CRS unless ``label_crs`` names another, in which case they go through
    :func:`starcop_amd.warp.transform_polygons`.  The default ``crs=None`` changes nothing.

    ``clean`` (with ``georeferenced=True``): a dict of :func:`starcop_amd.products.clean` keyword arguments -- ``open_radius``,
    ``min_area``, ``exclude``, ``exclude_buffer_px``, ``connectivity`` -- applied to ``pred_binary`` on the product grid (after the
    regrid) and before the annotations and the files, which then all describe the cleaned mask; ``out["clean"]`` has the pixel
    counts.  ``match_tolerance_px``: the ``tolerance_px`` of the match against ``label_polygons``.  ``plume_background``
    (``{"ring_px": .., "gap_px": .., "stat": "mean" | "median"}``) adds the background-ring columns of ``plumes.plume_table`` to the plume table
    (``stat="median"``: its ``background_stat``, the ring median and the noise columns).
    ``plume_quantify`` (the ``quantify=`` dict of ``plumes.plume_table``: ``wind_speed_m_s``, ...) adds its shape, mass and
    emission-rate columns to the plume table, ``plumes.csv`` and the GeoJSON properties; it needs mag1c and a metric grid
    (``crs="utm"``: on the granule's longitude / latitude grid it is a ValueError).  The defaults add nothing."""
    from .hdf5_reader import H5File
    products.check_clean(clean, "emit_granule_predict")
    products.check_plume_background(plume_background, "emit_granule_predict")
    products.check_plume_quantify(plume_quantify, "emit_granule_predict")
    if clean is not None and not georeferenced:
        raise ValueError("emit_granule_predict: clean works on the orthorectified products; pass georeferenced=True")
    if crs is not None and not georeferenced:
        raise ValueError("emit_granule_predict: crs warps the orthorectified products; pass georeferenced=True")
    if label_crs is not None and crs is None:
        raise ValueError("emit_granule_predict: label_crs needs crs= (without it the polygons are taken in the granule's own coordinates)")
    if out_folder is not None:
        if str(out_folder).startswith("gs://"):
            raise NotImplementedError(f"{out_folder}: writing to Google Cloud Storage is not supported")
        if not georeferenced:
            raise ValueError("emit_granule_predict: out_folder writes the orthorectified products; pass georeferenced=True")
    if plume_outlines and not plumes:
        raise ValueError("emit_granule_predict: plume_outlines=True needs plumes=True")
    if label_polygons is not None and not georeferenced:
        raise ValueError("emit_granule_predict: label_polygons are burnt into the orthorectified grid; pass georeferenced=True")
    if georeferenced and rows is not None:
        raise ValueError("emit_granule_predict: georeferenced=True needs the whole granule (rows=None): the GLT indexes all of its lines")
    dev = model.device
    rs = rows or slice(None)
    with H5File(nc_path) as f:
        wl = np.asarray(f["sensor_band_parameters/wavelengths"].read(), dtype=np.float64)
        fwhm = np.asarray(f["sensor_band_parameters/fwhm"].read(), dtype=np.float64)
        rad = f["radiance"]
        keep = np.nonzero((wl >= EMIT_MAG1C_RANGE_NM[0]) & (wl <= EMIT_MAG1C_RANGE_NM[1]))[0]
        assert keep.size, "There are no bands in the selected wavelength range"
        b0, b1 = int(keep[0]), int(keep[-1]) + 1
        fill = rad.attrs.get("_FillValue", rad.fillvalue)
        fill = float(fill) if fill is not None else -9999.0

        def plane(i):
            return np.ascontiguousarray(rad.read((rs, slice(None), slice(i, i + 1)), threads=threads)[..., 0], dtype=np.float32)
        sub_h = np.ascontiguousarray(rad.read((rs, slice(None), slice(b0, b1)), threads=threads), dtype=np.float32)
        rgb_h = np.stack([plane(i) for i in nearest_bands(wl)])
        ratio_h = [plane(i) for i in nearest_bands(wl, ratio_bands)] if ratio_bands is not None else None
        glt = (f["location/glt_x"].read(), f["location/glt_y"].read()) if ("location/glt_x" in f and "location/glt_y" in f) else (None, None)
        root = f.attrs("/") if out_folder is not None or crs is not None or ((plumes or label_polygons is not None) and georeferenced) else {}
    if georeferenced and glt[0] is None:
        raise ValueError(f"{nc_path}: no location/glt_x, location/glt_y to orthorectify with")
    template = mag1c.generate_template_from_bands(wl[b0:b1], fwhm[b0:b1])
    ratio = tuple(_upload_pinned(a, dev) for a in ratio_h) if ratio_h else None
    out = _emit_predict_parts(model, _upload_pinned(sub_h, dev), _upload_pinned(rgb_h, dev), ratio, template, fill, column_step,
                              num_iter, covariance_lerp_alpha, None, tile, halo, distributed, group, strips)
    if georeferenced:
        out = georeference_products(out, glt[0], glt[1], fill)
    out.update(wavelengths=wl[b0:b1], fwhm=fwhm[b0:b1], glt_x=glt[0], glt_y=glt[1], fill_value=fill)
    gt = geotransform if geotransform is not None else root.get("geotransform")
    geo = area = None
    if crs is not None:
        import os
        from . import warp
        from .ortho import emit_geo_tags
        if gt is None:
            raise ValueError("emit_granule_predict: crs needs the grid of the orthorectified products: the granule has no geotransform "
                             "attribute and none was passed")
        emit_geo_tags(gt, root.get("spatial_ref"))                        # refuses a granule that is not on a WGS-84 lon / lat grid
        gt = [float(v) for v in np.asarray(gt, dtype=np.float64).ravel()]
        if crs == "utm":
            h, w = out["mf"].shape
            crs = warp.utm_crs_for(*(float(v) for v in warp.apply_geotransform(gt, w / 2.0, h / 2.0)))
        gt, crs, area = products.regrid(out, gt, 4326, int(crs), resolution, resampling, fill, mask_resampling=mask_resampling)
        geo = warp.geo_tags(gt, crs)
        out.update(geotransform=gt, crs=crs)
        if label_polygons is not None and label_crs is not None:
            if isinstance(label_polygons, (str, os.PathLike)):
                from .plumes import read_plumes
                label_polygons = read_plumes(label_polygons)[1]
            label_polygons = warp.transform_polygons(label_polygons, label_crs, crs)
    mf = prob = None
    if plumes:
        # pixels that carry the fill value become NaN, which the per-plume statistics leave out; in sensor geometry the network
        # output covers the swath cropped to multiples of 32 (its top-left part): mf is cropped to it
        nan = torch.tensor(float("nan"), device=out["mf"].device)
        h, w = out["pred_binary"].shape
        mf = out["mf"][:h, :w]
        mf, prob = torch.where(mf == fill, nan, mf), torch.where(out["prediction"] == fill, nan, out["prediction"])
    if clean is not None:
        products.clean(out, **clean)
    products.annotate(out, out["pred_binary"], mf, prob, gt if georeferenced else None, area, plumes, plume_outlines, label_polygons,
                      match_tolerance_px, plume_background, plume_quantify)
    if out_folder is not None:
        from .ortho import emit_geo_tags
        if geo is None:
            geo = emit_geo_tags(gt, root.get("spatial_ref")) if gt is not None else {}
        out["files"] = products.write_rasters(
            out, products.EMIT_RASTERS, str(out_folder), overwrite, geo, fill, {"wavelengths": out["wavelengths"], "mag1c": "acrwl1mf"}, cog,
            "emit_granule_predict: the granule has no geotransform attribute and none was passed: the GeoTIFFs are written without georeferencing")
        out["files"] += products.write_annotations(out, str(out_folder), overwrite, geo, cog)
    return out


@torch.no_grad()
def aviris_scene_mag1c(aviris_img_folder, mf_filename, albedo_filename=None, use_wavelength_range=mag1c.DEFAULT_WAVELENGTH_RANGE,
                       device="cuda", extra_tags=None):
    """``run_mag1c`` of the reference (starcop/process_aviris.py:146-232) on the MI355X: opens ``<name>_img`` (radiance, ENVI)
    and ``<name>_glt`` (sample / line look-up, ENVI) of an AVIRIS-NG flight line as BIP memmaps, keeps the bands that are not
    affected by water vapour inside ``use_wavelength_range`` (they must form a slice), builds the CH4 target from the header's
    band centres and widths, runs acrwl1mf(num_iter=30) per detector sample (groups = |GLT sample index|, pixels with index 0
    are not data) and writes the result as tiled GeoTIFFs (BLOCKSIZE 128) that carry what the reference's ``save_cog`` call leaves
    in them (process_aviris.py:179-181,219-232): the radiance file's georeferencing (ENVI ``map info`` -> GeoTIFF transform + CRS
    keys), GDAL_NODATA, the band description and the dataset tags ``wavelengths`` (the kept band centres) and ``mag1c=acfwl1mf``.
    The target spectrum is cast to the radiance dtype as the reference does (:199).  Returns (mf, albedo) device tensors.
    The radiance slice is uploaded once from the memmap through pinned memory; everything after that stays on the device."""
    from . import io_formats as io
    mf, alb, meta, md = _aviris_mag1c(aviris_img_folder, use_wavelength_range, device)
    geo = io.envi_geo_tags(meta["header"])                                # transform + crs of the radiance file
    for row, path, image in ((products.MAG1C, mf_filename, mf), (products.ALBEDO, albedo_filename, alb)):
        if path is not None:                                              # GDAL_NODATA, as fill_value_default=NODATA
            products.write_raster(path, image, products.raster_tags(row, geo, mag1c.NODATA, md, extra_tags))
    return mf, alb


def _aviris_mag1c(aviris_img_folder, use_wavelength_range, device):
    """the matched filter of :func:`aviris_scene_mag1c` without the files -> (mf, albedo, ENVI meta, the dataset tags of its products)"""
    import os
    from . import io_formats as io
    folder = aviris_img_folder.rstrip("/")
    name = os.path.basename(folder)
    rdn, meta = io.open_envi(os.path.join(folder, f"{name}_img"))
    glt, _ = io.open_envi(os.path.join(folder, f"{name}_glt"))
    wl = meta["wavelengths"]
    keep = mag1c.get_mask_bad_bands(wl) & (wl >= use_wavelength_range[0]) & (wl <= use_wavelength_range[1])
    idx = np.flatnonzero(keep)
    assert idx[-1] - idx[0] + 1 == idx.shape[0], "Not all indexes included. Can't be a slice!"
    target = mag1c.generate_template_from_bands(centers=wl, fwhm=meta["fwhm"])
    spec = target.astype(rdn.dtype)[keep, 1]           # process_aviris.py:199: the template in the cube's dtype
    x = _upload_pinned(np.ascontiguousarray(rdn[..., idx[0]:idx[-1] + 1], dtype=np.float32), device)
    groups = np.abs(np.asarray(glt[..., 0])).astype(np.int64)
    mf, alb = mag1c.func_by_groups(mag1c.Filter(spec, num_iter=30), x, groups, mask=groups != 0, max_group=int(groups.max()))
    return mf, alb, meta, {"wavelengths": wl[keep], "mag1c": "acfwl1mf"}


def aviris_scene_products(input_products, normalize_by_acquisition_date=True):
    """what :func:`aviris_scene_predict` reads for a model's ``input_products``: [("mag1c", None) | ("band", centre in nm)].
    ``mag1c`` is the matched filter; ``TOA_AVIRIS_{w}nm`` (``{w}nm`` when not normalising by the acquisition date) the radiance
    band nearest to ``w`` nm, the names ``window_dataset.save_name`` gives them.  Anything else: NotImplementedError."""
    import re
    pat = r"TOA_AVIRIS_(\d+(?:\.\d+)?)nm" if normalize_by_acquisition_date else r"(\d+(?:\.\d+)?)nm"
    out = []
    for name in input_products:
        m = re.fullmatch(pat, name)
        if name == "mag1c":
            out.append(("mag1c", None))
        elif m:
            out.append(("band", float(m.group(1))))
        else:
            raise NotImplementedError(f"aviris_scene_predict: input product {name!r} cannot be derived from an AVIRIS-NG flight line "
                                      f"(mag1c and {'TOA_AVIRIS_{w}nm' if normalize_by_acquisition_date else '{w}nm'} can)")
    return out


def _envi_geotransform(header):
    """(GDAL geotransform, pixel area in m2) of an ENVI ``map info`` without rotation; (None, None) otherwise.  The area only
    for UTM (metres)."""
    mi = header.get("map info")
    if not isinstance(mi, list) or len(mi) < 7:
        return None, None
    try:
        xr, yr, e0, n0, px, py = (float(v) for v in mi[1:7])
    except ValueError:
        return None, None
    if any(v.lower().replace(" ", "").startswith("rotation=") and float(v.split("=")[1]) != 0.0 for v in mi[7:]):
        return None, None
    return (e0 - (xr - 1.0) * px, px, 0.0, n0 + (yr - 1.0) * py, 0.0, -py), (px * py if mi[0].strip().lower() == "utm" else None)


@torch.no_grad()
def aviris_scene_predict(model, aviris_img_folder, out_folder=None, mag1c_path=None, toa_correction_factor=None, solar_altitude=None,
                         normalize_by_acquisition_date=True, tile=None, halo=None, batch=None, plumes=False, overwrite=False,
                         device="cuda", plume_outlines=False, label_polygons=None, cog=False, north_up=False, resolution=None,
                         resampling="nearest", mask_resampling="nearest", clean=None, match_tolerance_px=0.0,
                         plume_background=None, plume_quantify=None):
    """An orthorectified AVIRIS-NG flight line through the plume model, file to file: ``{folder}/{name}_img`` (ENVI radiance,
    float32) -> the network's input products -> ``model.predict_scene`` -> (with ``out_folder``) ``pred.tif`` / ``predbinary.tif``.

    The channels follow ``model.input_products`` (:func:`aviris_scene_products`).  ``mag1c`` is read from ``mag1c_path``, else
    from ``{folder}/mag1c.tif`` when it exists, else computed as :func:`aviris_scene_mag1c` does (needs ``{name}_glt``; written to
    ``{out_folder}/mag1c.tif`` when ``out_folder`` is given); its no-data pixels enter the network as 0 and it is clipped to
    [0, 10000] (``window_dataset.product_ops``).  A radiance band is the band of the cube whose centre is nearest to the product's
    wavelength, as ``WindowDataset`` picks it: the bands are read from the memmap as one strided host read, uploaded as ONE pinned
    (H, W, k) buffer and read in place; the header's ``data ignore value`` enters as 0, everything else is multiplied by the
    acquisition-date factor -- ``toa_correction_factor``, or ``aviris.observation_date_correction_factor(date, solar_altitude)``
    with the date parsed from the ``angYYYYMMDDtHHMMSS`` folder name; with ``normalize_by_acquisition_date`` and neither: ValueError.

    Returns the dict of ``predict_scene`` (device tensors) plus ``mf``; ``plumes=True`` adds ``plumes``, the
    ``plumes.plume_table`` of the mask with ``mf`` and ``prediction`` and the geotransform / pixel area of the ENVI ``map info``.
    With ``out_folder``: ``pred.tif`` (float32, GDAL_NODATA = ``mag1c.NODATA``) and ``predbinary.tif`` (uint8), BLOCKSIZE 128, the
    radiance file's georeferencing, band descriptions; ``plumes.csv`` with ``plumes=True``; existing files are skipped unless
    ``overwrite``; the paths written come back under ``files``.  ``plume_outlines=True`` (with ``plumes=True``) adds
    ``plume_outlines``, the ``plumes.plume_outlines`` of the mask with the same geotransform, and writes ``plumes.geojson``, one
    Polygon per row of the table, next to ``plumes.csv``.  ``label_polygons`` (a ``.geojson`` path for ``plumes.read_plumes``, or
    polygons as ``plumes.rasterize_polygons`` takes them, in the coordinates of the ``map info``) adds ``label_mask``, the
    polygons burnt into the flight line's grid (device uint8), and ``plume_match``, the ``plumes.match_plumes_polygons`` of the
    mask against them, and writes ``label.tif`` like ``predbinary.tif``.

    ``cog=True`` (or a dict of :func:`starcop_amd.cog.write_cog` keyword arguments) writes every raster of the call --
    ``pred.tif``, ``predbinary.tif``, ``label.tif`` and a ``mag1c.tif`` it computes -- as a Cloud-Optimized GeoTIFF straight from
    the device tensor: tiles, overviews (average for float32, mode for uint8) and the search for empty tiles run on the device.
    The default leaves every byte of the files as it was.

    ``north_up=True``: a line whose ``map info`` carries a ``rotation=`` has no north-up geotransform, so by default its plume
    table has no ``x`` / ``y``, its outlines are in pixels and ``label_polygons`` cannot be burnt.  With this flag ``prediction``,
    ``pred_binary`` and ``mf`` of such a line are warped (same CRS, ``nearest``: :func:`starcop_amd.products.regrid`) onto the
    north-up :func:`starcop_amd.warp.suggest_grid` at the line's own pixel size before the annotations are made; ``pred.tif``,
    ``predbinary.tif`` and ``label.tif`` carry that grid (a ``mag1c.tif`` the call computes stays on the line's grid, where
    the next run reads it) and ``geotransform`` / ``crs`` are added to the dict.  A line without rotation is left as it is.

    ``resolution`` (with ``north_up=True``; the units of the ``map info``): the three products are put on the north-up grid at THAT
    pixel size, whether or not the line is rotated -- a 5 m line on a 60 m grid, say -- the float32 ones by ``resampling`` and
    ``pred_binary`` by ``mask_resampling`` (:func:`starcop_amd.products.regrid`; on a coarser grid the footprint modes
    ``"average"`` / ``"max"`` / ``"min"`` and ``"mode"`` / ``"max"`` / ``"min"``).  The plume table then has its areas and
    ``ime_ppmm_m2`` with the new pixel area.  ``resolution=None`` with the default modes is the behaviour described above.

    ``clean``: a dict of :func:`starcop_amd.products.clean` keyword arguments (``open_radius``, ``min_area``, ``exclude``,
    ``exclude_buffer_px``, ``connectivity``), applied to ``pred_binary`` after the regrid and before the annotations and the
    files: ``predbinary.tif``, ``plumes.csv``, ``plumes.geojson`` and ``plume_match`` describe the cleaned mask, ``pred.tif`` is
    untouched, ``out["clean"]`` has the pixel counts.  ``match_tolerance_px``: the ``tolerance_px`` of the match against
    ``label_polygons``.  ``plume_background``
    (``{"ring_px": .., "gap_px": .., "stat": "mean" | "median"}``) adds the background-ring columns of ``plumes.plume_table`` to the plume table
    (``stat="median"``: its ``background_stat``, the ring median and the noise columns).
    ``plume_quantify`` (the ``quantify=`` dict of ``plumes.plume_table``: ``wind_speed_m_s``, ...) adds its shape, mass and
    emission-rate columns to the plume table, ``plumes.csv`` and the GeoJSON properties; it needs mag1c and a metric grid
    (a UTM ``map info``).  The defaults add nothing and change no byte."""
    import datetime
    import os
    import re
    from . import aviris
    from . import io_formats as io
    from .sampling import _nodata
    if plume_outlines and not plumes:
        raise ValueError("aviris_scene_predict: plume_outlines=True needs plumes=True")
    products.check_clean(clean, "aviris_scene_predict")
    products.check_plume_background(plume_background, "aviris_scene_predict")
    products.check_plume_quantify(plume_quantify, "aviris_scene_predict")
    if not north_up and (resolution is not None or resampling != "nearest" or mask_resampling != "nearest"):
        raise ValueError("aviris_scene_predict: resolution, resampling and mask_resampling regrid the products; pass north_up=True")
    inputs = aviris_scene_products(model.input_products, normalize_by_acquisition_date)
    for path in (out_folder, mag1c_path, aviris_img_folder):
        if path is not None and str(path).startswith("gs://"):
            raise NotImplementedError(f"{path}: Google Cloud Storage is not supported; pass a local path")
    folder = str(aviris_img_folder).rstrip("/")
    name = os.path.basename(folder)
    factor = None
    if normalize_by_acquisition_date and any(kind == "band" for kind, _ in inputs):
        if toa_correction_factor is not None:
            factor = float(toa_correction_factor)
        elif solar_altitude is not None:
            m = re.search(r"ang(\d{8})t(\d{6})", name)
            if m is None:
                raise ValueError(f"aviris_scene_predict: no acquisition date (angYYYYMMDDtHHMMSS) in the folder name {name!r}; pass toa_correction_factor=")
            when = datetime.datetime.strptime(m.group(1) + m.group(2), "%Y%m%d%H%M%S").replace(tzinfo=datetime.timezone.utc)
            factor = float(aviris.observation_date_correction_factor(when, float(solar_altitude)))
        else:
            raise ValueError("aviris_scene_predict: the acquisition-date factor needs toa_correction_factor= or solar_altitude= (degrees; "
                             "aviris.observation_date_correction_factor), or normalize_by_acquisition_date=False")
    rdn, meta = io.open_envi(os.path.join(folder, f"{name}_img"))
    if meta["wavelengths"] is None:
        raise ValueError(f"{folder}/{name}_img: the ENVI header has no wavelengths")
    if rdn.dtype.itemsize != 4 or rdn.dtype.kind != "f":
        raise NotImplementedError(f"{folder}/{name}_img: {rdn.dtype} radiance is not supported (float32)")
    header = meta["header"]
    ignore = header.get("data ignore value")
    ignore = float(ignore) if ignore is not None else None
    dev = torch.device(device)
    files, geo = [], io.envi_geo_tags(header) if out_folder is not None else None
    # ---- the planes, in the order of input_products
    centres = [w for kind, w in inputs if kind == "band"]
    cube = None
    if centres:
        bands = np.argmin(np.abs(np.asarray(centres, dtype=np.float64)[:, None] - meta["wavelengths"]), axis=1)
        cube = _upload_pinned(np.ascontiguousarray(rdn[:, :, bands], dtype=np.float32), dev)     # one strided read of the memmap
    mf, mf_fill = None, float(mag1c.NODATA)
    if any(kind == "mag1c" for kind, _ in inputs):
        path = mag1c_path if mag1c_path is not None else os.path.join(folder, "mag1c.tif")
        if mag1c_path is not None or os.path.exists(path):
            info = io.tiff_info(path)
            a = io.read_tiff(path, info=info)
            a = a[0] if a.ndim == 3 else a
            if a.dtype != np.float32:
                raise ValueError(f"{path}: mag1c must be float32, got {a.dtype}")
            nod = _nodata(info)
            mf_fill = float(nod) if nod is not None else mf_fill
            mf = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        else:
            mf, _, _, md = _aviris_mag1c(folder, mag1c.DEFAULT_WAVELENGTH_RANGE, dev)
            if out_folder is not None:
                files += products.write_rasters({"mf": mf}, (products.MAG1C,), str(out_folder), overwrite, geo, mag1c.NODATA, md, cog)
        if tuple(mf.shape) != tuple(rdn.shape[:2]):
            raise ValueError(f"aviris_scene_predict: mag1c is {tuple(mf.shape)}, the radiance {tuple(rdn.shape[:2])}")
    planes, fills, scales, clips = [], [], [], []
    j = 0
    for kind, _ in inputs:
        if kind == "mag1c":
            planes.append(mf); fills.append(mf_fill); scales.append(None); clips.append((0.0, 10_000.0))
        else:
            planes.append(cube[:, :, j]); fills.append(ignore); scales.append(factor); clips.append(None)
            j += 1
    out = model.predict_scene(planes, fill_value=fills, scales=scales, clips=clips, tile=tile, halo=halo, batch=batch)
    out["mf"] = mf
    gt, area = _envi_geotransform(header)
    full, epsg, rotation = io.envi_geotransform(header) if north_up else (None, None, 0.0)
    if resolution is not None and full is None:
        raise ValueError("aviris_scene_predict: resolution needs the grid of the flight line: the header has no usable map info")
    if full is not None and (rotation != 0.0 or resolution is not None):
        from . import warp
        px, py = float(header["map info"][5]), float(header["map info"][6])
        if resolution is None and px != py:
            raise NotImplementedError(f"aviris_scene_predict: north_up with pixels of {px} x {py}: one pixel size per grid")
        gt, _, area = products.regrid(out, full, epsg, epsg, px if resolution is None else float(resolution), resampling,
                                      {"prediction": mag1c.NODATA, "mf": mf_fill}, keys=("prediction", "pred_binary", "mf"),
                                      mask_resampling=mask_resampling)
        mf = out["mf"]
        out.update(geotransform=gt, crs=epsg)
        if geo is not None:
            geo = warp.geo_tags(gt, epsg)
    if clean is not None:
        products.clean(out, **clean)
    products.annotate(out, out["pred_binary"], mf, out["prediction"], gt, area, plumes, plume_outlines, label_polygons, match_tolerance_px,
                      plume_background, plume_quantify)
    if out_folder is not None:
        files += products.write_rasters(out, products.AVIRIS_RASTERS, str(out_folder), overwrite, geo, mag1c.NODATA, cog=cog)
        out["files"] = files + products.write_annotations(out, str(out_folder), overwrite, geo, cog)
    return out


@torch.no_grad()
def mosaic_products(folders, out_folder, crs=None, resolution=None, rule="max", plumes=False, plume_outlines=False, label_polygons=None,
                    cog=False, overwrite=False, device="cuda", clean=None, match_tolerance_px=0.0,
                    plume_background=None, plume_quantify=None):
    """The product folders of N scenes -- what ``emit_granule_predict`` / ``aviris_scene_predict`` write -- composed into one:
    ``pred.tif``, ``predbinary.tif`` and, where every folder has one, ``mag1c.tif`` are read (``io_formats.read_tiff``; grid and
    CRS from the GeoTIFF tags, a file without them raises ValueError), put on the union grid of the scenes in ``crs`` (default:
    that of the first folder) at ``resolution`` by :func:`starcop_amd.products.mosaic` with ``rule`` on the probability, and written
    under the same names into ``out_folder``, with ``source.tif``: uint8, the number of the folder a pixel came from, 255 = none,
    the folder names in the GDAL metadata (``source_0``, ...).  ``plumes`` / ``plume_outlines`` / ``label_polygons`` add the files
    of ``products.write_annotations``, made on the mosaic: a plume in the overlap of two scenes is one row.  No-data of the float
    rasters is each file's GDAL_NODATA of the first folder (default -9999).  ``clean`` (a dict of :func:`starcop_amd.products.clean`
    keyword arguments) cleans the mosaicked mask before the annotations and the files; ``match_tolerance_px`` is the
    ``tolerance_px`` of the match against ``label_polygons``; ``plume_background`` (``{"ring_px": .., "gap_px": .., "stat": "mean" | "median"}``) adds the
    background-ring columns of ``plumes.plume_table`` (``stat="median"``: its ``background_stat``, the ring median and the noise
    columns) and needs the ``mf`` product among the folders';
    ``plume_quantify`` (the ``quantify=`` dict of ``plumes.plume_table``: ``wind_speed_m_s``, ...) adds its shape, mass and
    emission-rate columns to the plume table, ``plumes.csv`` and the GeoJSON properties; it needs mag1c and a metric grid
    (a UTM ``crs``).  -> the dict of ``products.mosaic`` with ``files``."""
    import os
    from . import io_formats as io
    from . import warp
    from .sampling import _nodata
    if plume_outlines and not plumes:
        raise ValueError("mosaic_products: plume_outlines=True needs plumes=True")
    products.check_clean(clean, "mosaic_products")
    products.check_plume_background(plume_background, "mosaic_products")
    products.check_plume_quantify(plume_quantify, "mosaic_products")
    folders = [str(f).rstrip("/") for f in folders]
    for path in folders + [out_folder]:
        if str(path).startswith("gs://"):
            raise NotImplementedError(f"{path}: Google Cloud Storage is not supported; pass a local path")
    if not folders:
        raise ValueError("mosaic_products: no folders")
    table = [products.PRED, products.PREDBINARY]
    if all(os.path.exists(os.path.join(f, products.MAG1C.name)) for f in folders):
        table.insert(0, products.MAG1C)
    dev = torch.device(device)
    outs, fills = [], {}
    for f in folders:
        o = {}
        for row in table:
            path = os.path.join(f, row.name)
            info = io.tiff_info(path)
            gt, epsg = io.geo_from_tags(info)
            if gt is None or epsg is None:
                raise ValueError(f"{path}: the file carries no georeferencing (geotransform and CRS tags)")
            if "geotransform" in o and (tuple(gt) != tuple(o["geotransform"]) or epsg != o["crs"]):
                raise ValueError(f"{path}: another grid than the other rasters of {f}")
            a = io.read_tiff(path, info=info)
            a = a[0] if a.ndim == 3 else a
            want = np.uint8 if row.uint8 else np.float32
            if a.dtype != want:
                raise ValueError(f"{path}: expected {np.dtype(want)}, got {a.dtype}")
            if row.nodata and row.key not in fills:
                nod = _nodata(info)
                fills[row.key] = float(mag1c.NODATA) if nod is None else nod
            o[row.key] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            o.update(geotransform=gt, crs=epsg)
        outs.append(o)
    out = products.mosaic(outs, crs, resolution, rule, "prediction", "nearest", fills, keys=[row.key for row in table])
    gt, epsg = out["geotransform"], out["crs"]
    area = abs(gt[1] * gt[5]) if warp.crs_kind(epsg)[0] == 2 else None
    if clean is not None:
        products.clean(out, **clean)
    products.annotate(out, out["pred_binary"], out.get("mf"), out["prediction"], gt, area, plumes, plume_outlines, label_polygons,
                      match_tolerance_px, plume_background, plume_quantify)
    geo = warp.geo_tags(gt, epsg)
    out_folder = str(out_folder)
    files = []
    for row in table:                             # every float raster under its own no-data value
        files += products.write_rasters(out, (row,), out_folder, overwrite, geo, fills.get(row.key), {}, cog)
    src = out["source_index"]
    out["source"] = torch.where(src < 0, products.SOURCE_NONE, src).to(torch.uint8)
    path = os.path.join(out_folder, products.SOURCE.name)
    if overwrite or not os.path.exists(path):
        os.makedirs(out_folder, exist_ok=True)
        names = {f"source_{i}": os.path.basename(f) for i, f in enumerate(folders)}
        tags = {**geo, 42113: (2, (nodata_text(products.SOURCE_NONE),)), **io.gdal_metadata_tag(names, list(products.SOURCE.bands))}
        products.write_raster(path, out["source"], tags, cog, products.SOURCE_NONE)
        files.append(path)
    out["files"] = files + products.write_annotations(out, out_folder, overwrite, geo, cog)
    return out


BANDS_S2 = ["B1", "B2", "B3", "B4", "B5", "B6", "B7", "B8", "B8A", "B9", "B10", "B11", "B12"]
BANDS_WV3 = ["SWIR1", "SWIR2", "SWIR3", "SWIR4", "SWIR5", "SWIR6", "SWIR7", "SWIR8"]
BANDS_SENSOR = {"S2A": BANDS_S2, "S2B": BANDS_S2, "WV3": BANDS_WV3}

_NANOMETERS = ("nanometers", "nanometer", "nm")


@torch.no_grad()
def aviris_as_sensor(aviris_img_folder_or_path, folder_dest, sensors=list(BANDS_SENSOR), bands=BANDS_SENSOR, columns_read=50,
                     path_tiffs_temp=".", disable_pbar=True, device="cuda", lines_per_chunk=None, resolution_dst=None, mode="constant"):
    """``aviris_as_sensor`` of the reference (starcop/process_aviris.py:26-90) on the MI355X: writes
    ``{folder_dest}/{sensor}_{band}.tif`` for every band of ``bands[sensor]`` (WV3 SWIR1..8, S2A / S2B B1..B12) simulated from the
    ENVI radiance ``<name>_img`` of an AVIRIS-NG flight-line folder, skipping files that already exist.  The SRF tables come from the
    module caches of :mod:`starcop_amd.aviris` (``load_srf_wv3`` / ``load_srf_s2`` with ``path_override``).

    The cube is streamed in chunks of ``lines_per_chunk`` lines (default: about 256 MB) memmap -> pinned staging -> device with two
    buffers, so the upload of one chunk overlaps the kernel on the previous one; one ``sc_srf_bands`` call per chunk computes every
    missing band of every sensor.  Band centres come from the header (nanometers), the fill value from its ``data ignore value``
    (none: nothing is masked and no nodata tag is written).  Outputs: float32 (lines, samples), tiled 128 x 128, the radiance file's
    georeferencing, GDAL_NODATA = the fill value, the band name as description.  ``columns_read``, ``path_tiffs_temp`` and
    ``disable_pbar`` are accepted for the reference's signature and ignored.  Returns the list of files written.

    ``resolution_dst=None`` (the reference's own call) writes every band on the AVIRIS grid.  A number resamples every band to pixels
    of that size, ``"native"`` every Sentinel-2 band to its own 10 / 20 / 60 m (a WV3 sensor then raises ValueError): the whole
    (bands, lines, samples) device buffer is resampled before the read-back, one ``sc_resize_aa`` call per resolution, as
    ``aviris.transform_to_sentinel_2`` / ``transform_to_worldview_3`` resample (Sentinel-2 bands blurred with the sigma of their own
    ground sampling distance, WV3 bands with the default of the scale; border ``mode``, ``cval`` = the fill value or 0), and only
    the small planes cross to the host.  The source pixel size is the header's ``map info`` x / y size (ValueError without one); the
    files carry the source's georeferencing with the pixel scaled by the true ratios lines / output lines and samples / output
    samples (``io_formats.scaled_geo_tags``), so the upper-left corner and the full extent stay exact."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    from . import aviris, io_formats as io, resample
    for sensor in sensors:
        if sensor != "WV3" and not str(sensor).startswith("S2"):
            raise NotImplementedError(f"Sensor {sensor} not known. Expected sensors [WV3, S2A, S2B]")
    native = isinstance(resolution_dst, str)
    if native and resolution_dst != "native":
        raise ValueError(f"resolution_dst '{resolution_dst}': expected None, a pixel size or 'native'")
    if native and "WV3" in sensors:
        raise ValueError("resolution_dst='native' is defined for the Sentinel-2 sensors only (WV3 bands have no table of native pixel sizes)")
    if resolution_dst is not None and mode not in resample.MODES:
        raise ValueError(f"border mode '{mode}': expected one of {resample.MODES}")
    src = str(aviris_img_folder_or_path)
    if src.endswith(".tif"):
        raise NotImplementedError(f"{src}: only ENVI flight-line folders are supported, not GeoTIFF radiance")
    if str(folder_dest).startswith("gs://"):
        raise NotImplementedError(f"{folder_dest}: writing to Google Cloud Storage is not supported")
    folder = src.rstrip("/")
    name = os.path.basename(folder)
    envi_path = os.path.join(folder, f"{name}_img")
    if not os.path.exists(envi_path):
        raise NotImplementedError(f"{folder}: no ENVI radiance {name}_img; the one-file-per-band layout is not supported")
    todo = [(sensor, band, os.path.join(folder_dest, f"{sensor}_{band}.tif")) for sensor in sensors for band in bands[sensor]]
    todo = [t for t in todo if not os.path.exists(t[2])]
    if not todo:
        return []
    os.makedirs(folder_dest, exist_ok=True)

    cube, meta = io.open_envi(envi_path)
    header = meta["header"]
    units = str(header.get("wavelength units", "nanometers")).strip().lower()
    if units not in _NANOMETERS:
        raise ValueError(f"{envi_path}: wavelength units '{units}', expected nanometers")
    if meta["wavelengths"] is None:
        raise ValueError(f"{envi_path}: the header has no wavelength list")
    if cube.dtype.kind not in "fiu" or (cube.dtype.kind == "f" and cube.dtype.itemsize != 4) or \
            (cube.dtype.kind in "iu" and cube.dtype.itemsize > 2):
        raise NotImplementedError(f"{envi_path}: radiance of type {cube.dtype} (float32 or 8/16-bit integers expected)")
    fill = header.get("data ignore value")
    fill = float(fill) if fill is not None else None

    L, S, B = cube.shape
    # resampling: the planes of one target pixel size are made neighbours in the device buffer (a stable sort of `todo`), so that each
    # group is one slice of it; everything that can be refused is refused here, before the cube is streamed
    groups = []                                              # (first plane, last plane + 1, (oh, ow) or None, sigmas (n, 2))
    if resolution_dst is not None:
        mi = header.get("map info")
        try:
            res_src = (abs(float(mi[6])), abs(float(mi[5])))              # (y, x) pixel size
        except (TypeError, IndexError, ValueError):
            raise ValueError(f"{envi_path}: no map info with a pixel size in the header; resolution_dst needs the source's") from None
        res_band = [float(aviris.BANDS_S2_RESOLUTION[b]) if native else float(resolution_dst) for _, b, _ in todo]
        todo = [todo[j] for j in sorted(range(len(todo)), key=lambda j: res_band[j])]
        res_band = sorted(res_band)
        for k0 in range(len(todo)):
            if k0 and res_band[k0] == res_band[k0 - 1]:
                continue
            k1 = k0 + res_band[k0:].count(res_band[k0])
            shape = resample.output_shape_for((L, S), res_src, res_band[k0])
            if shape[0] > L or shape[1] > S:
                raise ValueError(f"{envi_path}: pixels of {res_src} m cannot be resampled to the finer {res_band[k0]} m; only "
                                 "downscaling is supported")
            sig = np.array([(aviris.sentinel_2_sigmas([b], res_src)[0],) * 2 if s != "WV3" else
                            (resample.default_sigma(L, shape[0]), resample.default_sigma(S, shape[1])) for s, b, _ in todo[k0:k1]])
            groups.append((k0, k1, None if shape == (L, S) else shape, sig))

    rows = [None] * len(todo)                                # the CSR row of every output plane, in the order of `todo`
    for sensor in dict.fromkeys(s for s, _, _ in todo):
        js = [j for j, t in enumerate(todo) if t[0] == sensor]
        srf = aviris.load_srf_wv3() if sensor == "WV3" else aviris.sentinel_2_srf(sensor)
        p, b, w = aviris.srf_weights([todo[j][1] for j in js], srf, meta["wavelengths"])
        for i, j in enumerate(js):
            rows[j] = (b[p[i]:p[i + 1]], w[p[i]:p[i + 1]])
    ptrs = np.concatenate([[0], np.cumsum([len(b) for b, _ in rows])]).astype(np.int32)
    plan = aviris.SrfPlan(ptrs, np.concatenate([b for b, _ in rows]), np.concatenate([w for _, w in rows]), device)

    perm = tuple(int(v) for v in np.argsort([-s for s in cube.strides], kind="stable"))    # memory order of (line, sample, band)
    inv = tuple(int(v) for v in np.argsort(perm))
    if lines_per_chunk is None:
        lines_per_chunk = max(1, (256 << 20) // (S * B * 4))
    lpc = max(1, min(int(lines_per_chunk), L))
    nmax = lpc * S * B
    out = torch.empty((plan.n_out, L, S), dtype=torch.float32, device=device)
    pinned = [torch.empty(nmax, dtype=torch.float32).pin_memory() for _ in range(2)]
    staged = [torch.empty(nmax, dtype=torch.float32, device=device) for _ in range(2)]
    uploaded = [torch.cuda.Event() for _ in range(2)]
    consumed = [torch.cuda.Event() for _ in range(2)]
    used = [False, False]
    compute = torch.cuda.current_stream(device)
    upload = torch.cuda.Stream(device)
    for c, l0 in enumerate(range(0, L, lpc)):
        i = c % 2
        n = min(lpc, L - l0)
        raw = cube[l0:l0 + n].transpose(perm)
        if used[i]:
            uploaded[i].synchronize()                         # the previous upload from this pinned buffer has finished
        host = pinned[i][:raw.size].view(raw.shape)
        np.copyto(host.numpy(), raw, casting="unsafe")
        dev = staged[i][:raw.size].view(raw.shape)
        with torch.cuda.stream(upload):
            if used[i]:
                upload.wait_event(consumed[i])                # the kernel that read this device buffer has finished
            dev.copy_(host, non_blocking=True)
            uploaded[i].record(upload)
        compute.wait_event(uploaded[i])
        plan.run(dev.permute(inv), out[:, l0:l0 + n], fill)
        consumed[i].record(compute)
        used[i] = True
    geo = io.envi_geo_tags(header)
    if fill is not None:
        geo[42113] = (2, (nodata_text(fill),))
    if resolution_dst is None:
        result = out.cpu().numpy()
        tags = [geo] * len(todo)
    else:
        result, tags = [], []
        for k0, k1, shape, sig in groups:
            if shape is None:                                # already at this pixel size: the spectral result, as transform_to_srf
                small, g = out[k0:k1], geo
            else:
                small = resample.resize_antialiased(out[k0:k1], shape, sigma=sig, mode=mode, cval=0.0 if fill is None else fill)
                g = io.scaled_geo_tags(geo, L / shape[0], S / shape[1])
            result.extend(small.cpu().numpy())
            tags.extend([g] * (k1 - k0))

    def write(j):
        _, band, path = todo[j]
        io.write_tiff(path, result[j], blocksize=128, extra_tags={**tags[j], **io.gdal_metadata_tag({}, [band])})
        return path
    with ThreadPoolExecutor(max_workers=min(8, len(todo))) as pool:
        return list(pool.map(write, range(len(todo))))
