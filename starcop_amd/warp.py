"""Reprojection of rasters between grids on the MI355X (``sc_warp``, include/starcop_hip.h) and the host side that goes with it.

A grid is a shape, a 6-term GDAL geotransform (rotation allowed) and a CRS code: 4326 (WGS-84 longitude / latitude in degrees) or
326zz / 327zz (WGS-84 UTM north / south); ``None`` or any equal pair of integers means "the same CRS, whatever it is" and takes the
affine-only path.  For every destination pixel the kernel computes the source pixel coordinates in fp64 -- affine, Transverse
Mercator by the Krueger series to order n^6 (Karney 2011) where the CRS differ, inverse affine of the source -- and samples all
planes of a call there, ``nearest`` (a word copy: bit-equal to a numpy gather for every dtype) or ``bilinear`` (float32; fp64
weights renormalised over the samples that are inside, not NaN and not no-data; one rounding).  Both modes give a pixel the plane's
no-data when it lies outside the source; ``bilinear`` also when its nearest source pixel does not count, so the two have the same
valid pixels.  ``average``, ``max``, ``min`` and ``mode`` (``sc_warp_area``) reduce the source pixels under the destination pixel's
footprint instead -- what a coarser destination needs; :func:`reproject` states the rule.  There is no CPU fallback for the rasters.

:func:`transform_points` is the host restatement of the projection step, the same series in numpy; bounds (:func:`suggest_grid`),
polygons (:func:`transform_polygons`) and the tests use it.  Datums other than WGS-84, polar stereographic and the Norway / Svalbard
exceptions of the UTM grid are not handled."""
import math
import os
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check as _check, sc_warp_area_args, sc_warp_args, stream
from .planes import as_planes, chunks, fill_bits, numpy_dtype, per_plane, set_planes

MAX_PLANES = _lib.WARP_MAX_PLANES
RESAMPLING = {"nearest": _lib.WARP_NEAREST, "bilinear": _lib.WARP_BILINEAR, "average": _lib.WARP_AREA_AVERAGE,
              "max": _lib.WARP_AREA_MAX, "min": _lib.WARP_AREA_MIN, "mode": _lib.WARP_AREA_MODE}
POINT_RESAMPLING = ("nearest", "bilinear")        # look at the destination pixel's centre (sc_warp)
AREA_RESAMPLING = ("average", "max", "min", "mode")      # reduce the source pixels under its footprint (sc_warp_area)
AREA_VARIANTS = {None: 0, "thread": _lib.WARP_AREA_THREAD, "lanes": _lib.WARP_AREA_LANES}
MAX_DLON = 30.0            # degrees from a zone's central meridian beyond which a point is outside (NaN)
NEWTON_STEPS = 3            # of the conformal-latitude inversion, as in the kernel: 2 reach the last place for |lat| < 89.999, one spare

# ---------------------------------------------------------------------------------------------- WGS-84 Transverse Mercator
_A, _F, _K0 = 6378137.0, 1.0 / 298.257223563, 0.9996
_N = _F / (2.0 - _F)
E1 = math.sqrt(_F * (2.0 - _F))                 # first eccentricity
E2M = (1.0 - _F) ** 2                           # 1 - e^2
KA = _K0 * _A / (1.0 + _N) * (1.0 + _N ** 2 / 4.0 + _N ** 4 / 64.0 + _N ** 6 / 256.0)      # k0 x rectifying radius


def _poly(*c):
    """c[0] n^k + c[1] n^(k+1) + ... with k = 7 - len(c): the tail of a series that ends at n^6"""
    k = 7 - len(c)
    return sum(v * _N ** (k + i) for i, v in enumerate(c))


# Karney 2011 eq. 35 (alpha: conformal sphere -> rectifying) and eq. 36 (beta: back), to order n^6
ALPHA = (_poly(1 / 2, -2 / 3, 5 / 16, 41 / 180, -127 / 288, 7891 / 37800),
         _poly(13 / 48, -3 / 5, 557 / 1440, 281 / 630, -1983433 / 1935360),
         _poly(61 / 240, -103 / 140, 15061 / 26880, 167603 / 181440),
         _poly(49561 / 161280, -179 / 168, 6601661 / 7257600),
         _poly(34729 / 80640, -3418889 / 1995840),
         _poly(212378941 / 319334400))
BETA = (_poly(1 / 2, -2 / 3, 37 / 96, -1 / 360, -81 / 512, 96199 / 604800),
        _poly(1 / 48, 1 / 15, -437 / 1440, 46 / 105, -1118711 / 3870720),
        _poly(17 / 480, -37 / 840, -209 / 4480, 5569 / 90720),
        _poly(4397 / 161280, -11 / 504, -830251 / 7257600),
        _poly(4583 / 161280, -108847 / 3991680),
        _poly(20648693 / 638668800))


def crs_kind(code) -> Tuple[int, float, float]:
    """(kind, central meridian in degrees, false northing): kind 1 = 4326, 2 = WGS-84 UTM, -1 = a code the projection does not know"""
    code = int(code)
    if code == 4326:
        return 1, 0.0, 0.0
    if 32601 <= code <= 32660 or 32701 <= code <= 32760:
        return 2, 6.0 * (code % 100) - 183.0, 10_000_000.0 if code >= 32701 else 0.0
    return -1, 0.0, 0.0


def crs_pair(src_crs, dst_crs, who):
    """-> (src code, dst code) for the kernel: (0, 0) when both are None or equal; NotImplementedError for a pair that needs a
    projection other than 4326 <-> UTM"""
    if src_crs is None and dst_crs is None:
        return 0, 0
    if src_crs is None or dst_crs is None:
        raise ValueError(f"{who}: one CRS is None and the other {src_crs if dst_crs is None else dst_crs}; give both or neither")
    s, d = int(src_crs), int(dst_crs)
    if s == d:
        return 0, 0
    if crs_kind(s)[0] < 0 or crs_kind(d)[0] < 0:
        raise NotImplementedError(f"{who}: EPSG:{s} -> EPSG:{d} is not supported (WGS-84 only: 4326 and UTM 32601..32660 / 32701..32760)")
    return s, d


def _clenshaw_sin(c, xi, eta):
    """sum_j c[j-1] sin(2 j (xi + i eta)) -> (real, imaginary) part, as the kernel sums it"""
    s0, c0, sh0, ch0 = np.sin(2.0 * xi), np.cos(2.0 * xi), np.sinh(2.0 * eta), np.cosh(2.0 * eta)
    ar, ai = 2.0 * c0 * ch0, -2.0 * s0 * sh0
    y1r = y1i = y2r = y2i = np.zeros_like(xi)
    for j in range(5, -1, -1):
        yr = c[j] + ar * y1r - ai * y1i - y2r
        yi = ar * y1i + ai * y1r - y2i
        y2r, y2i, y1r, y1i = y1r, y1i, yr, yi
    zr, zi = s0 * ch0, c0 * sh0
    return zr * y1r - zi * y1i, zr * y1i + zi * y1r


def _taup(tau):
    t1 = np.sqrt(1.0 + tau * tau)
    sig = np.sinh(E1 * np.arctanh(E1 * tau / t1))
    return tau * np.sqrt(1.0 + sig * sig) - sig * t1


def _tm_forward(lon, lat, lon0, fn):
    """degrees -> (easting, northing); NaN beyond MAX_DLON of the central meridian or |lat| > 90"""
    with np.errstate(all="ignore"):
        dl = lon - lon0
        dl = dl - 360.0 * np.round(dl / 360.0)
        ok = (np.abs(dl) <= MAX_DLON) & (np.abs(lat) <= 90.0)
        taup = _taup(np.tan(np.radians(lat)))
        sl, cl = np.sin(np.radians(dl)), np.cos(np.radians(dl))
        xip, etap = np.arctan2(taup, cl), np.arcsinh(sl / np.sqrt(taup * taup + cl * cl))
        dx, de = _clenshaw_sin(ALPHA, xip, etap)
        e, n = 500000.0 + KA * (etap + de), fn + KA * (xip + dx)
    return np.where(ok, e, np.nan), np.where(ok, n, np.nan)


def _tm_inverse(e, n, lon0, fn):
    """(easting, northing) -> degrees; NaN beyond MAX_DLON of the central meridian"""
    with np.errstate(all="ignore"):
        xi, eta = (n - fn) / KA, (e - 500000.0) / KA
        dx, de = _clenshaw_sin(BETA, xi, eta)
        xip, etap = xi - dx, eta - de
        sx, cx, shp = np.sin(xip), np.cos(xip), np.sinh(etap)
        taup = sx / np.sqrt(shp * shp + cx * cx)
        lam = np.arctan2(shp, cx)
        tau = taup / E2M
        for _ in range(NEWTON_STEPS):
            ta = _taup(tau)
            tau = tau + (taup - ta) * (1.0 + E2M * tau * tau) / (E2M * np.sqrt(1.0 + ta * ta) * np.sqrt(1.0 + tau * tau))
        ok = np.abs(lam) <= math.radians(MAX_DLON)
        lon, lat = lon0 + np.degrees(lam), np.degrees(np.arctan(tau))
    return np.where(ok, lon, np.nan), np.where(ok, lat, np.nan)


def transform_points(x, y, src_crs, dst_crs):
    """Coordinates ``(x, y)`` in ``src_crs`` -> float64 numpy arrays in ``dst_crs`` (host; no device needed): longitude /
    latitude in degrees for 4326, easting / northing in metres for WGS-84 UTM.  The Krueger series of the kernel, term for term:
    4326 -> UTM forward, UTM -> 4326 inverse, zone A -> zone B through longitude / latitude.  Points further than 30 degrees of
    longitude from a zone's central meridian, latitudes beyond +-90 and non-finite results come back as NaN.  Equal codes (or None
    on both sides) return the input as float64."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    s, d = crs_pair(src_crs, dst_crs, "transform_points")
    if s == d:
        return x.copy(), y.copy()
    (ks, slon0, sfn), (kd, dlon0, dfn) = crs_kind(s), crs_kind(d)
    if ks == 2:
        x, y = _tm_inverse(x, y, slon0, sfn)
    if kd == 2:
        x, y = _tm_forward(x, y, dlon0, dfn)
    bad = ~(np.isfinite(x) & np.isfinite(y))
    return np.where(bad, np.nan, x), np.where(bad, np.nan, y)


def utm_crs_for(lon, lat) -> int:
    """EPSG code of the WGS-84 UTM zone of a point: 326zz north of the equator (and on it), 327zz south.  The plain 6-degree grid:
    the exceptions around Norway (32V) and Svalbard (31X-37X) are NOT handled."""
    lon, lat = float(lon), float(lat)
    if not (math.isfinite(lon) and -90.0 <= lat <= 90.0):
        raise ValueError(f"utm_crs_for: ({lon}, {lat}) is not a longitude / latitude")
    zone = int(math.floor(((lon + 180.0) % 360.0) / 6.0)) % 60 + 1
    return (32600 if lat >= 0.0 else 32700) + zone


# ---------------------------------------------------------------------------------------------- grids
def gt6(gt, who):
    g = [float(v) for v in np.asarray(gt, dtype=np.float64).ravel()]
    if len(g) != 6 or not all(math.isfinite(v) for v in g):
        raise ValueError(f"{who}: a geotransform is 6 finite numbers in GDAL order, got {gt!r}")
    if g[1] * g[5] - g[2] * g[4] == 0.0:
        raise ValueError(f"{who}: singular geotransform {tuple(g)}")
    return g


def invert_geotransform(gt):
    """the affine world -> pixel of a GDAL geotransform, in the same 6-term order: u = inv[0] + x inv[1] + y inv[2],
    v = inv[3] + x inv[4] + y inv[5] (float64)"""
    x0, a, b, y0, c, d = gt6(gt, "invert_geotransform")
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return (-(ia * x0 + ib * y0), ia, ib, -(ic * x0 + id_ * y0), ic, id_)


def apply_geotransform(gt, col, row):
    """pixel coordinates (fractional, corner-based) -> world"""
    col, row = np.asarray(col, dtype=np.float64), np.asarray(row, dtype=np.float64)
    return gt[0] + col * gt[1] + row * gt[2], gt[3] + col * gt[4] + row * gt[5]


def suggest_grid(src_shape, src_gt, src_crs, dst_crs, resolution=None):
    """A north-up grid in ``dst_crs`` that covers a source raster -> ``(dst_shape, dst_gt)``.

    The source outline -- every pixel corner along its four edges -- is transformed and its bounding box taken.  The default
    ``resolution`` keeps the number of pixels along the source's diagonal: the diagonal of that box divided by
    sqrt(rows^2 + cols^2), which is the rule GDAL's suggested warp output uses (nothing more is claimed: GDAL's handling of
    outlines that fail to transform is not restated).  The origin is snapped OUTWARD to multiples of ``resolution``, so two
    scenes warped to one CRS and resolution share a lattice.  A grid of 2^31 pixels or more is refused."""
    H, W = (int(v) for v in src_shape)
    if H < 1 or W < 1:
        raise ValueError(f"suggest_grid: empty source {src_shape}")
    gt = gt6(src_gt, "suggest_grid")
    cols = np.concatenate([np.arange(W + 1.0), np.full(H + 1, float(W)), np.arange(W + 1.0), np.zeros(H + 1)])
    rows = np.concatenate([np.zeros(W + 1), np.arange(H + 1.0), np.full(W + 1, float(H)), np.arange(H + 1.0)])
    x, y = transform_points(*apply_geotransform(gt, cols, rows), src_crs, dst_crs)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError(f"suggest_grid: part of the source outline has no coordinates in EPSG:{dst_crs}")
    xmin, xmax, ymin, ymax = float(x.min()), float(x.max()), float(y.min()), float(y.max())
    if resolution is None:
        resolution = math.hypot(xmax - xmin, ymax - ymin) / math.hypot(W, H)
    res = float(resolution)
    if not (math.isfinite(res) and res > 0.0):
        raise ValueError(f"suggest_grid: resolution {resolution!r}")
    i0, j0 = math.floor(xmin / res), math.ceil(ymax / res)
    Wd, Hd = max(1, math.ceil(xmax / res) - i0), max(1, j0 - math.floor(ymin / res))
    if Hd * Wd >= 2 ** 31:
        raise ValueError(f"suggest_grid: {Hd} x {Wd} pixels at resolution {res}: 2^31 pixels or more")
    return (Hd, Wd), (i0 * res, res, 0.0, j0 * res, 0.0, -res)


def geo_tags(gt, crs) -> Dict[int, tuple]:
    """GeoTIFF tags of a grid: ModelPixelScale (33550) + ModelTiepoint (33922) for a north-up geotransform, else the
    ModelTransformation (34264), and the GeoKeyDirectory (34735) in the layouts ``io_formats.envi_geo_tags`` and
    ``ortho.emit_geo_tags`` write: geographic for 4326, projected with ProjectedCSType = the EPSG code for WGS-84 UTM.  Any other
    ``crs`` (None included) gives no key directory."""
    x0, a, b, y0, c, d = gt6(gt, "geo_tags")
    tags: Dict[int, tuple] = {}
    if b == 0.0 and c == 0.0 and a > 0.0 and d < 0.0:
        tags[33550] = (12, (a, -d, 0.0))
        tags[33922] = (12, (0.0, 0.0, 0.0, x0, y0, 0.0))
    else:
        tags[34264] = (12, (a, b, 0.0, x0, c, d, 0.0, y0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0))
    kind = crs_kind(crs)[0] if crs is not None else -1
    if kind == 1:
        tags[34735] = (3, (1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326))
    elif kind == 2:
        tags[34735] = (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, int(crs)))
    return tags


def _ring_map(ring, src_crs, dst_crs):
    a = np.asarray(ring, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError(f"transform_polygons: a ring is an (n, 2) array of x, y; got shape {a.shape}")
    x, y = transform_points(a[:, 0], a[:, 1], src_crs, dst_crs)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError(f"transform_polygons: a vertex has no coordinates in EPSG:{dst_crs}")
    return np.stack([x, y], axis=1)


def transform_polygons(polygons, src_crs, dst_crs):
    """Polygons as ``plumes.plume_outlines`` returns and ``plumes.rasterize_polygons`` takes them -- a list of polygons, each a list
    of (n, 2) rings, or a dict {id: such a list} -- with every vertex moved from ``src_crs`` to ``dst_crs`` (host).  Ring count,
    vertex count and closure are kept: equal vertices map to equal vertices.  A vertex outside the target's domain: ValueError."""
    if isinstance(polygons, dict):
        return {k: [_ring_map(r, src_crs, dst_crs) for r in rings] for k, rings in polygons.items()}
    return [[_ring_map(r, src_crs, dst_crs) for r in rings] for rings in polygons]


# ---------------------------------------------------------------------------------------------- the device side
def _grid_pair(who, src_gt, src_crs, dst_gt, dst_crs, dst_shape):
    """the checked grid pair of a call -> (inverse source affine, source code, destination code, destination affine, (H_d, W_d))"""
    s_code, d_code = crs_pair(src_crs, dst_crs, who)
    return invert_geotransform(src_gt), s_code, d_code, gt6(dst_gt, who), dst_grid_shape(dst_shape, who)


def _grid_args(cls, grid, src_shape):
    """a ``cls`` (sc_warp_args or sc_warp_area_args: the fields of the grid pair have one name in both) for a :func:`_grid_pair`"""
    a = cls()
    a.src_inv[:], a.src_crs, a.dst_crs, a.dst_gt[:], (a.out_h, a.out_w) = grid
    a.src_h, a.src_w = src_shape
    return a


def _chunk_args(cls, grid, src_shape, planes, nd, bits, out, p0, n):
    """... and the planes [p0, p0 + n) of a call with their no-data patterns and their part of ``out``"""
    a = _grid_args(cls, grid, src_shape)
    a.P, a.elem_bytes = n, nd.itemsize if n else 0
    set_planes(a, planes, p0)
    a.nodata_bits[:n] = bits[p0:p0 + n]
    a.out = out[p0].data_ptr() if n else None
    return a


def _launch(grid, src_shape, planes, nd, bits, mode, out, coords, flags=0):
    lib = _lib.load()
    for p0, n in chunks(len(planes), MAX_PLANES):
        a = _chunk_args(sc_warp_args, grid, src_shape, planes, nd, bits, out, p0, n)
        a.resampling, a.flags = mode, flags
        a.coords = coords.data_ptr() if coords is not None and p0 == 0 else None      # the coordinates are the same for every chunk
        _check(lib.sc_warp(a, stream()))


def _variant_code(variant):
    if variant not in AREA_VARIANTS:
        raise ValueError(f"variant {variant!r}; expected None (chosen by the library), 'thread' or 'lanes'")
    return AREA_VARIANTS[variant]


def _launch_area(grid, src_shape, planes, nd, bits, mode, min_coverage, out, cov, boxes, variant):
    lib = _lib.load()
    for p0, n in chunks(len(planes), MAX_PLANES):
        a = _chunk_args(sc_warp_area_args, grid, src_shape, planes, nd, bits, out, p0, n)
        a.mode, a.min_coverage, a.variant = mode, min_coverage, _variant_code(variant)
        a.coverage = cov[p0].data_ptr() if cov is not None and n else None
        a.boxes = boxes.data_ptr() if boxes is not None and p0 == 0 else None        # the boxes are the same for every chunk
        _check(lib.sc_warp_area(a, stream()))


def _area_dtype_check(resampling, dt):
    """the dtype refusals of the footprint modes (``dt``: a numpy or torch dtype); before any device use"""
    name = str(dt).replace("torch.", "")
    ok = {"average": ("float32",), "mode": ("uint8",), "max": ("float32", "uint8"), "min": ("float32", "uint8")}[resampling]
    if name not in ok:
        raise ValueError(f"reproject: {resampling} resampling is defined for {' and '.join(ok)}, not {name}")


def dst_grid_shape(shape, who):
    H, W = (int(v) for v in shape)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{who}: destination shape {tuple(shape)} (at least 1 x 1, fewer than 2^31 pixels)")
    return H, W


def reproject(data, src_gt, src_crs, dst_gt, dst_crs, dst_shape, resampling="nearest", nodata=None, min_coverage=0.5,
              return_coverage=False, variant=None):
    """``data`` on the grid ``(src_gt, src_crs)`` resampled onto ``(dst_shape, dst_gt, dst_crs)`` on the GPU.

    ``data``: a device tensor (H, W) or (P, H, W) with any non-negative strides (a permuted pixel-interleaved cube is read in
    place), a list of 2-D tensors of one dtype and shape, or a numpy array (numpy in, numpy out).  ``nodata``: a scalar or one
    value per plane (default 0): what pixels outside the source get, and -- for ``bilinear`` -- the value that is left out of the
    interpolation.  ``resampling``: ``"nearest"`` for any 1-, 2-, 4- or 8-byte dtype, ``"bilinear"`` for float32 (an integer dtype
    raises ValueError).  Geotransforms are 6 numbers in GDAL order and may be rotated.  Equal CRS codes, or None on both sides,
    take the affine-only path (any integer is allowed there); otherwise both must be 4326 or WGS-84 UTM (NotImplementedError names
    the pair).  Returns (H_d, W_d) for 2-D input, else (P, H_d, W_d): contiguous, in the dtype of the input.  No CPU fallback.

    The footprint modes, for a destination coarser than the source: ``"average"`` (float32), ``"max"`` / ``"min"`` (float32 and
    uint8) and ``"mode"`` (uint8; ties to the smallest value).  The four corners of the destination pixel are projected like its
    centre; their axis-aligned BOUNDING BOX in source pixel coordinates is the footprint (for a rotated pair it is larger than the
    true quadrilateral, as in GDAL).  A source pixel takes part when it overlaps the box by more than 2^-20 px along both axes
    (the sliver rule: on a shared lattice the corners land on integers +- 1e-11, and the result must not depend on that noise)
    and counts when it is not ``nodata`` and not NaN.  ``average`` weighs by overlap area; ``coverage`` is the overlap area of
    the counting samples over the area of the whole box, the part outside the raster included.  The pixel is data when a sample
    counts and ``coverage >= min_coverage`` (in [0, 1]; 0: any counting sample suffices), else ``nodata``.
    ``return_coverage=True`` returns ``(out, coverage)``, coverage float32 in the shape of ``out`` and 0 where the pixel is
    no-data: ``sum(average * coverage) * pixel area`` conserves an integral.  ``variant`` forces one of the kernel's two mappings
    (``"thread"`` / ``"lanes"``; tests and measurements)."""
    if resampling not in RESAMPLING:
        raise ValueError(f"reproject: resampling {resampling!r}; expected one of {sorted(RESAMPLING)}")
    area = resampling in AREA_RESAMPLING
    if return_coverage and not area:
        raise ValueError(f"reproject: return_coverage goes with the footprint resampling modes {AREA_RESAMPLING}, not {resampling!r}")
    if variant is not None and not area:
        raise ValueError(f"reproject: variant goes with the footprint resampling modes {AREA_RESAMPLING}, not {resampling!r}")
    min_coverage = float(min_coverage)
    if not 0.0 <= min_coverage <= 1.0:
        raise ValueError(f"reproject: min_coverage {min_coverage!r} outside [0, 1]")
    grid = _grid_pair("reproject", src_gt, src_crs, dst_gt, dst_crs, dst_shape)
    planes, single, host = as_planes(data, "reproject")
    dt, shape = planes[0].dtype, tuple(planes[0].shape)
    if resampling == "bilinear" and dt != torch.float32:       # a numpy input is named as numpy names it
        raise ValueError(f"reproject: bilinear resampling is defined for float32, not {str(dt).replace('torch.', '') if host else dt}")
    if area:
        _area_dtype_check(resampling, dt)
    nd = numpy_dtype(dt, "reproject")
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"reproject: empty source {shape}")
    P = len(planes)
    bits = [fill_bits(v, nd, "reproject") for v in per_plane(nodata, P, "reproject", "nodata values", default=0)]
    _lib.require_device(None if host else planes[0])
    if host:
        planes = [p.cuda() for p in planes]
    dev = planes[0].device
    out = torch.empty((P, *grid[4]), dtype=dt, device=dev)
    cov = torch.empty_like(out, dtype=torch.float32) if return_coverage else None
    if area:
        _launch_area(grid, shape, planes, nd, bits, RESAMPLING[resampling], min_coverage, out, cov, None, variant)
    else:
        _launch(grid, shape, planes, nd, bits, RESAMPLING[resampling], out, None)
    res = [t[0] if single else t for t in ((out, cov) if return_coverage else (out,))]
    res = [t.cpu().numpy() if host else t for t in res]
    return tuple(res) if return_coverage else res[0]


def source_coords(dst_shape, dst_gt, dst_crs, src_gt, src_crs, src_shape=None, device="cuda"):
    """The source pixel coordinates ``(u, v)`` of every destination pixel centre, as the kernel computes them: device float64
    (2, H, W), u along columns and v along rows of the source (pixel (row, col) covers [col, col + 1) x [row, row + 1)).  With
    ``src_shape=(H_s, W_s)`` pixels outside the source are NaN, as they are no-data in :func:`reproject`; without it only points
    the projection cannot place are."""
    grid = _grid_pair("source_coords", src_gt, src_crs, dst_gt, dst_crs, dst_shape)
    _lib.require_device()
    coords = torch.empty((2, *grid[4]), dtype=torch.float64, device=device)
    shape = (1, 1) if src_shape is None else tuple(int(v) for v in src_shape)
    _launch(grid, shape, [], None, [], 0, None, coords, flags=_lib.WARP_UNBOUNDED if src_shape is None else 0)
    return coords


def source_boxes(dst_shape, dst_gt, dst_crs, src_gt, src_crs, device="cuda", variant=None):
    """The footprint of every destination pixel in source pixel coordinates, as the kernel of the footprint modes computes it: device
    float64 (4, H, W) = u0, u1, v0, v1, the axis-aligned bounding box of the pixel's four projected corners, NOT clipped to the
    source; NaN where a corner has no coordinates.  The counterpart of :func:`source_coords`."""
    grid = _grid_pair("source_boxes", src_gt, src_crs, dst_gt, dst_crs, dst_shape)
    _lib.require_device()
    boxes = torch.empty((4, *grid[4]), dtype=torch.float64, device=device)
    _launch_area(grid, (1, 1), [], None, [], 0, 0.0, None, None, boxes, variant)
    return boxes


def area_variant(dst_shape, dst_gt, dst_crs, src_gt, src_crs) -> str:
    """the mapping the library chooses for the footprint modes on a grid pair: ``"thread"`` (one thread per destination pixel; boxes of
    a few source pixels) or ``"lanes"`` (16 lanes along the source columns of one pixel's box).  Host only."""
    a = _grid_args(sc_warp_area_args, _grid_pair("area_variant", src_gt, src_crs, dst_gt, dst_crs, dst_shape), (1, 1))
    rc = _lib.load().sc_warp_area_variant(a)
    if rc < 0:
        _check(rc)
    return {v: k for k, v in AREA_VARIANTS.items()}[rc]


def reproject_like(data, src_gt, src_crs, like, resampling="nearest", nodata=None, min_coverage=0.5, return_coverage=False):
    """:func:`reproject` onto the grid of another raster: ``like`` is an ``io_formats.TiffInfo`` or the path of a GeoTIFF; its shape
    comes from the image, its geotransform from ModelPixelScale + ModelTiepoint or the ModelTransformation tag, its CRS from the
    GeoKeyDirectory (``io_formats.geo_from_tags``).  A file without georeferencing: ValueError."""
    from . import io_formats as io
    info = io.tiff_info(like) if isinstance(like, (str, os.PathLike)) else like
    gt, epsg = io.geo_from_tags(info)
    if gt is None:
        raise ValueError("reproject_like: the target raster carries no georeferencing tags")
    return reproject(data, src_gt, src_crs, gt, epsg, (info.height, info.width), resampling, nodata, min_coverage, return_coverage)
