"""Orthorectification through a geometry look-up table (GLT) on the MI355X: what ``EMITImage.georreference`` does to the outputs
of the reference's ``mag1c_emit`` (starcop/models/mag1c_emit.py:86-88, its ``georreferenced=True`` default; the gather is
restated in the note at :206-221)

    out[i, j] = data[glt_y[i, j] - 1, glt_x[i, j] - 1]   where glt_x[i, j] != 0 and glt_y[i, j] != 0,   fill elsewhere

for any number of planes in one ``sc_glt_ortho`` launch (include/starcop_hip.h), and the GeoTIFF tags of the orthorectified
grid.  The kernel copies elements as 1-, 2-, 4- or 8-byte words, so the result is bit-equal to the numpy gather for every dtype
of those widths.  There is no CPU fallback.
"""
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check as _check, sc_ortho_args, stream
from .planes import as_planes, chunks, fill_bits, numpy_dtype, per_plane, set_planes

NOUT_MAX = _lib.ORTHO_MAX_PLANES


def _glt_device(g, dev):
    """one GLT word plane -> dense int32 device tensor (a dense int32 device tensor is used as it is)"""
    if isinstance(g, torch.Tensor):
        if g.dim() != 2 or g.dtype.is_floating_point or g.dtype == torch.bool:
            raise ValueError(f"georeference: the GLT must be a 2-D integer array, got {g.dtype} {tuple(g.shape)}")
        return g.to(device=dev, dtype=torch.int32).contiguous()
    a = np.asarray(g)
    if a.ndim != 2 or a.dtype.kind not in "iu":
        raise ValueError(f"georeference: the GLT must be a 2-D integer array, got {a.dtype} {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def georeference(data, glt_x, glt_y, fill_value_default=-9999.0, absolute=False, check=True, shape=None):
    """``EMITImage.georreference(data, fill_value_default)`` on the GPU for one or many planes.

    ``data``: a device tensor (rows, cols) or (P, rows, cols) with any non-negative strides -- ``cube.permute(2, 0, 1)`` of a
    pixel-interleaved (rows, cols, C) cube and column slices are read in place --, a list of 2-D tensors of one dtype, or a numpy
    array (numpy in, numpy out).  ``glt_x`` / ``glt_y``: (H_o, W_o) integer arrays (numpy or device): 1-based column / row of the
    swath for every pixel of the orthorectified grid, 0 = no data; ``absolute=True`` takes their absolute values (AVIRIS-NG GLTs
    mark interpolated pixels with a negative index).  ``fill_value_default``: a scalar, or one value per plane.
    ``shape=(rows, cols)``: the swath the GLT indexes when the planes of a list are smaller than it (the network output is the
    swath cropped at the bottom / right to multiples of 32): pixels beyond a plane get its fill value.
    Returns (H_o, W_o) for 2-D input, else (P, H_o, W_o), contiguous, in the dtype of the input.

    GLT entries that point outside the swath are never dereferenced: the pixel gets the fill value and is counted on the device;
    ``check=True`` reads the counter back once and raises ``ValueError`` with the count, ``check=False`` skips the read-back."""
    who = "georeference"
    planes, single, host = as_planes(data, who, "a tensor (rows, cols) or (P, rows, cols), a numpy array or a list of 2-D tensors",
                                     TypeError, same_shape=False)
    dt = planes[0].dtype
    nd = numpy_dtype(dt, who)
    if shape is None:
        rows, cols = (int(v) for v in planes[0].shape)
        if any(tuple(p.shape) != (rows, cols) for p in planes):
            raise ValueError("georeference: planes of different shapes need shape=(rows, cols) of the swath")
    else:
        rows, cols = (int(v) for v in shape)
    if rows < 1 or cols < 1 or any(p.shape[0] < 1 or p.shape[1] < 1 or p.shape[0] > rows or p.shape[1] > cols for p in planes):
        raise ValueError(f"georeference: every plane must be non-empty and inside the {rows} x {cols} swath")
    P = len(planes)
    bits = [fill_bits(v, nd, who) for v in per_plane(fill_value_default, P, who, "fill values")]
    _lib.require_device(None if host else planes[0])
    if host:
        planes = [p.cuda() for p in planes]
    dev = planes[0].device
    lib = _lib.load()
    gx, gy = _glt_device(glt_x, dev), _glt_device(glt_y, dev)
    if gx.shape != gy.shape:
        raise ValueError("georeference: glt_x and glt_y differ in shape")
    Ho, Wo = (int(v) for v in gx.shape)
    if Ho < 1 or Wo < 1:
        raise ValueError("georeference: empty GLT")
    out = torch.empty((P, Ho, Wo), dtype=dt, device=dev)
    oob = torch.zeros(1, dtype=torch.int64, device=dev) if check else None
    for p0, n in chunks(P, NOUT_MAX):
        a = sc_ortho_args()
        a.glt_x, a.glt_y = gx.data_ptr(), gy.data_ptr()
        a.out_h, a.out_w, a.rows, a.cols = Ho, Wo, rows, cols
        a.P, a.elem_bytes, a.absolute = n, nd.itemsize, int(bool(absolute))
        set_planes(a, planes, p0, rows=a.plane_rows, cols=a.plane_cols)
        a.fill_bits[:n] = bits[p0:p0 + n]
        a.out = out[p0].data_ptr()
        a.oob_count = oob.data_ptr() if oob is not None and p0 == 0 else None      # the GLT is the same for every chunk
        _check(lib.sc_glt_ortho(a, stream()))
    if oob is not None:
        bad = int(oob.item())
        if bad:
            raise ValueError(f"georeference: {bad} GLT entries point outside the {rows} x {cols} swath"
                             + ("" if absolute else " (negative entries need absolute=True)"))
    res = out[0] if single else out
    return res.cpu().numpy() if host else res


def emit_geo_tags(geotransform: Sequence[float], spatial_ref: Optional[str] = None) -> Dict[int, tuple]:
    """GeoTIFF tags of the orthorectified grid of an EMIT granule: ``geotransform`` is the granule's root attribute of that name,
    six numbers in GDAL order (x of the upper-left corner, pixel width, row rotation, y of the upper-left corner, column
    rotation, pixel height (negative: north up)); ``spatial_ref`` its WKT, WGS-84 geographic for every EMIT product.  Returns
    ModelPixelScale (33550) + ModelTiepoint (33922) and the geographic GeoKeyDirectory (34735) ``io_formats.envi_geo_tags`` writes
    for ``Geographic Lat/Lon``.  Rotation terms other than 0 raise ``NotImplementedError``, and so does a ``spatial_ref`` that
    does not name WGS 84."""
    gt = [float(v) for v in np.asarray(geotransform, dtype=np.float64).ravel()]
    if len(gt) != 6:
        raise ValueError(f"emit_geo_tags: geotransform must have 6 numbers, got {len(gt)}")
    x0, dx, rx, y0, ry, dy = gt
    if rx != 0.0 or ry != 0.0:
        raise NotImplementedError(f"emit_geo_tags: rotated geotransform (terms {rx}, {ry}) is not supported")
    if dx <= 0.0 or dy >= 0.0:
        raise NotImplementedError(f"emit_geo_tags: only north-up grids (pixel width > 0, pixel height < 0), got {dx}, {dy}")
    if spatial_ref is not None:
        s = spatial_ref.decode("latin-1") if isinstance(spatial_ref, bytes) else str(spatial_ref)
        if not any(k in s.replace("_", " ").upper() for k in ("WGS 84", "WGS84", "WGS 1984", "4326")):
            raise NotImplementedError("emit_geo_tags: only WGS-84 geographic coordinates are supported")
    return {33550: (12, (dx, -dy, 0.0)),
            33922: (12, (0.0, 0.0, 0.0, x0, y0, 0.0)),
            # header (version 1, revision 1.0, 3 keys), GTModelType = geographic, GTRasterType = PixelIsArea, GeographicType = WGS 84
            34735: (3, (1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326))}
