"""Mosaics on the MI355X (``sc_mosaic``, include/starcop_hip.h): N rasters on grids of their own composed into one raster on a
destination grid in one launch, and the host side that goes with it.

Per destination pixel the kernel computes the source coordinates in every source whose footprint box meets the pixel's tile -- the
projection of :mod:`starcop_amd.warp`, with the inverse series of a UTM destination summed once per pixel and not once per source
-- and applies a rule:

``first`` / ``last``  the valid source with the lowest / highest number wins (any 1-, 2-, 4- or 8-byte dtype);
``max`` / ``min``     float32: the valid source whose NEAREST element of the key plane is largest / smallest wins; equal values go
                      to the lower number;
``index``             the winner of every pixel is given (``select``, int32; values outside [0, N) mean none);
``mean``              float32: per plane the mean of the valid sources' samples that count, summed in fp64 in source order.

A source is valid at a pixel when the pixel lies inside it and the nearest element of its plane ``key`` is not the no-data value
(and not NaN for float32 / float64); ``key=-1`` lets the footprint alone decide.  The planes of the winner are sampled as
``warp.reproject`` samples them (``nearest`` or, float32, ``bilinear``), so a mosaic of one source with ``key=-1`` is its warp.
``index`` (the winner, -1 for none) says which scene a pixel came from; ``count`` how many sources were valid.  No CPU fallback."""
import ctypes
import math

import numpy as np
import torch

from . import _lib, warp
from ._lib import check as _check, sc_mosaic_args, sc_mosaic_source, stream
from .planes import as_planes, fill_bits, numpy_dtype, per_plane, set_planes

MAX_SOURCES = _lib.MOSAIC_MAX_SOURCES
MAX_PLANES = _lib.WARP_MAX_PLANES
MEAN_PLANES = _lib.MOSAIC_MEAN_PLANES
RULES = {"first": _lib.MOSAIC_FIRST, "last": _lib.MOSAIC_LAST, "max": _lib.MOSAIC_MAX, "min": _lib.MOSAIC_MIN,
         "mean": _lib.MOSAIC_MEAN, "index": _lib.MOSAIC_BY_INDEX}


# ---------------------------------------------------------------------------------------------- grids (host)
def footprint_box(src_shape, src_gt, src_crs, dst_gt, dst_crs, dst_shape):
    """``(r0, r1, c0, c1)``: a half-open box of destination pixels outside of which the source has no pixel.  The source outline
    -- every pixel corner along its four edges, as ``warp.suggest_grid`` takes it -- is transformed to the destination CRS and pushed
    through the inverse destination affine; the box is floor(min) - 1 .. ceil(max) + 1, clipped to the grid (empty, r0 >= r1 or
    c0 >= c1, for a source that misses the grid).  If any outline point has no coordinates the box is the whole grid."""
    H, W = (int(v) for v in src_shape)
    Hd, Wd = (int(v) for v in dst_shape)
    if H < 1 or W < 1:
        raise ValueError(f"footprint_box: empty source {src_shape}")
    gt = warp.gt6(src_gt, "footprint_box")
    inv = warp.invert_geotransform(dst_gt)
    cols = np.concatenate([np.arange(W + 1.0), np.full(H + 1, float(W)), np.arange(W + 1.0), np.zeros(H + 1)])
    rows = np.concatenate([np.zeros(W + 1), np.arange(H + 1.0), np.full(W + 1, float(H)), np.arange(H + 1.0)])
    x, y = warp.transform_points(*warp.apply_geotransform(gt, cols, rows), src_crs, dst_crs)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return 0, Hd, 0, Wd
    c = inv[0] + x * inv[1] + y * inv[2]
    r = inv[3] + x * inv[4] + y * inv[5]
    clip = lambda v, hi: int(min(max(v, 0), hi))
    return (clip(math.floor(r.min()) - 1, Hd), clip(math.ceil(r.max()) + 1, Hd),
            clip(math.floor(c.min()) - 1, Wd), clip(math.ceil(c.max()) + 1, Wd))


def union_grid(grids, dst_crs, resolution=None):
    """One north-up grid in ``dst_crs`` that covers every ``(shape, gt, crs)`` of ``grids`` -> ``(shape, gt)``: the union of their
    ``warp.suggest_grid``.  The default ``resolution`` is the finest of the per-source suggestions.  Every suggestion is snapped
    outward to multiples of the resolution, so the union is the minimum / maximum of lattice indices and each scene's pixels fall
    on the lattice it would have alone.  A grid of 2^31 pixels or more is refused."""
    grids = list(grids)
    if not grids:
        raise ValueError("union_grid: no grids")
    if resolution is None:
        resolution = min(warp.suggest_grid(s, g, c, dst_crs)[1][1] for s, g, c in grids)
    res = float(resolution)
    if not (math.isfinite(res) and res > 0.0):
        raise ValueError(f"union_grid: resolution {resolution!r}")
    i0 = j0 = i1 = j1 = None
    for s, g, c in grids:
        (h, w), gt = warp.suggest_grid(s, g, c, dst_crs, res)
        a, b = round(gt[0] / res), round(gt[3] / res)               # lattice indices of the upper left corner
        i0, i1 = (a, a + w) if i0 is None else (min(i0, a), max(i1, a + w))
        j1, j0 = (b, b - h) if j1 is None else (max(j1, b), min(j0, b - h))
    Hd, Wd = j1 - j0, i1 - i0
    if Hd * Wd >= 2 ** 31:
        raise ValueError(f"union_grid: {Hd} x {Wd} pixels at resolution {res}: 2^31 pixels or more")
    return (Hd, Wd), (i0 * res, res, 0.0, j1 * res, 0.0, -res)


# ---------------------------------------------------------------------------------------------- the device side
def _code(crs):
    return 0 if crs is None else int(crs)


def _launch(lib, srcs, planes_of, idx, nd, bits, dgt, d_code, dst_shape, boxes, rule, key, mode, out, index, count, select):
    """one sc_mosaic call on the planes ``idx`` of every source"""
    N, n = len(srcs), len(idx)
    table = (sc_mosaic_source * N)()
    for s, (shape, inv, code) in enumerate(srcs):
        q = table[s]
        q.src_inv[:], q.src_crs, (q.src_h, q.src_w), q.box[:] = inv, code, shape, boxes[s]
        set_planes(q, [planes_of[s][p] for p in idx])
    a = sc_mosaic_args()
    a.dst_gt[:], a.dst_crs, (a.out_h, a.out_w) = dgt, d_code, dst_shape
    a.N, a.P, a.elem_bytes, a.rule, a.key_plane, a.resampling = N, n, nd.itemsize, rule, key, mode
    a.flags = _lib.MOSAIC_KEY_FLOAT if key >= 0 and nd.kind == "f" and nd.itemsize in (4, 8) else 0
    a.nodata_bits[:n] = [bits[p] for p in idx]
    a.sources = ctypes.cast(table, ctypes.POINTER(sc_mosaic_source))
    dev_table = torch.empty(ctypes.sizeof(table), dtype=torch.uint8, device=out.device)
    a.table, a.out = dev_table.data_ptr(), out.data_ptr()
    a.index = index.data_ptr() if index is not None else None
    a.count = count.data_ptr() if count is not None else None
    a.select = select.data_ptr() if select is not None else None
    _check(lib.sc_mosaic(a, stream()))


def mosaic(sources, dst_gt, dst_crs, dst_shape, rule="first", key=0, resampling="nearest", nodata=None, return_index=False,
           return_count=False, select=None):
    """``sources`` -- a list of ``(data, gt, crs)`` -- composed onto the grid ``(dst_shape, dst_gt, dst_crs)`` on the GPU.

    ``data`` as in ``warp.reproject``: a device tensor (H, W) or (P, H, W) with any non-negative strides (read in place), a list of
    2-D tensors, or a numpy array (numpy in, numpy out); all sources share one dtype and plane count, shapes and grids are their
    own.  ``rule``: ``"first"``, ``"last"``, ``"max"``, ``"min"``, ``"mean"`` or ``"index"`` (see the module text); ``key``: the
    plane that decides validity and, for max / min, the winner; -1 for the footprint alone.  ``nodata``: a scalar or one value per
    plane (default 0), shared by all sources: what a pixel without a winner gets and what does not count in a source.
    ``select``: for ``"index"``, the int32 (H_d, W_d) winner of every pixel.  At most 64 sources per call; any number of planes
    (32 per launch: further launches reuse the first one's index; ``mean``: 4 per launch).  CRS pairs are those of
    ``warp.reproject``.  Returns ``out`` -- (H_d, W_d) when the sources are 2-D, else (P, H_d, W_d) -- or ``(out, index?,
    count?)`` with ``return_index`` / ``return_count``: int32 (H_d, W_d), the winner (-1: none; not for ``mean``) and the number
    of valid sources (not for ``index``)."""
    who = "mosaic"
    if rule not in RULES:
        raise ValueError(f"{who}: rule {rule!r}; expected one of {sorted(RULES)}")
    if resampling not in warp.POINT_RESAMPLING:         # the footprint modes of warp.reproject are not part of the mosaic
        raise ValueError(f"{who}: resampling {resampling!r}; expected one of {sorted(warp.POINT_RESAMPLING)}")
    sources = list(sources)
    N = len(sources)
    if N < 1 or N > MAX_SOURCES:
        raise ValueError(f"{who}: {N} sources; one call takes 1 to {MAX_SOURCES}")
    dgt = warp.gt6(dst_gt, who)
    Hd, Wd = warp.dst_grid_shape(dst_shape, who)
    parsed = [as_planes(d, who, same_shape=False) for d, _, _ in sources]
    host, single = parsed[0][2], all(p[1] for p in parsed)
    P = len(parsed[0][0])
    dts = {str(pl[0].dtype).replace("torch.", "") for pl, _, _ in parsed}            # as_planes: one dtype and device per source
    if len(dts) != 1 or any(len(pl) != P for pl, _, _ in parsed):
        raise ValueError(f"{who}: all sources share one dtype and plane count; got dtypes {sorted(dts)}, plane counts "
                         f"{[len(pl) for pl, _, _ in parsed]}")
    first = parsed[0][0][0]
    nd = numpy_dtype(first.dtype, who)
    if nd != np.float32 and (rule in ("max", "min", "mean") or resampling == "bilinear"):
        raise ValueError(f"{who}: the rules max, min and mean and bilinear resampling are defined for float32, not {nd}")
    key = int(key)
    if not -1 <= key < P:
        raise ValueError(f"{who}: key plane {key} outside [-1, {P})")
    if rule in ("max", "min") and key < 0:
        raise ValueError(f"{who}: rule {rule!r} needs a key plane")
    if (rule == "index") != (select is not None):
        raise ValueError(f"{who}: `select` goes with rule 'index' and only with it")
    if rule == "index" and return_count:
        raise ValueError(f"{who}: rule 'index' consults no validity: there is no count")
    if rule == "mean" and return_index:
        raise ValueError(f"{who}: rule 'mean' has no winner: there is no index")
    if select is not None:
        sel_dt = str(select.dtype).replace("torch.", "")
        if tuple(select.shape) != (Hd, Wd) or sel_dt != "int32":
            raise ValueError(f"{who}: `select` must be int32 {(Hd, Wd)}, got {sel_dt} {tuple(select.shape)}")
    d_code = _code(dst_crs)
    srcs = []
    for (pl, _, _), (_, gt, crs) in zip(parsed, sources):
        warp.crs_pair(crs, dst_crs, who)
        shape = tuple(int(v) for v in pl[0].shape)
        if shape[0] < 1 or shape[1] < 1 or any(tuple(p.shape) != shape for p in pl):
            raise ValueError(f"{who}: the planes of a source share one non-empty shape")
        srcs.append((shape, warp.invert_geotransform(gt), _code(crs)))
    bits = [fill_bits(v, nd, who) for v in per_plane(nodata, P, who, "nodata values", default=0)]
    boxes = [footprint_box(shape, gt, crs, dgt, dst_crs, (Hd, Wd)) for (shape, _, _), (_, gt, crs) in zip(srcs, sources)]
    # ---- the device from here on
    _lib.require_device(None if host else first)
    dev = torch.device("cuda", torch.cuda.current_device()) if host else first.device
    planes_of = []
    for pl, _, is_np in parsed:
        if is_np:
            pl = [p.to(dev) for p in pl]
        if pl[0].device != dev:
            raise ValueError(f"{who}: all planes live on one device")
        planes_of.append(pl)
    if select is not None:
        select = (torch.from_numpy(np.ascontiguousarray(select)) if isinstance(select, np.ndarray) else select).to(dev).contiguous()
    lib = _lib.load()
    mode = warp.RESAMPLING[resampling]
    out = torch.empty((P, Hd, Wd), dtype=planes_of[0][0].dtype, device=dev)
    count = torch.empty((Hd, Wd), dtype=torch.int32, device=dev) if return_count else None
    args = (lib, srcs, planes_of)
    tail = (nd, bits, dgt, d_code, (Hd, Wd), boxes)
    index = None
    if rule == "mean":
        if P <= MEAN_PLANES:
            _launch(*args, list(range(P)), *tail, RULES[rule], key, mode, out, None, count, None)
        else:                                                       # the key plane rides along in the last slot of every launch
            rest = [p for p in range(P) if p != key]
            step = MEAN_PLANES - (1 if key >= 0 else 0)
            for q0 in range(0, len(rest), step):
                idx = rest[q0:q0 + step] + ([key] if key >= 0 else [])
                tmp = torch.empty((len(idx), Hd, Wd), dtype=out.dtype, device=dev)
                _launch(*args, idx, *tail, RULES[rule], len(idx) - 1 if key >= 0 else -1, mode, tmp, None, count if q0 == 0 else None, None)
                for k, p in enumerate(idx):
                    out[p] = tmp[k]
    else:
        chunks = [list(range(p0, min(P, p0 + MAX_PLANES))) for p0 in range(0, P, MAX_PLANES)]
        if rule == "index":
            index = select
        else:
            lead = next(c for c in chunks if key < 0 or key in c)      # the launch that decides the winners
            index = torch.empty((Hd, Wd), dtype=torch.int32, device=dev) if return_index or len(chunks) > 1 else None
            _launch(*args, lead, *tail, RULES[rule], lead.index(key) if key >= 0 else -1, mode, out[lead[0]:], index, count, None)
            chunks.remove(lead)
        for c in chunks:
            _launch(*args, c, *tail, RULES["index"], -1, mode, out[c[0]:], None, None, index)
    res = [out[0] if single else out] + ([index] if return_index else []) + ([count] if return_count else [])
    if host:
        res = [r.cpu().numpy() for r in res]
    return res[0] if len(res) == 1 else tuple(res)
