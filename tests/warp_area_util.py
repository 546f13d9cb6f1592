"""numpy float64 restatement of the footprint resampling of the warp (sc_warp_area / warp.reproject with ``average``, ``max``, ``min``,
``mode``): the corner boxes through ``warp.transform_points``, the per-pixel reduction, and the tie sets the GPU tests leave out.

For destination pixel (r, c): the corners (c, r), (c+1, r), (c, r+1), (c+1, r+1) through the destination affine, the CRS route and
the inverse source affine; the axis-aligned bounding box [u0, u1] x [v0, v1]; its area A; the box clipped to the raster; per source
column / row the overlap with the clipped box, taking part above 2^-20; counting = not the no-data bits, not NaN; coverage =
sum of w over counting samples / A; data when a sample counts and coverage >= min_coverage."""
import math

import numpy as np

from starcop_amd import warp

SLIVER = 2.0 ** -20
PX = 5.4e-4
TH = math.radians(17.0)
ROT5 = (500001.37, 5.0 * math.cos(TH), 5.0 * math.sin(TH), 4100002.71, 5.0 * math.sin(TH), -5.0 * math.cos(TH))
GEO = (-103.94127, PX, 0.0, 32.45231, 0.0, -PX)
#        name: (dst_shape, dst_gt, dst_crs, src_shape, src_gt, src_crs)
GRIDS = {
    "down12_aligned": ((9, 13), (600120.0, 60.0, 0.0, 3590460.0, 0.0, -60.0), 32613,
                       (120, 170), (600120.0, 5.0, 0.0, 3590460.0, 0.0, -5.0), 32613),
    "down_geo": ((23, 31), (600123.37, 60.0, 0.0, 3590456.71, 0.0, -60.0), 32613,
                 (160, 230), (-103.94127, PX / 6, 0.0, 32.45231, 0.0, -PX / 6), 4326),
    "rotated17": ((12, 14), (499990.77, 20.0, 0.0, 4100050.31, 0.0, -20.0), 32611, (40, 30), ROT5, 32611),
    "near_one": ((37, 53), (600123.37, 60.0, 0.0, 3590456.71, 0.0, -60.0), 32613, (60, 90), GEO, 4326),
    "up3": ((37, 72), (600123.37, 20.0, 0.0, 3590456.71, 0.0, -20.0), 32613, (30, 40), GEO, 4326),
    "half_outside": ((19, 36), (598623.37, 120.0, 0.0, 3591756.71, 0.0, -120.0), 32613, (60, 90), GEO, 4326),
    "all_outside": ((9, 13), (650123.37, 60.0, 0.0, 3590456.71, 0.0, -60.0), 32613, (60, 90), GEO, 4326),
    "one_pixel": ((1, 1), (600923.37, 60.0, 0.0, 3589456.71, 0.0, -60.0), 32613,
                  (2, 2), (-103.92727, 20 * PX, 0.0, 32.44931, 0.0, -20 * PX), 4326),
}


def boxes_ref(dst_shape, dst_gt, dst_crs, src_gt, src_crs):
    """(4, H, W) float64 = u0, u1, v0, v1 of every destination pixel, unclipped; NaN where a corner has no coordinates"""
    H, W = dst_shape
    r, c = np.mgrid[0:H + 1, 0:W + 1]
    x, y = warp.apply_geotransform([float(v) for v in dst_gt], c.astype(np.float64), r.astype(np.float64))
    x, y = warp.transform_points(x, y, dst_crs, src_crs)
    inv = warp.invert_geotransform(src_gt)
    u, v = inv[0] + x * inv[1] + y * inv[2], inv[3] + x * inv[4] + y * inv[5]
    us = np.stack([u[:-1, :-1], u[:-1, 1:], u[1:, :-1], u[1:, 1:]])
    vs = np.stack([v[:-1, :-1], v[:-1, 1:], v[1:, :-1], v[1:, 1:]])
    ok = np.isfinite(us).all(0) & np.isfinite(vs).all(0)
    with np.errstate(invalid="ignore"):
        box = np.stack([us.min(0), us.max(0), vs.min(0), vs.max(0)])
    return np.where(ok, box, np.nan)


def _axis(lo, hi, n):
    """clipped interval [max(lo, 0), min(hi, n)] -> (indices that take part, their overlaps, geometric tie)"""
    a, b = max(lo, 0.0), min(hi, float(n))
    if not b > a:
        return np.zeros(0, dtype=np.int64), np.zeros(0), False
    idx = np.arange(int(math.floor(a)), int(math.ceil(b)))
    w = np.minimum(idx + 1.0, b) - np.maximum(idx.astype(np.float64), a)
    tie = bool((np.abs(w - SLIVER) < 1e-8).any())
    # an edge within 1e-6 px of an integer whose sliver pixel still takes part: moving the edge across would drop or add that pixel
    for edge in (a, b):
        d = abs(edge - round(edge))
        tie |= SLIVER < d < 1e-6
    keep = w > SLIVER
    return idx[keep], w[keep], tie


class Footprints:
    """what the planes of a case share: per destination pixel the rows / columns that take part with their overlaps, and A"""

    def __init__(self, boxes, src_shape):
        self.boxes, self.src_shape = boxes, tuple(src_shape)
        H, W = boxes.shape[1:]
        self.shape = (H, W)
        self.pix = {}
        self.geom_tie = np.zeros((H, W), dtype=bool)
        for r in range(H):
            for c in range(W):
                u0, u1, v0, v1 = boxes[:, r, c]
                if not np.isfinite(u0):
                    continue
                js, wx, tx = _axis(u0, u1, src_shape[1])
                is_, wy, ty = _axis(v0, v1, src_shape[0])
                self.geom_tie[r, c] = tx or ty
                if len(js) and len(is_):
                    self.pix[(r, c)] = (is_, js, wy[:, None] * wx[None, :], (u1 - u0) * (v1 - v0))


def counting(plane, nodata):
    plane = np.asarray(plane)
    if plane.dtype == np.float32:
        return (plane.view(np.uint32) != np.array(nodata, dtype=np.float32).view(np.uint32)) & ~np.isnan(plane)
    return plane != np.array(nodata, dtype=plane.dtype)


def reduce_ref(plane, nodata, fp, mode, min_coverage=0.5):
    """one plane -> (value, coverage, valid, tie): value float64 (average, BEFORE the rounding to float32) or the plane's dtype
    (max / min / mode), meaningful where ``valid``; coverage float64 as computed (also where it stays below min_coverage);
    tie = the pixels a comparison leaves out: a geometric tie or a coverage within 1e-9 of min_coverage"""
    plane = np.asarray(plane)
    H, W = fp.shape
    cnt = counting(plane, nodata)
    val = np.zeros((H, W), dtype=np.float64 if mode == "average" else plane.dtype)
    cov, valid = np.zeros((H, W)), np.zeros((H, W), dtype=bool)
    tie = fp.geom_tie.copy()
    for (r, c), (is_, js, w, area) in fp.pix.items():
        m = cnt[np.ix_(is_, js)]
        if not m.any():
            continue
        sub = plane[np.ix_(is_, js)]
        cw = float((w * m).sum())
        cov[r, c] = cw / area
        if min_coverage > 0.0 and abs(cov[r, c] - min_coverage) < 1e-9:
            tie[r, c] = True
        if cov[r, c] >= min_coverage:
            valid[r, c] = True
            if mode == "average":
                val[r, c] = float((w * np.where(m, sub, 0).astype(np.float64)).sum()) / cw
            elif mode == "max":
                val[r, c] = sub[m].max()
            elif mode == "min":
                val[r, c] = sub[m].min()
            elif mode == "mode":
                val[r, c] = np.bincount(sub[m], minlength=256).argmax()          # the first of equal counts: the smallest value
            else:
                raise ValueError(mode)
    return val, cov, valid, tie


def seeded_plane(src_shape, seed=11, kind="holes"):
    """as test_gpu_warp.bilinear_plane: about 8 % no-data (-9999), about 4 % NaN, and a no-data block over rows 10:24, columns 20:41"""
    Hs, Ws = src_shape
    rng = np.random.default_rng(seed)
    if kind == "constant":
        a = np.full((Hs, Ws), 1234.5678, dtype=np.float32)
    else:
        a = (rng.standard_normal((Hs, Ws)) * 300 + 200).astype(np.float32)
    if kind != "dense":
        a[rng.random((Hs, Ws)) < 0.08] = -9999.0
        a[rng.random((Hs, Ws)) < 0.04] = np.nan
        a[10:24, 20:41] = -9999.0
    return a


def class_map(src_shape, classes, seed=11):
    """uint8 class map with `classes` distinct values in blobs of a few pixels (so that a mode exists), plus salt noise; at least `classes` pixels"""
    Hs, Ws = src_shape
    rng = np.random.default_rng(seed + classes)
    coarse = rng.integers(0, classes, size=((Hs + 3) // 4, (Ws + 4) // 5))
    a = np.kron(coarse, np.ones((4, 5), dtype=np.int64))[:Hs, :Ws]
    noise = rng.random((Hs, Ws)) < 0.3
    a = np.where(noise, rng.integers(0, classes, size=(Hs, Ws)), a)
    a.reshape(-1)[rng.choice(Hs * Ws, size=classes, replace=False)] = np.arange(classes)      # every class is there
    return (a * (256 // classes) if classes < 256 else a).astype(np.uint8)
