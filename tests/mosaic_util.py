"""The shared scene of the mosaic tests and the numpy restatement of sc_mosaic / starcop_amd.mosaic: per source the restated
coordinates, nearest gather and float64 bilinear interpolation of tests/warp_util.py, and the rule applied in numpy.  The
restatement has no cull and no shared inverse: every source is projected on its own."""
import functools
import math

import numpy as np

import warp_util as U

PX = 5.4e-4
TH = math.radians(17.0)
DST_GT = (600123.37, 60.0, 0.0, 3590456.71, 0.0, -60.0)
DST_CRS = 32613
#         vector path, 3 x 2 tiles; one pixel per thread; the last tile column meets no box
SHAPES = ((45, 88), (45, 85), (45, 152))
#         name, shape, geotransform, CRS: offsets that look irrational keep pixel centres off cell boundaries
SOURCES = (
    ("geo_a", (60, 56), (-103.94127, PX, 0.0, 32.45231, 0.0, -PX), 4326),
    ("geo_b", (50, 60), (-103.92313, PX, 0.0, 32.44817, 0.0, -PX), 4326),
    ("utm_same", (30, 40), (602251.13, 60.0, 0.0, 3589907.29, 0.0, -60.0), 32613),
    ("utm_rot", (40, 30), (601500.77, 45.0 * math.cos(TH), 45.0 * math.sin(TH), 3589402.71, 45.0 * math.sin(TH), -45.0 * math.cos(TH)), 32613),
    ("zone14", (24, 30), (38100.29, 60.0, 0.0, 3599650.83, 0.0, -60.0), 32614),
    ("far", (20, 20), (650123.37, 60.0, 0.0, 3590456.71, 0.0, -60.0), 32613),
)
N = len(SOURCES)
NODATA = -9999.0
NP_DTYPES = ("uint8", "int16", "float32", "float64")


@functools.lru_cache(maxsize=None)
def coords(shape):
    """tuple of the restated (2, H, W) (u, v) of every source on the destination of ``shape``, NaN outside; computed once, read-only"""
    out = []
    for _, ss, sgt, scrs in SOURCES:
        uv = U.source_coords_ref(shape, DST_GT, DST_CRS, sgt, scrs, ss)
        uv.setflags(write=False)
        out.append(uv)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def compared(shape):
    """the pixels that take part in comparisons: all but those within 1e-6 px of a cell boundary of ANY source; at most 0.1 % may be
    left out (asserted on the restatement alone; with these geotransforms none is)"""
    near = np.zeros(shape, dtype=bool)
    for uv in coords(shape):
        near |= U.near_boundary(uv)
    assert near.mean() <= 1e-3, (shape, near.mean())
    keep = ~near
    keep.setflags(write=False)
    return keep


def inside(shape):
    return np.stack([np.isfinite(uv[0]) for uv in coords(shape)])


def float_planes(P, seed=0):
    """per source (P, Hs, Ws) float32: values around 200 +- 300 with no-data holes (-9999), NaNs -- some with payloads --, -0.0 and
    infinities; plane 0 is the usual key"""
    out = []
    for i, (_, (Hs, Ws), _, _) in enumerate(SOURCES):
        rng = np.random.default_rng(1000 * seed + i)
        a = (rng.standard_normal((P, Hs, Ws)) * 300 + 200).astype(np.float32)
        a[rng.random((P, Hs, Ws)) < 0.08] = NODATA
        a[rng.random((P, Hs, Ws)) < 0.04] = np.nan
        a[:, 10:14, 12:21] = NODATA
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=max(6, flat.size // 50), replace=False)
        flat[idx[0::3]] = -0.0
        flat[idx[1::3]] = np.inf
        flat.view(np.uint32)[idx[2::3]] = np.array(np.nan, dtype=np.float32).view(np.uint32) | 0x1234      # a NaN with a payload
        out.append(a)
    return out


def typed_planes(dt, P, seed=0):
    """per source (P, Hs, Ws) of dtype dt: integers over the whole range; floats as warp's test planes (NaNs with payloads, -0.0, inf)"""
    nd = np.dtype(dt)
    if nd == np.float32:
        return float_planes(P, seed)
    out = []
    for i, (_, (Hs, Ws), _, _) in enumerate(SOURCES):
        rng = np.random.default_rng(1000 * seed + 77 + i)
        if nd.kind == "f":
            a = rng.standard_normal((P, Hs, Ws)).astype(nd) * 100
            flat = a.reshape(-1)
            idx = rng.choice(flat.size, size=max(4, flat.size // 20), replace=False)
            flat[idx[0::4]] = np.nan
            flat[idx[1::4]] = -0.0
            flat[idx[2::4]] = np.inf
            flat.view(f"u{nd.itemsize}")[idx[3::4]] = np.array(np.nan, dtype=nd).view(f"u{nd.itemsize}") | 0x1234
            a[rng.random((P, Hs, Ws)) < 0.08] = NODATA
        else:
            info = np.iinfo(nd)
            a = rng.integers(info.min, info.max, size=(P, Hs, Ws), endpoint=True).astype(nd)
            a[rng.random((P, Hs, Ws)) < 0.08] = nodata_for(dt)
        out.append(a)
    return out


def nodata_for(dt):
    return NODATA if np.dtype(dt).kind == "f" else {"uint8": 255, "int16": -9999}[str(np.dtype(dt))]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def key_counts(sample, nodata):
    """a nearest sample of the key plane counts: its bits differ from the no-data value's and, for floats, it is not NaN"""
    ok = _bits(sample) != _bits(np.array(nodata, dtype=sample.dtype))
    if sample.dtype.kind == "f":
        ok &= ~np.isnan(sample)
    return ok


def mosaic_ref(planes, shape, rule, key=0, resampling="nearest", nodata=NODATA, select=None, sources=None):
    """-> dict: ``out`` (nearest: (P, H, W) in the planes' dtype; bilinear / mean: float64 BEFORE the one rounding, NaN where the
    result is no-data), ``nodata`` (P, H, W) bool: the pixel gets the plane's no-data, ``index`` (winner or -1; None for mean),
    ``count`` (valid sources; None for index).  ``sources``: the numbers of SOURCES that take part (default all), renumbered from 0."""
    which = list(range(N)) if sources is None else list(sources)
    P = planes[0].shape[0]
    dt = planes[0].dtype
    uvs = [coords(shape)[s] for s in which]
    ins = [np.isfinite(uv[0]) for uv in uvs]
    near = [U.nearest_ref(planes[s], uv, [nodata] * P) for s, uv in zip(which, uvs)]             # (P, H, W) per source
    valid = [i & (key_counts(n[key], nodata) if key >= 0 else True) for i, n in zip(ins, near)]
    count = np.sum(valid, axis=0).astype(np.int32)
    if resampling == "bilinear":
        samp, has = [], []
        for s, uv in zip(which, uvs):
            r = [U.bilinear_ref(planes[s][p], uv, nodata) for p in range(P)]
            samp.append(np.stack([v for v, _ in r]))
            has.append(np.stack([m for _, m in r]))
    if rule == "mean":
        tot, terms = np.zeros((P,) + shape), np.zeros((P,) + shape, dtype=np.int64)
        for k in range(len(which)):
            for p in range(P):
                if resampling == "bilinear":
                    ok, val = valid[k] & has[k][p], samp[k][p]
                else:
                    ok, val = valid[k] & key_counts(near[k][p], nodata), near[k][p].astype(np.float64)
                tot[p] += np.where(ok, np.where(ok, val, 0.0), 0.0)
                terms[p] += ok
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.where(terms > 0, tot / terms, np.nan)
        return {"out": out, "nodata": terms == 0, "index": None, "count": count}
    index = np.full(shape, -1, dtype=np.int32)
    if rule == "index":
        for k in range(len(which)):
            index[(select == k) & ins[k]] = k
        count = None
    elif rule == "first":
        for k in reversed(range(len(which))):
            index[valid[k]] = k
    elif rule == "last":
        for k in range(len(which)):
            index[valid[k]] = k
    else:
        best = np.zeros(shape, dtype=np.float32)
        for k in range(len(which)):
            kv = near[k][key]
            with np.errstate(invalid="ignore"):
                better = kv > best if rule == "max" else kv < best
            take = valid[k] & ((index < 0) | better)
            index[take] = k
            best = np.where(take, kv, best)
    if resampling == "bilinear":
        out, nod = np.full((P,) + shape, np.nan), np.ones((P,) + shape, dtype=bool)
        for k in range(len(which)):
            m = index == k
            out[:, m] = samp[k][:, m]
            nod[:, m] = ~has[k][:, m]
        return {"out": out, "nodata": nod, "index": index, "count": count}
    out = np.full((P,) + shape, nodata, dtype=dt)
    for k in range(len(which)):
        m = index == k
        out[:, m] = near[k][:, m]
    return {"out": out, "nodata": np.broadcast_to(index < 0, out.shape), "index": index, "count": count}


def gate(planes):
    """2 * 2^-24 * max|x| over the finite values that count: one float32 rounding, doubled for a last-place flip of the float64 quotient"""
    m = 0.0
    for a in planes:
        f = a[np.isfinite(a) & (a != NODATA)]
        m = max(m, float(np.abs(f).max()))
    return 2 * 2.0 ** -24 * m
