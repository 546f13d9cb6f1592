"""numpy restatements of the warp (sc_warp / starcop_amd.warp): Snyder's Transverse Mercator series as a projection that shares no
term with the Krueger series under test, the source coordinates of a destination grid, the nearest gather and the float64 bilinear
interpolation with renormalised weights."""
import numpy as np

from starcop_amd import warp

A, F, K0 = 6378137.0, 1.0 / 298.257223563, 0.9996
E2 = F * (2.0 - F)


def snyder_forward(lon, lat, lon0, false_northing=0.0):
    """longitude / latitude (degrees) -> UTM easting / northing by Snyder, Map Projections: A Working Manual (USGS PP 1395), eq.
    8-9 ... 8-15 with 3-21 for M: a power series in the longitude difference A = (lon - lon0) cos(lat), truncated at A^6 (y) and
    A^5 (x)"""
    phi, lam = np.radians(np.asarray(lat, dtype=np.float64)), np.radians(np.asarray(lon, dtype=np.float64) - lon0)
    ep2 = E2 / (1.0 - E2)                                                      # 8-12
    N = A / np.sqrt(1.0 - E2 * np.sin(phi) ** 2)                               # 4-20
    T, C, Al = np.tan(phi) ** 2, ep2 * np.cos(phi) ** 2, lam * np.cos(phi)     # 8-13, 8-14, 8-15
    M = A * ((1 - E2 / 4 - 3 * E2 ** 2 / 64 - 5 * E2 ** 3 / 256) * phi - (3 * E2 / 8 + 3 * E2 ** 2 / 32 + 45 * E2 ** 3 / 1024) * np.sin(2 * phi)
             + (15 * E2 ** 2 / 256 + 45 * E2 ** 3 / 1024) * np.sin(4 * phi) - (35 * E2 ** 3 / 3072) * np.sin(6 * phi))      # 3-21
    x = K0 * N * (Al + (1 - T + C) * Al ** 3 / 6 + (5 - 18 * T + T ** 2 + 72 * C - 58 * ep2) * Al ** 5 / 120)               # 8-9
    y = K0 * (M + N * np.tan(phi) * (Al ** 2 / 2 + (5 - T + 9 * C + 4 * C ** 2) * Al ** 4 / 24
                                     + (61 - 58 * T + T ** 2 + 600 * C - 330 * ep2) * Al ** 6 / 720))                      # 8-10
    return 500000.0 + x, false_northing + y


def seeded_points(n=200_000, seed=20240607, max_dlon=3.5):
    """(lon, lat, lon0, epsg) of n points: latitude in [-80, 84], |lon - lon0| <= max_dlon, zones 1..60, the hemisphere of the latitude"""
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-80.0, 84.0, n)
    zone = rng.integers(1, 61, n)
    lon0 = 6.0 * zone - 183.0
    lon = lon0 + rng.uniform(-max_dlon, max_dlon, n)
    return lon, lat, lon0, np.where(lat < 0, 32700, 32600) + zone


def source_coords_ref(dst_shape, dst_gt, dst_crs, src_gt, src_crs, src_shape=None):
    """(2, H, W) float64: (u, v) of every destination pixel centre in source pixel coordinates; NaN where the projection gives
    none and, with ``src_shape``, outside [0, W_s) x [0, H_s)"""
    H, W = dst_shape
    r, c = np.mgrid[0:H, 0:W]
    x, y = warp.apply_geotransform([float(v) for v in dst_gt], c + 0.5, r + 0.5)
    x, y = warp.transform_points(x, y, dst_crs, src_crs)
    inv = warp.invert_geotransform(src_gt)
    u, v = inv[0] + x * inv[1] + y * inv[2], inv[3] + x * inv[4] + y * inv[5]
    bad = ~(np.isfinite(u) & np.isfinite(v))
    if src_shape is not None:
        with np.errstate(invalid="ignore"):
            bad |= ~((u >= 0) & (u < src_shape[1]) & (v >= 0) & (v < src_shape[0]))
    return np.stack([np.where(bad, np.nan, u), np.where(bad, np.nan, v)])


def near_boundary(uv, eps=1e-6):
    """pixels whose (u, v) lies within eps of a cell boundary (an integer) -- or of the raster's edge, which is one"""
    with np.errstate(invalid="ignore"):
        d = np.abs(uv - np.round(uv))
    return np.nan_to_num(d, nan=1.0).min(axis=0) < eps


def nearest_ref(planes, uv, nodata):
    """planes (P, Hs, Ws) any dtype, uv from source_coords_ref with src_shape -> (P, H, W): planes[p][floor(v), floor(u)], nodata[p] outside"""
    planes = np.asarray(planes)
    inside = np.isfinite(uv[0])
    col = np.where(inside, np.floor(np.nan_to_num(uv[0])), 0).astype(np.int64)
    row = np.where(inside, np.floor(np.nan_to_num(uv[1])), 0).astype(np.int64)
    out = np.empty((planes.shape[0],) + uv.shape[1:], dtype=planes.dtype)
    for p in range(planes.shape[0]):
        out[p] = np.where(inside, planes[p][row, col], np.array(nodata[p], dtype=planes.dtype))
    return out


def _counts(a, nodata):
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (bits != np.array(nodata, dtype=np.float32).view(np.uint32)) & ~np.isnan(a)


def bilinear_ref(plane, uv, nodata):
    """float32 plane (Hs, Ws) -> float64 (H, W) BEFORE the rounding to float32, and the valid mask: the four pixels around
    (u - 0.5, v - 0.5), weights (1 - fx | fx)(1 - fy | fy), samples outside the raster / NaN / nodata (bits) / of weight 0 left
    out, divided by the weight of the rest; not valid where (u, v) is outside or the nearest pixel does not count"""
    Hs, Ws = plane.shape
    cnt = _counts(plane, nodata)
    inside = np.isfinite(uv[0])
    u, v = np.nan_to_num(uv[0]), np.nan_to_num(uv[1])
    valid = inside & cnt[np.floor(v).astype(np.int64).clip(0, Hs - 1), np.floor(u).astype(np.int64).clip(0, Ws - 1)]
    x0, y0 = np.floor(u - 0.5), np.floor(v - 0.5)
    fx, fy = u - 0.5 - x0, v - 0.5 - y0
    acc, wsum = np.zeros(u.shape), np.zeros(u.shape)
    for k in range(4):
        xx, yy = (x0 + (k & 1)).astype(np.int64), (y0 + (k >> 1)).astype(np.int64)
        w = (fx if k & 1 else 1.0 - fx) * (fy if k >> 1 else 1.0 - fy)
        ok = (w > 0) & (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
        xs, ys = xx.clip(0, Ws - 1), yy.clip(0, Hs - 1)
        ok &= cnt[ys, xs]
        acc += np.where(ok, w * np.where(ok, plane[ys, xs], 0).astype(np.float64), 0.0)
        wsum += np.where(ok, w, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = acc / wsum
    return np.where(valid, val, np.nan), valid


def mismatching_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return int((a.view(np.uint8) != b.view(np.uint8)).sum())
