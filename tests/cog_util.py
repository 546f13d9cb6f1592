"""numpy restatements of the Cloud-Optimized GeoTIFF kernels (sc_overview_reduce, sc_tiff_pack_tiles, sc_tiff_tile_flags) and the
seeded images of their tests.  Everything works on bit patterns: a float32 image is compared through its uint32 view."""
import zlib

import numpy as np

NAN_BITS = np.uint32(0x7FC00000)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def nodata_bits(nodata, dtype):
    if nodata is None:
        return None
    return np.float32(nodata).view(np.uint32) if np.dtype(dtype) == np.float32 else np.uint8(nodata)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def reduce_level(a, resampling, nodata=None):
    """one level of the pyramid: (nb, h, w) float32 / uint8 -> (nb, ceil(h / 2), ceil(w / 2)).  Output (r, c) is made from the
    source pixels (2r + i, 2c + j) inside the image, in the order (0,0), (0,1), (1,0), (1,1); a sample is valid unless it is NaN
    or has the nodata bits."""
    a = np.ascontiguousarray(a)
    nb, h, w = a.shape
    h2, w2 = -(-h // 2), -(-w // 2)
    b = np.zeros((nb, 2 * h2, 2 * w2), dtype=bits(a).dtype)
    b[:, :h, :w] = bits(a)
    inside = np.zeros((nb, 2 * h2, 2 * w2), dtype=bool)
    inside[:, :h, :w] = True
    v = [b[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    ok = [inside[:, i::2, j::2].copy() for i in (0, 1) for j in (0, 1)]
    if resampling == "nearest":
        return v[0].copy().view(a.dtype)
    nd = nodata_bits(nodata, a.dtype)
    for k in range(4):
        if a.dtype == np.float32:
            ok[k] &= (v[k] & np.uint32(0x7FFFFFFF)) <= np.uint32(0x7F800000)
        if nd is not None:
            ok[k] &= v[k] != nd
    if a.dtype == np.float32:
        assert resampling == "average"
        s = np.zeros(v[0].shape, dtype=np.float64)
        n = np.zeros(v[0].shape, dtype=np.int64)
        with np.errstate(all="ignore"):
            for k in range(4):
                x = v[k].view(np.float32).astype(np.float64)
                s = np.where(ok[k], np.where(n == 0, x, s + x), s)
                n += ok[k]
            q = (s / np.maximum(n, 1)).astype(np.float32).view(np.uint32)
        none = nd if nd is not None else NAN_BITS
        return np.where(n > 0, q, none).astype(np.uint32).view(np.float32)
    none = nd if nd is not None else np.uint8(0)
    if resampling == "average":
        s = sum(np.where(ok[k], v[k], 0).astype(np.int64) for k in range(4))
        n = sum(ok[k].astype(np.int64) for k in range(4))
        return np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), none).astype(np.uint8)
    assert resampling == "mode"
    best_n = np.zeros(v[0].shape, dtype=np.int64)
    best_v = np.full(v[0].shape, none, dtype=np.int64)
    for k in range(4):
        n = sum((ok[j] & (v[j] == v[k])).astype(np.int64) for j in range(4))
        take = ok[k] & ((n > best_n) | ((n == best_n) & (v[k] < best_v)))
        best_n = np.where(take, n, best_n)
        best_v = np.where(take, v[k], best_v)
    return best_v.astype(np.uint8)


def pyramid(a, levels, resampling, nodata=None):
    out = []
    for _ in range(levels):
        a = reduce_level(a, resampling, nodata)
        out.append(a)
    return out


def predict_rows(t, predictor, nb):
    """t: (rows, cols, nb) little-endian samples of a tile -> the (rows, row bytes) uint8 bytes after the TIFF predictor"""
    rows = t.shape[0]
    raw = np.ascontiguousarray(t).view(np.uint8).reshape(rows, -1)
    if predictor == 1:
        return raw
    if predictor == 2:
        assert t.dtype == np.uint8
        out = raw.copy()
        out[:, nb:] = raw[:, nb:] - raw[:, :-nb]
        return out
    assert predictor == 3 and t.dtype == np.float32
    by_sample = raw.reshape(rows, -1, 4)                                   # [row][sample][byte], little-endian
    planes = np.ascontiguousarray(by_sample[:, :, ::-1].transpose(0, 2, 1)).reshape(rows, -1)     # most significant bytes first
    out = planes.copy()
    out[:, nb:] = planes[:, nb:] - planes[:, :-nb]
    return out


def pack_tiles(a, bs, predictor=1):
    """(nb, h, w) -> the TIFF tile bytes of every bs x bs tile, row-major: [bs][bs][nb] chunky samples, zero beyond the edge"""
    a = np.ascontiguousarray(a)
    nb, h, w = a.shape
    px = np.ascontiguousarray(np.moveaxis(a, 0, 2)).astype(a.dtype.newbyteorder("<"))
    out = []
    for by in range(-(-h // bs)):
        for bx in range(-(-w // bs)):
            t = np.zeros((bs, bs, nb), dtype=a.dtype)
            part = px[by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs]
            t[:part.shape[0], :part.shape[1]] = part
            out.append(predict_rows(t, predictor, nb).tobytes())
    return out


def tile_flags(a, bs, nodata=None):
    """1 per tile whose in-image samples all have the bits of the fill value (nodata, else 0)"""
    a = np.ascontiguousarray(a)
    nb, h, w = a.shape
    fill = nodata_bits(nodata, a.dtype)
    fill = bits(np.zeros(1, a.dtype))[0] if fill is None else fill
    same = bits(a) == fill
    return np.array([same[:, by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs].all()
                     for by in range(-(-h // bs)) for bx in range(-(-w // bs))], dtype=np.uint8)


def payloads(a, bs, predictor=1, absent=(), compress=True):
    """tiles of a level for io_formats.write_tiff_levels: deflated bytes, None for the tile indices in ``absent``"""
    return [None if i in absent else (zlib.compress(t, 6) if compress else t) for i, t in enumerate(pack_tiles(a, bs, predictor))]


def float_image(nb, h, w, seed, nodata=0.0):
    """seeded float32 (nb, h, w): magnitudes from 1e-3 to 1e6 with both signs, NaNs, -0.0 and +0.0, and a grid of 2 x 2 blocks that
    hold 0, 1, 2, 3 and 4 samples of ``nodata`` (so 4 .. 0 valid ones), some of them NaN instead"""
    rng = np.random.default_rng(seed)
    a = (10.0 ** rng.uniform(-3, 6, size=(nb, h, w)) * rng.choice([-1.0, 1.0], size=(nb, h, w))).astype(np.float32)
    a[rng.random((nb, h, w)) < 0.04] = np.nan
    a[rng.random((nb, h, w)) < 0.04] = np.float32(-0.0)
    a[rng.random((nb, h, w)) < 0.04] = np.float32(0.0)
    nd = np.float32(0.0 if nodata is None else nodata)
    for r in range(0, h - 1, 2):
        for c in range(0, w - 1, 2):
            k = ((r // 2) * 7 + c // 2) % 10                 # 0..4: that many fill samples; 5..9: leave the block alone
            if k <= 4:
                cells = [(0, 0), (0, 1), (1, 0), (1, 1)]
                for i, j in [cells[(t + r + c) % 4] for t in range(k)]:
                    a[:, r + i, c + j] = np.nan if (r + c) % 8 == 0 and nodata is None else nd
    return a


def byte_image(nb, h, w, seed, values=4):
    """seeded uint8 (nb, h, w) of few values: most 2 x 2 blocks hold mode ties"""
    return np.random.default_rng(seed).integers(0, values, size=(nb, h, w)).astype(np.uint8)
