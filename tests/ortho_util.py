"""numpy oracle of the GLT orthorectification (what the note at starcop/models/mag1c_emit.py:206-221 and
``EMITImage.georreference`` compute) and the seeded look-up tables / sources the ortho tests and tools/bench_glt_ortho.py share."""
import numpy as np


def oracle(src, gx, gy, fill, absolute=False):
    """src: (rows, cols) -> (H_o, W_o) of the GLT"""
    valid = (gx != 0) & (gy != 0)
    out = np.full(gx.shape, fill, dtype=src.dtype)
    if absolute:
        out[valid] = src[np.abs(gy[valid]) - 1, np.abs(gx[valid]) - 1]
    else:
        out[valid] = src[gy[valid] - 1, gx[valid] - 1]
    return out


def oracle_planes(planes, gx, gy, fills, absolute=False, shape=None):
    """the oracle per plane, stacked; a plane smaller than the swath ``shape`` is its top-left part, the rest holds the fill value"""
    out = []
    for p, f in zip(planes, fills):
        p = np.asarray(p)
        if shape is not None and p.shape != tuple(shape):
            full = np.full(shape, f, dtype=p.dtype)
            full[:p.shape[0], :p.shape[1]] = p
            p = full
        out.append(oracle(p, gx, gy, f, absolute))
    return np.stack(out)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def mismatching_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return int((a.view(np.uint8) != b.view(np.uint8)).sum())


def random_source(rng, shape, dtype):
    """random BIT PATTERNS of the dtype: floats include NaNs with payloads, infinities, denormals and -0.0"""
    dt = np.dtype(dtype)
    raw = rng.integers(0, 256, size=tuple(shape) + (dt.itemsize,), dtype=np.uint8)
    a = raw.view(dt)[..., 0].copy()
    if dt.kind == "f" and a.size >= 2:
        a.flat[0], a.flat[1] = -0.0, np.nan
    return a


def random_glt(rng, out_shape, rows, cols, p_nodata=0.2):
    """independent random entries, about p_nodata of them no-data in both words"""
    gx = rng.integers(1, cols + 1, size=out_shape).astype(np.int32)
    gy = rng.integers(1, rows + 1, size=out_shape).astype(np.int32)
    hole = rng.random(out_shape) < p_nodata
    gx[hole] = 0
    gy[hole] = 0
    return gx, gy


def identity_glt(rows, cols):
    gy, gx = np.meshgrid(np.arange(1, rows + 1, dtype=np.int32), np.arange(1, cols + 1, dtype=np.int32), indexing="ij")
    return np.ascontiguousarray(gx), np.ascontiguousarray(gy)


def swath_glt(rows=1280, cols=1242, out_h=2000, out_w=2300, angle=0.45, scale=1.15):
    """a realistic look-up table: the rows x cols swath rotated by ``angle`` (radians) about the centre of an out_h x out_w grid
    that samples it ``scale`` times finer (nearest neighbour), so the strip lies at an angle inside a no-data border and
    neighbouring output pixels map to neighbouring or identical source pixels"""
    i, j = np.meshgrid(np.arange(out_h, dtype=np.float64), np.arange(out_w, dtype=np.float64), indexing="ij")
    y, x = (i - (out_h - 1) / 2) / scale, (j - (out_w - 1) / 2) / scale
    c, s = np.cos(angle), np.sin(angle)
    r = np.rint(c * y - s * x + (rows - 1) / 2).astype(np.int64)
    q = np.rint(s * y + c * x + (cols - 1) / 2).astype(np.int64)
    ok = (r >= 0) & (r < rows) & (q >= 0) & (q < cols)
    gx = np.where(ok, q + 1, 0).astype(np.int32)
    gy = np.where(ok, r + 1, 0).astype(np.int32)
    return gx, gy
