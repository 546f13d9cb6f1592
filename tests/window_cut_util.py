"""numpy restatement of the reads of the reference's WindowDataset.__getitem__ (starcop/data/sampling_dataset.py:259-303) and of
georeader.window_utils.pad_window_to_size: the oracle of tests/test_window_cut_host.py and tests/test_gpu_window_cut.py.

The reference multiplies a float32 array in place by a float64 scalar (``values *= s``).  The numpy 1.x that produced the published
dataset computes that in float32 with the scalar rounded to float32 once; it is written here as ``values * np.float32(s)`` so that
the result does not depend on the installed numpy.  Results are compared with ``equal`` (``np.array_equal(..., equal_nan=True)``):
NaN equals NaN and the sign of a zero is not part of the contract."""
import numpy as np


def pad_window(window, size):
    """(row_off, col_off, height, width) padded to size = (height, width): a dimension smaller than the target grows by
    pad = target - size, pad // 2 on the leading side, the rest on the trailing side; a large enough dimension is unchanged"""
    r, c, h, w = window
    if h < size[0]:
        pad = size[0] - h
        r, h = r - pad // 2, h + pad // 2 + (pad - pad // 2)
    if w < size[1]:
        pad = size[1] - w
        c, w = c - pad // 2, w + pad // 2 + (pad - pad // 2)
    return r, c, h, w


def read_boundless(plane, window, origin=(0, 0)):
    """``read_from_window(window, boundless=True).load(boundless=True)`` (:266) for one 2-D plane whose element (0, 0) sits at
    ``origin`` of the scene: what the plane does not hold reads as 0"""
    r, c, h, w = window
    out = np.zeros((h, w), dtype=plane.dtype)
    r0, c0 = r - origin[0], c - origin[1]
    ys, ye = max(r0, 0), min(r0 + h, plane.shape[0])
    xs, xe = max(c0, 0), min(c0 + w, plane.shape[1])
    if ye > ys and xe > xs:
        out[ys - r0:ye - r0, xs - c0:xe - c0] = plane[ys:ye, xs:xe]
    return out


def post(values, fill=None, scale=None, clip=None):
    """:269-271 (nodata -> 0), :285 / :289 (the float32 multiply), :287 / :293 (np.clip)"""
    values = values.copy()
    if fill is not None:
        with np.errstate(invalid="ignore"):
            values[values == fill] = 0
    if scale is not None:
        assert values.dtype == np.float32
        with np.errstate(invalid="ignore", over="ignore"):
            values = values * np.float32(scale)
        assert values.dtype == np.float32
    if clip is not None:
        values = np.clip(values, np.float32(clip[0]), np.float32(clip[1]))
    return values


def cut(plane, window, origin=(0, 0), fill=None, scale=None, clip=None):
    return post(read_boundless(plane, window, origin), fill, scale, clip)


def equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b)


def float_plane(rng, shape, fill=-9999.0):
    """float32 values around the clip bounds of the products (negative, 0 .. 2, large), with the fill value, NaN and +-inf"""
    a = (rng.standard_normal(shape) * 3).astype(np.float32)
    a[rng.random(shape) < .1] *= np.float32(5000)
    a[rng.random(shape) < .1] = np.float32(fill)
    a[rng.random(shape) < .05] = np.nan
    a[rng.random(shape) < .03] = np.inf
    a[rng.random(shape) < .03] = -np.inf
    a[rng.random(shape) < .03] = 0
    return a


def windows_for(scene, out):
    """(row_off, col_off) of windows of size ``out`` = (h, w) over a ``scene`` = (H, W): inside (where one fits), over each of the
    four edges, over the corners, wholly outside, every residue of col_off mod 4, negative offsets and duplicates"""
    H, W = scene
    h, w = out
    offs = [(max(0, (H - h) // 2), max(0, (W - w) // 2)),        # inside (larger than the scene on all sides where it is small)
            (-h // 2, 3), (H - h // 2, 2), (5, -w // 2), (6, W - w // 2),      # top, bottom, left, right
            (-3, -5), (H - 2, W - 3), (-h + 1, W - 1),                       # corners
            (-h, 0), (H, 1), (0, -w), (2, W), (-4 * h, -4 * w), (H + 7, W + 9)]     # wholly outside
    offs += [(1, k) for k in range(4)] + [(2, -k) for k in range(1, 5)]       # col_off mod 4
    if h > H and w > W:
        offs.append((-(h - H) // 2, -(w - W) // 2))               # larger than the scene on all sides
    offs += [offs[0], offs[1], offs[0]]                          # duplicates
    return offs
