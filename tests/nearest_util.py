"""Oracles of the feature-transform tests (test_nearest_host.py, test_gpu_nearest.py).  numpy / scipy only: nothing here touches
the device or the library.

The rule: nearest(p) is the target minimising the squared distance; among equally near targets the smallest column, then the
smallest row -- the arg-min of the int64 key d2 * (H * W) + col * H + row."""
import numpy as np

FAR = 2 ** 31 - 1


def nearest_brute(targets):
    """all pixels x all targets -> (index int64 (H, W): row_t * W + col_t of the arg-min of the key, d2 int64 (H, W)); -1 / FAR
    everywhere without a target.  A target is its own nearest target (d2 = 0 is a unique minimum), so only the other pixels are
    compared with every target, chunked like ``morphology_util.d2_brute``."""
    targets = np.asarray(targets, dtype=bool)
    H, W = targets.shape
    ty, tx = (v.astype(np.int64) for v in np.nonzero(targets))
    if ty.size == 0:
        return np.full((H, W), -1, dtype=np.int64), np.full((H, W), FAR, dtype=np.int64)
    index = np.arange(H * W, dtype=np.int64)
    d2 = np.zeros(H * W, dtype=np.int64)
    py, px = (v.astype(np.int64) for v in np.nonzero(~targets))
    tie = tx * H + ty
    step = max(1, (1 << 22) // ty.size)
    for s in range(0, py.size, step):
        y, x = py[s:s + step, None], px[s:s + step, None]
        d = (y - ty[None, :]) ** 2 + (x - tx[None, :]) ** 2
        k = (d * (H * W) + tie[None, :]).argmin(1)
        at = y[:, 0] * W + x[:, 0]
        index[at] = ty[k] * W + tx[k]
        d2[at] = d[np.arange(k.size), k]
    return index.reshape(H, W), d2.reshape(H, W)


def capped(index, d2, cap):
    """(index, d2) under a cap on the squared distance: -1 / FAR wherever d2 > cap"""
    far = d2 > cap
    return np.where(far, -1, index), np.where(far, FAR, d2)


def expand_labels_ref(labels, distance):
    """skimage's expand_labels with the tie rule above: background within floor(distance^2) takes the nearest pixel's label"""
    labels = np.asarray(labels)
    out = labels.astype(np.int32)
    index, d2 = nearest_brute(labels != 0)
    sel = (labels == 0) & (index >= 0) & (d2 <= int(np.floor(float(distance) ** 2)))
    out[sel] = labels.reshape(-1)[index[sel]]
    return out


def fill_nearest_ref(data, invalid, max_distance=None):
    """float32 (H, W): invalid pixels take the BITS of the nearest valid pixel; beyond the cap, or without one, they keep theirs"""
    bits = np.ascontiguousarray(data, dtype=np.float32).view(np.uint32)
    index, d2 = nearest_brute(np.asarray(invalid) == 0)
    sel = index >= 0
    if max_distance is not None:
        sel &= d2 <= int(np.floor(float(max_distance) ** 2))
    out = bits.copy()
    out[sel] = bits.reshape(-1)[index[sel]]
    return out.view(np.float32)


def rings_ref(labels, ring_px, gap_px=0.0):
    """background_rings: unlabelled pixels with floor(gap^2) < d2 <= floor(ring^2) carry the label of their nearest labelled pixel"""
    labels = np.asarray(labels)
    index, d2 = nearest_brute(labels != 0)
    sel = (labels == 0) & (index >= 0) & (d2 > int(np.floor(float(gap_px) ** 2))) & (d2 <= int(np.floor(float(ring_px) ** 2)))
    out = np.zeros(labels.shape, dtype=np.int32)
    out[sel] = labels.reshape(-1)[index[sel]]
    return out


def tie_cases():
    """[(name, uint8 mask)]: contents where most pixels have several equally near targets"""
    yy, xx = np.mgrid[0:37, 0:53]
    lattice = ((yy % 4 == 0) & (xx % 6 == 0)).astype(np.uint8)
    rows = np.zeros((64, 130), dtype=np.uint8)
    rows[20] = rows[30] = 1                                   # every pixel of row 25 ties up against down
    cols = np.zeros((9, 257), dtype=np.uint8)
    cols[:, 100] = cols[:, 140] = 1                           # every pixel of column 120 ties left against right
    return [("lattice_37x53", lattice), ("tworows_64x130", rows), ("twocols_9x257", cols)]


def four_symmetric():
    """four targets placed symmetrically about the centre of a 5 x 5 image, and the result written out by hand:
    A = (0, 2) -> 2, B = (2, 0) -> 10, C = (2, 4) -> 14, D = (4, 2) -> 22; B has the smallest column, then A and D (A the smaller
    row), then C"""
    m = np.zeros((5, 5), dtype=np.uint8)
    m[0, 2] = m[2, 0] = m[2, 4] = m[4, 2] = 1
    index = np.array([[10, 2, 2, 2, 2],
                      [10, 10, 2, 2, 14],
                      [10, 10, 10, 14, 14],
                      [10, 10, 22, 22, 14],
                      [10, 22, 22, 22, 22]], dtype=np.int64)
    d2 = np.array([[4, 1, 0, 1, 4],
                   [1, 2, 1, 2, 1],
                   [0, 1, 4, 1, 0],
                   [1, 2, 1, 2, 1],
                   [4, 1, 0, 1, 4]], dtype=np.int64)
    return m, index, d2
