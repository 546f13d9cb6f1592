"""Oracles and the seeded case table of the morphology tests (test_morphology_host.py, test_gpu_morphology.py).  numpy / scipy
only: nothing here touches the device or the library."""
import numpy as np
from scipy import ndimage

FAR = 2 ** 31 - 1
BRUTE_MAX_PIXELS = 64 * 130


def d2_brute(targets):
    """all pixels x all targets in int64 -> int64 (H, W) squared distances; FAR everywhere without a target"""
    targets = np.asarray(targets, dtype=bool)
    H, W = targets.shape
    ty, tx = np.nonzero(targets)
    if ty.size == 0:
        return np.full((H, W), FAR, dtype=np.int64)
    py, px = np.mgrid[0:H, 0:W]
    py, px = py.reshape(-1, 1).astype(np.int64), px.reshape(-1, 1).astype(np.int64)
    out = np.empty(H * W, dtype=np.int64)
    step = max(1, (1 << 22) // max(ty.size, 1))
    for s in range(0, H * W, step):
        out[s:s + step] = ((py[s:s + step] - ty[None, :]) ** 2 + (px[s:s + step] - tx[None, :]) ** 2).min(1)
    return out.reshape(H, W)


def d2_scipy(targets):
    """np.rint(distance_transform_edt(~targets) ** 2) as int64; by the definition (all FAR) without a target, where scipy's
    result is arbitrary"""
    targets = np.asarray(targets, dtype=bool)
    if not targets.any():
        return np.full(targets.shape, FAR, dtype=np.int64)
    return np.rint(ndimage.distance_transform_edt(~targets) ** 2).astype(np.int64)


def d2_oracle(targets):
    targets = np.asarray(targets, dtype=bool)
    return d2_brute(targets) if targets.size <= BRUTE_MAX_PIXELS else d2_scipy(targets)


def capped(d2, cap):
    """values above the cap replaced by FAR"""
    return np.where(d2 > cap, FAR, d2)


def dist_f32(d2, pixel_size=1.0):
    """the float32 distances the library must reproduce bit for bit: one rounding of the float64 product; inf where FAR"""
    with np.errstate(over="ignore"):
        d = (np.sqrt(d2.astype(np.float64)) * pixel_size).astype(np.float32)
    return np.where(d2 == FAR, np.float32(np.inf), d).astype(np.float32)


def disc(radius):
    t = int(np.floor(float(radius) * float(radius)))
    r = int(np.floor(np.sqrt(t)))
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (y * y + x * x) <= t


def dilate(m, radius):
    m = np.asarray(m) != 0
    if radius == 0:
        return m.astype(np.uint8)
    return ndimage.binary_dilation(m, disc(radius)).astype(np.uint8)


def erode(m, radius):
    m = np.asarray(m) != 0
    if radius == 0:
        return m.astype(np.uint8)
    return ndimage.binary_erosion(m, disc(radius), border_value=1).astype(np.uint8)


def sieve(m, min_area, connectivity=2):
    m = np.asarray(m) != 0
    structure = np.ones((3, 3), dtype=bool) if connectivity == 2 else ndimage.generate_binary_structure(2, 1)
    lab, n = ndimage.label(m, structure)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= max(int(min_area), 1)
    keep[0] = False
    return keep[lab].astype(np.uint8)


def bernoulli(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def case_table():
    """[(name, uint8 mask)]: the shapes and contents at which the two passes can go wrong"""
    cases = []
    shapes = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 130)] + [(9, w) for w in (63, 64, 65, 255, 256, 257)]
    for k, (H, W) in enumerate(shapes):
        cases.append((f"empty_{H}x{W}", np.zeros((H, W), dtype=np.uint8)))
        cases.append((f"full_{H}x{W}", np.ones((H, W), dtype=np.uint8)))
        for d in (0.002, 0.05, 0.5):
            cases.append((f"bern{d}_{H}x{W}", bernoulli((H, W), d, 1000 * k + int(d * 1000))))
    for H, W in ((37, 53), (64, 130)):
        row = np.zeros((H, W), dtype=np.uint8)
        row[H // 3] = 1
        col = np.zeros((H, W), dtype=np.uint8)
        col[:, W - 2] = 1
        yy, xx = np.mgrid[0:H, 0:W]
        cases += [(f"row_{H}x{W}", row), (f"col_{H}x{W}", col), (f"checker_{H}x{W}", ((yy + xx) & 1).astype(np.uint8))]
    corner = np.zeros((129, 257), dtype=np.uint8)
    corner[128, 0] = 1
    cases.append(("corner_129x257", corner))
    cases.append(("sparse_300x1100", bernoulli((300, 1100), 1e-4, 3001100)))
    return cases
