"""CPU oracle of the plume label mask (starcop/data/mask_creation.py:6-27, proposed_mask) restated with scipy.ndimage, and the
seeded plume fields the label tests use.  scikit-image (what the reference calls) is not a dependency here: its
binary_erosion / binary_dilation are scipy's with border_value=1 / 0, and measure.label's default for 2-D images is
8-connectivity, i.e. scipy's label with a 3 x 3 block of ones.  numpy + scipy only."""
import numpy as np

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)      # skimage.morphology.disk(1)
EIGHT = np.ones((3, 3), dtype=bool)


def dilated_opening(t):
    """dilation(opening(t, disk(1)), disk(1)) with skimage's borders (erosion: outside set, dilations: outside unset)"""
    from scipy import ndimage
    e = ndimage.binary_erosion(t, CROSS, border_value=1)
    o = ndimage.binary_dilation(e, CROSS, border_value=0)
    return ndimage.binary_dilation(o, CROSS, border_value=0)


def proposed_mask(label_rgba_values, mag1c_values, threshold=200.0):
    """(C, H, W) label_rgba and (Cm, H, W) mag1c -> (H, W) bool, the reference's steps one by one"""
    from scipy import ndimage
    existing = np.asarray(label_rgba_values)[-1] != 0
    with np.errstate(invalid="ignore"):
        t = np.asarray(mag1c_values)[0] >= threshold              # NaN >= 200 is False
    d = dilated_opening(t)
    lab, _ = ndimage.label(d, structure=EIGHT)
    hit = np.unique(lab[existing & (lab != 0)])
    return np.isin(lab, hit) & (lab != 0) & t


def plume_field(rng, H, W, blobs=6, nan_frac=0.002, exact=True):
    """(mag1c (1, H, W) float32, label_rgba (4, H, W) uint8): Gaussian plumes plus noise around the 200 threshold, some pixels
    exactly 200, some NaN; alpha inside some plumes, on the background and across components."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    mag = rng.normal(60, 90, (H, W)).astype(np.float32)
    centres = []
    for _ in range(blobs):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        sy, sx = rng.uniform(2, max(3, H / 10)), rng.uniform(2, max(3, W / 10))
        mag += rng.uniform(300, 1500) * np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)).astype(np.float32)
        centres.append((int(cy), int(cx)))
    if exact:
        sel = rng.uniform(size=(H, W)) < 0.02
        mag[sel] = 200.0
    mag[rng.uniform(size=(H, W)) < nan_frac] = np.nan
    alpha = np.zeros((H, W), np.uint8)
    for k, (cy, cx) in enumerate(centres):
        if k % 2 == 0:                                          # a labelled box around every other plume
            alpha[max(0, cy - 3):cy + 3, max(0, cx - 3):cx + 3] = 255
    for _ in range(3):                                          # stray labels on the background and long strokes across
        y, x = rng.integers(0, H), rng.integers(0, W)
        alpha[y, max(0, x - W // 4):x + W // 4] = 128
    alpha[rng.uniform(size=(H, W)) < 0.001] = 7
    rgba = np.zeros((4, H, W), np.uint8)
    rgba[0] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    rgba[3] = alpha
    return mag[None], rgba
