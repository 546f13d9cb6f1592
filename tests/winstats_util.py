"""CPU oracle and seeded scenes of the mag1c window statistics (starcop_amd.sampling.window_stats / sc_window_stats).

``oracle_rows`` is the reference loop (scripts/preprocessing/stats_mag1c.py:41-63) on a numpy array: the same masking, the same
clip, and the same numpy functions (np.max, np.min, np.percentile(x, 1 / 5 / 95 / 99), np.median) called on the float32 values.
``sum`` / ``mean`` are the float64 ones the kernel reports (``sum64`` / ``mean64``); numpy's float32 pairwise results, which the
reference stores, are kept next to them (``sum32`` / ``mean32``) for the bound below.

What numpy computes for a percentile of float32 data, found by probing numpy 2.2 over 12 000 random (count, q) and read off
``numpy/lib/_function_base_impl.py``: the quantile is ``q / float32(100)`` (float32), the virtual index ``(n - 1) * quantile`` is
float32, the weight is its fractional part (float32), and ``_lerp`` -- ``a + (b - a) * t``, replaced by ``b - (b - a) * (1 - t)``
where ``t >= 0.5`` -- runs in float32 throughout.  "fp64 lerp, rounded once" (what ``k_percentile_bounds`` of features.hip does
for its trim bounds) differs from that in about 10 % of the cases, so the kernel reproduces the float32 arithmetic and the gate
stays bit equality.  The median is ``np.mean`` of the two middle order statistics: ``(a + b) / 2`` in float32.
-0.0 passes ``v >= 0`` and is an equal key to +0.0, so which of the two a partition leaves at a rank is unspecified in numpy as
well: results are compared as bit patterns after ``+ 0.0`` (``bits``), which only maps -0.0 to +0.0.
"""
import math

import numpy as np

# The bit-equality gates of the percentile columns hold against numpy >= 2.0 only: since NEP 50 a Python q divided by
# float32(100) stays float32, so the virtual index, the weight and the lerp are float32 operations, which is what the kernel
# reproduces.  numpy 1.x promoted them to float64 and gives other last bits: that would be a difference of oracles, not a kernel fault.
assert int(np.__version__.split(".")[0]) >= 2, \
    f"tests/winstats_util.py needs numpy >= 2.0 (found {np.__version__}): numpy 1.x interpolates float32 percentiles in float64"

COLUMNS = ["window_col_off", "window_row_off", "window_width", "window_height", "max", "min", "mean", "percentile01",
           "percentile05", "median", "percentile95", "percentile99", "sum", "count"]
F32_COLUMNS = ["max", "min", "percentile01", "percentile05", "median", "percentile95", "percentile99"]


def create_windows(shape, window_size, overlap, include_incomplete=True):
    sr, sc = window_size[0] - overlap[0], window_size[1] - overlap[1]
    out = []
    for r in range(0, shape[0], sr):
        for c in range(0, shape[1], sc):
            h, w = min(window_size[0], shape[0] - r), min(window_size[1], shape[1] - c)
            if (h, w) == tuple(window_size) or include_incomplete:
                out.append((r, c, h, w))
    return out


def oracle_rows(scene, windows, fill=None, clip=10_000.):
    """list of dicts, one per non-empty window, in window order"""
    scene = np.asarray(scene, dtype=np.float32)
    rows = []
    for (r, c, h, w) in windows:
        data = scene[r:r + h, c:c + w]
        values = data[data != np.float32(fill)] if fill is not None else data.ravel()
        with np.errstate(invalid="ignore"):
            values = values[values >= 0]
        values = values.copy()
        values[values >= clip] = clip
        if values.shape[0] == 0:
            continue
        assert values.dtype == np.float32
        rows.append({"window_col_off": c, "window_row_off": r, "window_width": w, "window_height": h,
                     "max": np.max(values), "min": np.min(values), "percentile01": np.percentile(values, 1),
                     "percentile05": np.percentile(values, 5), "median": np.median(values),
                     "percentile95": np.percentile(values, 95), "percentile99": np.percentile(values, 99),
                     "sum64": math.fsum(values.astype(np.float64)), "sum32": np.sum(values), "mean32": np.mean(values),
                     "count": values.shape[0]})
        rows[-1]["mean64"] = rows[-1]["sum64"] / values.shape[0]
    return rows


def bits(v):
    """float32 bit patterns with -0.0 mapped to +0.0"""
    return (np.asarray(v, dtype=np.float32) + np.float32(0)).view(np.uint32)


def pairwise_depth(n):
    """Most float32 additions any term passes through in numpy's pairwise sum of n contiguous float32 values
    (numpy/_core/src/umath/loops_utils.h.src, PW_BLOCKSIZE = 128): a leaf of at most 128 values feeds eight accumulators
    (at most 16 terms each: 15 additions), combines them in three levels and adds at most 7 left-over terms one by one
    (15 + 3 + 7 = 25); above 128 the range is halved (the lower half rounded down to a multiple of 8, so the halves are at most
    n/2 + 8 long and the recursion is at most ceil(log2(n / 128)) + 1 deep), one addition per level."""
    return 25 + (0 if n <= 128 else math.ceil(math.log2(n / 128)) + 1)


def sum_bounds(count):
    """(relative bound of the fp64 sum against the exact one, relative bound of numpy's float32 pairwise sum against it).
    All terms are non-negative, so a summation in which every term passes through at most d additions of unit roundoff u is
    within (1 + u)^d - 1 of the exact sum, relatively, in any order: d = count - 1, u = 2^-53 for the kernel (first order, as
    the issue states it), d = pairwise_depth, u = 2^-24 for numpy."""
    return max(count - 1, 0) * 2.0 ** -53, (1 + 2.0 ** -24) ** pairwise_depth(count) - 1


def ragged_scene():
    """701 x 333: continuous positive / negative values, a -9999 wedge, NaN, negative, -0.0, +inf and >= 10 000 pixels; with
    windows 128 / overlap 64 (stride 64, incomplete edge windows): window (0, 0) is entirely nodata, (128, 128) has a single
    valid pixel, (256, 128) has two, (384, 0) is dominated by ties (thousands of exact 0.0 and of exact 10 000)."""
    rng = np.random.default_rng(701333)
    H, W = 701, 333
    s = (rng.standard_normal((H, W)) * 900 + 400).astype(np.float32)
    s[rng.random((H, W)) < .01] = np.nan
    s[rng.random((H, W)) < .01] = -0.0
    s[rng.random((H, W)) < .005] = np.inf
    s[rng.random((H, W)) < .01] = 10_000.
    s[rng.random((H, W)) < .01] = 23_456.5
    rr, cc = np.mgrid[:H, :W]
    s[cc > 250 + rr // 8] = -9999.                     # wedge
    s[0:128, 0:128] = -9999.                           # window (0, 0): nothing valid
    s[128:256, 128:256] = -9999.
    s[200, 200] = 321.5                                # window (128, 128): one valid pixel
    s[256:384, 128:256] = np.nan
    s[300, 150], s[383, 255] = 7.25, 12_000.           # window (256, 128): two valid pixels, one above the clip
    t = rng.random((128, 128))
    blk = np.where(t < .45, 0.0, np.where(t < .9, 10_000., rng.random((128, 128)) * 9000)).astype(np.float32)
    s[384:512, 0:128] = blk                            # window (384, 0): ties
    return s, create_windows((H, W), (128, 128), (64, 64)), -9999.


def flightline_scene(H=4096, W=668, seed=4096668):
    """A mag1c-like flight line: heavy-tailed background around zero (half of it negative), a planted plume, a slanted nodata
    border of -9999 on both sides, a few saturated pixels."""
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((H, W)) * 350).astype(np.float32)
    s += (rng.standard_exponential((H, W)) * 60).astype(np.float32)
    rr, cc = np.mgrid[:H, :W]
    s += (4000 * np.exp(-(((rr - H * .4) / 90.) ** 2 + ((cc - 300) / 40.) ** 2))).astype(np.float32)
    s[rng.random((H, W)) < .0005] = 15_000.
    left = 30 + (rr * 40) // H
    s[(cc < left) | (cc >= W - 70 + left)] = -9999.
    return s


def windows_flightline(shape):
    return create_windows(shape, (512, 512), (256, 256))
