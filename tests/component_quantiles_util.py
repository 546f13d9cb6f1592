"""numpy restatement of sc_component_quantiles / plumes.component_quantiles, written from numpy's documented behaviour.

Per row: ``t = plane[labels == k]`` (or ``np.abs(t - np.float32(c))`` with a centre), the finite ones kept, then
``np.percentile(t, q)`` one Python scalar ``q`` at a time and ``np.median(t)`` on the float32 values.  Results are compared with
``np.array_equal(got, want, equal_nan=True)``: a zero may have either sign, everything else is bit equality; there is no tolerance.
"""
import numpy as np

# The bit-equality gates hold against numpy >= 2.0 only: since NEP 50 a Python q divided by float32(100) stays float32, so the
# virtual index, the weight and the lerp are float32 operations, which is what the kernel reproduces (tests/winstats_util.py).
assert int(np.__version__.split(".")[0]) >= 2, \
    f"tests/component_quantiles_util.py needs numpy >= 2.0 (found {np.__version__}): numpy 1.x interpolates float32 percentiles in float64"


def one(values, q):
    """the order statistics ``q`` (numbers and / or "median") of a 1-D float32 array with at least one value -> float32 (Q,)"""
    assert values.dtype == np.float32 and values.ndim == 1 and values.size
    out = [np.median(values) if isinstance(v, str) else np.percentile(values, v) for v in q]
    assert all(o.dtype == np.float32 for o in out)
    return np.array(out, dtype=np.float32)


def members(labels, plane, k, c=None):
    """the finite values of component k of one (H, W) image, |v - c| with a centre"""
    t = np.asarray(plane, dtype=np.float32)[np.asarray(labels) == k]
    if c is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.abs(t - np.float32(c))
    return t[np.isfinite(t)]


def oracle(labels, counts, plane, q=("median",), center=None, M=None):
    """(N, H, W) labels, (N,) counts, (N, H, W) float32 plane, optional (N, M) centres -> n_finite (N, M) int64, quantile
    (N, M, Q) float32; rows at or above min(counts[n], M) and rows without a member are 0 and NaN"""
    labels, plane = np.asarray(labels), np.asarray(plane, dtype=np.float32)
    if labels.ndim == 2:
        labels, plane = labels[None], plane[None]
    counts = np.asarray(counts).reshape(-1)
    N = labels.shape[0]
    M = max(int(counts.max()), 0) if M is None else int(M)
    nf = np.zeros((N, M), np.int64)
    qs = np.full((N, M, len(q)), np.nan, np.float32)
    for n in range(N):
        for k in range(1, min(max(int(counts[n]), 0), M) + 1):
            t = members(labels[n], plane[n], k, None if center is None else np.asarray(center)[n, k - 1])
            nf[n, k - 1] = t.size
            if t.size:
                qs[n, k - 1] = one(t, q)
    return nf, qs


def median_mad(labels, counts, plane, M=None):
    """-> n_finite, median, mad (N, M): np.median(v) and np.median(|v - median|) over the finite values of each component"""
    nf, med = oracle(labels, counts, plane, ("median",), M=M)
    _, mad = oracle(labels, counts, plane, ("median",), center=med[..., 0], M=M)
    return nf, med[..., 0], mad[..., 0]


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
