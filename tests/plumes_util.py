"""CPU oracle of sc_component_stats / starcop_amd.plumes (numpy + scipy.ndimage only) and the masks the plume tests share."""
import math

import numpy as np

COMPONENT_FIELDS = ("area", "row_min", "row_max", "col_min", "col_max", "sum_row", "sum_col", "first_pixel", "n_other")
PLANE_FIELDS = ("n_finite", "sum", "max", "min", "argmax")
EIGHT = np.ones((3, 3), dtype=bool)


def scipy_label(mask, connectivity):
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=EIGHT if connectivity == 2 else None)
    return lab.astype(np.int32), int(n)


def oracle_stats(labels, count, planes=(), other=None):
    """labels (H, W) int, components 1..count (values outside [0, count] are ignored) -> dict of arrays with ``count`` rows:
    the columns of sc_component_stats, plus ``sum_abs`` (count, P): fsum of |x| over the finite values, for the sum tolerance"""
    from scipy import ndimage
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    lab = np.where((lab < 0) | (lab > count), 0, lab)
    P = len(planes)
    out = {f: np.zeros(count, dtype=np.int64) for f in COMPONENT_FIELDS}
    out.update(n_finite=np.zeros((count, P), np.int64), sum=np.zeros((count, P), np.float64), sum_abs=np.zeros((count, P), np.float64),
               max=np.full((count, P), np.nan, np.float32), min=np.full((count, P), np.nan, np.float32),
               argmax=np.full((count, P), -1, np.int64))
    if count == 0:
        return out
    index = np.arange(1, count + 1)
    rows, cols = np.indices((H, W))
    out["area"] = np.rint(ndimage.sum_labels(np.ones((H, W)), lab, index)).astype(np.int64)
    out["sum_row"] = np.rint(ndimage.sum_labels(rows.astype(np.float64), lab, index)).astype(np.int64)     # < 2^53: exact
    out["sum_col"] = np.rint(ndimage.sum_labels(cols.astype(np.float64), lab, index)).astype(np.int64)
    if other is not None:
        out["n_other"] = np.rint(ndimage.sum_labels((np.asarray(other) != 0).astype(np.float64), lab, index)).astype(np.int64)
    raster = rows * W + cols
    for k, sl in enumerate(ndimage.find_objects(lab, max_label=count)):
        if sl is None:
            out["first_pixel"][k] = -1
            continue
        out["row_min"][k], out["row_max"][k] = sl[0].start, sl[0].stop - 1
        out["col_min"][k], out["col_max"][k] = sl[1].start, sl[1].stop - 1
        inside = lab[sl] == k + 1
        idx = raster[sl][inside]                      # ascending raster order
        out["first_pixel"][k] = idx[0]
        for q, plane in enumerate(planes):
            v = np.asarray(plane, dtype=np.float32)[sl][inside]
            fin = np.isfinite(v)
            v, vi = v[fin], idx[fin]
            out["n_finite"][k, q] = v.size
            if v.size:
                out["sum"][k, q] = math.fsum(float(x) for x in v)
                out["sum_abs"][k, q] = math.fsum(abs(float(x)) for x in v)
                out["max"][k, q], out["min"][k, q] = v.max(), v.min()
                out["argmax"][k, q] = vi[np.flatnonzero(v == v.max())[0]]
    return out


def oracle_table(mask, connectivity=2, mag1c=None, prob=None, label_mask=None, min_area=1, geotransform=None, pixel_area_m2=None):
    """the columns of plumes.plume_table for one (H, W) mask as a dict of numpy arrays (item = 0); under ``"_tol"`` the absolute
    tolerance of every column that derives from an fp64 sum: area * 2^-50 * sum|x| on the sum (8 x the first-order bound of a
    float64 summation in any order), carried through the division / product plus one rounding of the result"""
    lab, n = scipy_label(np.asarray(mask) != 0, connectivity)
    planes = [p for p in (mag1c, prob) if p is not None]
    st = oracle_stats(lab, n, planes, label_mask)
    keep = st["area"] >= max(min_area, 1)
    W = lab.shape[1]
    t = {"item": np.zeros(int(keep.sum()), np.int64), "plume_id": np.arange(1, n + 1)[keep], "area_px": st["area"][keep]}
    for f in ("row_min", "row_max", "col_min", "col_max"):
        t[f] = st[f][keep]
    t["centroid_row"] = st["sum_row"][keep] / st["area"][keep]
    t["centroid_col"] = st["sum_col"][keep] / st["area"][keep]
    q = 0
    tol = {}
    sum_tol = st["area"][keep, None] * 2.0 ** -50 * st["sum_abs"][keep]

    def mean_of(q):
        nf = st["n_finite"][keep, q]
        m = np.where(nf > 0, st["sum"][keep, q] / np.maximum(nf, 1), np.nan)
        return m, sum_tol[:, q] / np.maximum(nf, 1) + 2.0 ** -52 * np.abs(np.nan_to_num(m))
    if mag1c is not None:
        am = st["argmax"][keep, q]
        t["mag1c_sum"], tol["mag1c_sum"] = st["sum"][keep, q], sum_tol[:, q]
        t["mag1c_mean"], tol["mag1c_mean"] = mean_of(q)
        t["mag1c_max"] = st["max"][keep, q].astype(np.float64)
        t["mag1c_max_row"], t["mag1c_max_col"] = np.where(am >= 0, am // W, -1), np.where(am >= 0, am % W, -1)
        if pixel_area_m2 is not None:
            t["ime_ppmm_m2"] = t["mag1c_sum"] * pixel_area_m2
            tol["ime_ppmm_m2"] = sum_tol[:, q] * pixel_area_m2 + 2.0 ** -52 * np.abs(t["ime_ppmm_m2"])
        q += 1
    if prob is not None:
        t["prob_mean"], tol["prob_mean"] = mean_of(q)
        t["prob_max"] = st["max"][keep, q].astype(np.float64)
    if label_mask is not None:
        t["overlap_px"] = st["n_other"][keep]
    if geotransform is not None:
        gt = geotransform
        t["x"] = gt[0] + (t["centroid_col"] + 0.5) * gt[1]
        t["y"] = gt[3] + (t["centroid_row"] + 0.5) * gt[5]
    t["_tol"] = tol
    return t


def assert_table(table, want):
    """DataFrame == oracle_table dict: same columns in the same order, every column equal except those that derive from an fp64
    sum, which lie within the oracle's tolerance"""
    want = dict(want)
    tol = want.pop("_tol")
    assert list(table.columns) == list(want), (list(table.columns), list(want))
    assert len(table) == len(want["item"]), (len(table), len(want["item"]))
    for c, w in want.items():
        got = table[c].to_numpy()
        if c in tol:
            assert np.array_equal(np.isnan(got), np.isnan(w)), c
            ok = ~np.isnan(w)
            assert (np.abs(got[ok] - w[ok]) <= tol[c][ok]).all(), (c, got, w, tol[c])
        else:
            assert np.array_equal(got, w, equal_nan=got.dtype.kind == "f"), (c, got, w)


def spiral(n):
    """one-pixel-wide square spiral that fills an n x n image, walls one pixel apart"""
    m = np.zeros((n, n), dtype=bool)
    r = c = 0
    dr, dc = 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        nr, nc = r + dr, c + dc
        ahead2 = (nr + dr, nc + dc)
        blocked = not (0 <= nr < n and 0 <= nc < n) or m[nr, nc] or \
            (0 <= ahead2[0] < n and 0 <= ahead2[1] < n and m[ahead2])
        if blocked:
            dr, dc = dc, -dr
            turns += 1
            continue
        r, c, turns = nr, nc, 0
        m[r, c] = True
    return m


def diagonal_stripes(H, W, period=4):
    """one-pixel anti-diagonal lines every ``period`` pixels: under connectivity 2 each is one component, boxes overlap heavily"""
    return (np.add.outer(np.arange(H), np.arange(W)) % period) == 0
