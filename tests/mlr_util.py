"""Seeded WV3-like tiles and the float64 host oracle of the MLR ratio (starcop/data/feature_extration.py:58-109), shared by
tests/golden/make_golden_mlr.py and the MLR tests.  numpy only."""
import os

import numpy as np

QUANT = 16384          # tests/golden/g12_mlr.npz stores its tiles as uint16 counts of 1 / QUANT
DIVISIONS = ("c_matched_outliers", "simple_plus", "residual")


def load_g12(path=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_mlr.npz")):
    """tests/golden/g12_mlr.npz (see make_golden_mlr.py) unpacked: {name}_bands / _target float32, {name}_{f32,f64}_{division}
    for the three divisions and 'autoclip', {name}_{f32,f64}_coef / _intercept, names, registry_keys, registry_inputs"""
    z = np.load(path)
    g = {k: z[k] for k in ("names", "registry_keys", "registry_inputs")}
    for name in g["names"]:
        g[f"{name}_bands"] = z[f"{name}_bands_q"].astype(np.float32) / np.float32(QUANT)
        g[f"{name}_target"] = z[f"{name}_target_q"].astype(np.float32) / np.float32(QUANT)
        for tag in ("f32", "f64"):
            g[f"{name}_{tag}_coef"], g[f"{name}_{tag}_intercept"] = z[f"{name}_{tag}_coef"], z[f"{name}_{tag}_intercept"]
        for div in DIVISIONS:
            f32 = z[f"{name}_f32_{div}"]
            g[f"{name}_f32_{div}"] = f32
            g[f"{name}_f64_{div}"] = f32.astype(np.float64) + z[f"{name}_d64_{div}"].astype(np.float64)
        for tag in ("f32", "f64"):                 # the reference's autoclip=True: np.clip of the c_matched_outliers result
            g[f"{name}_{tag}_autoclip"] = np.clip(g[f"{name}_{tag}_c_matched_outliers"], -0.2, 0.2)
    return g


def wv3_tile(rng, H, W, k=5, border=6, plume=True, scale=1.0, offset=0.0):
    """(k, H, W) regressors and the (H, W) target, float32: correlated SWIR-like bands over a smooth albedo field, a nodata
    zero border and (plume=True) a plume-like absorption patch in the target only."""
    yy, xx = np.mgrid[0:H, 0:W] / max(H, W)
    alb = 0.18 + 0.08 * np.sin(6 * xx + 2 * rng.uniform()) * np.cos(4 * yy + rng.uniform()) + 0.03 * rng.standard_normal((H, W))
    gains = rng.uniform(0.6, 1.4, size=k)
    bands = np.stack([alb * gains[j] + 0.025 * rng.standard_normal((H, W)) for j in range(k)])
    w = rng.uniform(-0.3, 1.0, size=k) * 2.0 / k
    w[0] = abs(w[0]) + 0.5
    target = 0.06 + np.tensordot(w, bands, 1) * 0.5 + 0.01 * rng.standard_normal((H, W))
    target = np.maximum(target, 0.03)
    if plume:
        cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
        d2 = ((np.mgrid[0:H, 0:W][0] - cy) / (0.08 * H)) ** 2 + ((np.mgrid[0:H, 0:W][1] - cx) / (0.12 * W)) ** 2
        target = target * (1.0 - 0.08 * np.exp(-d2))
    bands, target = bands * scale + offset, target * scale + offset
    if border:
        for a in list(bands) + [target]:
            a[:border] = 0; a[-border:] = 0; a[:, :border] = 0; a[:, -border:] = 0
    return bands.astype(np.float32), target.astype(np.float32)


def fit64(bands, target):
    """least squares with intercept over all pixels in float64, as sklearn's LinearRegression solves it: centre X and t, take
    numpy's minimum-norm lstsq solution, intercept = mean(t) - mean(X) . coef -> (coef (k,), intercept)"""
    k = bands.shape[0]
    X = bands.reshape(k, -1).T.astype(np.float64)
    t = target.reshape(-1).astype(np.float64)
    xm, tm = X.mean(0), t.mean()
    coef = np.linalg.lstsq(X - xm, t - tm, rcond=None)[0]
    return coef, tm - xm.dot(coef)


def _percentile_trimmed_sum(x, p=5, f32_bounds=False):
    lo, hi = np.percentile(x, p), np.percentile(x, 100 - p)
    if f32_bounds:                 # the bounds as numpy computes them on a float32 tile (and sc_trimmed_sums stores them)
        lo, hi = np.float32(lo), np.float32(hi)
    return x[(x >= lo) & (x <= hi)].sum()


def ratio64(bands, target, division="c_matched_outliers", autoclip=False, r_f32=False):
    """ratio_MLR_local's arithmetic in float64 on the float64 least-squares prediction.  r_f32: the prediction rounded to
    float32 first, as the reference's float32 run and sc_mlr_predict store it -- the 5/95 % trim of c_matched_outliers is
    discontinuous in r (two neighbouring order statistics that tie in float32 both enter the trimmed sum), so a float32 r can
    move c by one pixel's share of the sum against the all-float64 result"""
    coef, icpt = fit64(bands, target)
    t = target.astype(np.float64)
    r = icpt + np.tensordot(coef, bands.astype(np.float64), 1)
    if r_f32:
        r = r.astype(np.float32).astype(np.float64)
    if division == "c_matched_outliers":
        c = _percentile_trimmed_sum(t.ravel(), f32_bounds=r_f32) / _percentile_trimmed_sum(r.ravel(), f32_bounds=r_f32)
        with np.errstate(invalid="ignore", divide="ignore"):
            R = (c * r - t) / (t + 1e-6)
        R[(r < 1e-6) & (t < 1e-6)] = -0.5
        R = np.where(t == 0.0, -0.5, R)
    elif division == "simple_plus":
        R0 = -t / (r + 1e-6)
        with np.errstate(invalid="ignore", divide="ignore"):
            R = (R0 - R0.mean()) / R0.std()
        R = np.where(t == 0.0, np.min(R), R)
    elif division == "residual":
        R = np.where(t == 0.0, 0.0, (t - r) / (r + 1e-6))
    else:
        raise ValueError(division)
    return np.clip(R, -0.2, 0.2) if autoclip else R
