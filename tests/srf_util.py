"""Spectral-response-function (SRF) band simulation: synthetic SRF tables and AVIRIS band grids, and a numpy / pandas restatement
of the reference's transform_to_srf (starcop/data/aviris.py:262-331) for cases too large for the golden file g13_srf.npz."""
import os

import numpy as np
import pandas as pd

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

WV3_BANDS = ["SWIR1", "SWIR2", "SWIR3", "SWIR4", "SWIR5", "SWIR6", "SWIR7", "SWIR8"]
WV3_CENTERS = [1210, 1570, 1660, 1730, 2165, 2205, 2260, 2330]          # aviris.py:51
WV3_WIDTHS = [30, 40, 40, 40, 40, 40, 50, 70]
S2_BANDS = ["B1", "B2", "B3", "B4", "B5", "B6", "B7", "B8", "B8A", "B9", "B10", "B11", "B12"]
S2_CENTERS = [443, 490, 560, 665, 705, 740, 783, 842, 865, 945, 1375, 1610, 2190]
S2_WIDTHS = [20, 65, 35, 30, 15, 15, 20, 115, 20, 20, 30, 90, 180]


def g3_grid():
    """425 AVIRIS-NG-like band centres on a 5 nm grid: midpoints fall on x.5 nm"""
    return 377.0 + 5.0 * np.arange(425)


def emit_grid():
    """285 EMIT-like band centres with non-integer spacing"""
    return np.linspace(381.0056, 2493.2515, 285)


def _bell(wl, c, width, ripple):
    # a flat-topped response with Gaussian-like tails (rows between 1e-6 and 1e-4 among them) and a small ripple
    x = (wl - c) / (width / 2.0)
    return np.exp(-0.5 * np.abs(x) ** 3 * 4.0) * (1.0 + ripple * np.sin(wl * 0.37))


def _f32(v):
    return v.astype(np.float32).astype(np.float64)        # float64 columns, as read from a CSV, of float32-representable values


def wv3_table():
    """WV3 SWIR1..8 on 1 nm rows 1100..2450 plus rows at x.5 nm on band midpoints of g3_grid"""
    wl = np.union1d(np.arange(1100.0, 2451.0), [1209.5, 1569.5, 1734.5, 2164.5, 2329.5])
    cols = {b: _f32(_bell(wl, c, w, 0.05)) for b, c, w in zip(WV3_BANDS, WV3_CENTERS, WV3_WIDTHS)}
    return pd.DataFrame({"SR_WL": wl, **cols})


def s2_table():
    """joint S2 table: S2A_SR_AV_* and S2B_SR_AV_* (centres shifted by 1 nm) on 1 nm rows 412..2320 plus x.5 nm midpoint rows"""
    wl = np.union1d(np.arange(412.0, 2321.0), [444.5, 559.5, 864.5, 1374.5, 2189.5])
    cols = {}
    for sensor, shift in (("S2A", 0.0), ("S2B", 1.0)):
        for b, c, w in zip(S2_BANDS, S2_CENTERS, S2_WIDTHS):
            cols[f"{sensor}_SR_AV_{b}"] = _f32(_bell(wl, c + shift, w, 0.03))
    return pd.DataFrame({"SR_WL": wl, **cols})


def drop_zero_rows(table):
    """the reference's loading: indexed by SR_WL, rows where no band is above 1e-6 dropped"""
    t = table.set_index("SR_WL")
    return t.loc[np.any((t > 1e-6).values, axis=1)]


def s2_sensor(srf_s2, sensor):
    t = srf_s2[[c for c in srf_s2.columns if sensor in c]].copy()
    t.columns = [c.replace(f"{sensor}_SR_AV_", "") for c in t.columns]
    return t


def oracle_weights(bands, srf, wavelengths):
    """per output band: (AVIRIS band indices ascending, float64 weights), the reference's pandas arithmetic"""
    from scipy import interpolate
    near = interpolate.interp1d(wavelengths, np.arange(len(wavelengths)), kind="nearest")(srf.index).astype(int)
    table = pd.DataFrame({"SR_WL": srf.index, "AVIRIS_band": near}).set_index("SR_WL")
    out = []
    for b in bands:
        sel = srf.loc[~(srf[b] <= 1e-4), [b]].copy().join(table)
        sel["norm"] = sel[b] / sel[b].sum()
        g = sel.groupby("AVIRIS_band")[["norm"]].sum()
        out.append((g.index.values.astype(np.int64), g["norm"].values))
    return out


def oracle_transform(cube_chw, bands, srf, wavelengths, fill=None, weights=None):
    """(C, H, W) float32 -> (len(bands), H, W) float32: float64 products summed over the band axis, fill where any support value
    equals ``fill`` (None: nothing masked)"""
    cube = np.asarray(cube_chw)
    out = np.empty((len(bands),) + cube.shape[1:], np.float32)
    for j, (idx, w) in enumerate(weights or oracle_weights(bands, srf, wavelengths)):
        x = cube[idx]
        with np.errstate(invalid="ignore", over="ignore"):
            out[j] = np.sum(w[:, None, None] * x, axis=0)
        if fill is not None:
            out[j][np.any(x == fill, axis=0)] = fill
    return out


def all_sensor_weights(wv3=None, s2=None):
    """{sensor: (bands, srf)} for WV3, S2A and S2B from the synthetic tables"""
    wv3 = drop_zero_rows(wv3_table()) if wv3 is None else wv3
    s2 = drop_zero_rows(s2_table()) if s2 is None else s2
    return {"WV3": (WV3_BANDS, wv3), "S2A": (S2_BANDS, s2_sensor(s2, "S2A")), "S2B": (S2_BANDS, s2_sensor(s2, "S2B"))}


def load_g13():
    """the golden file as a dict of arrays; tables rebuilt as the DataFrames the reference ran on"""
    g = dict(np.load(os.path.join(G, "g13_srf.npz")))
    g["srf_wv3"] = pd.DataFrame(g["wv3_values"], index=pd.Index(g["wv3_wl"], name="SR_WL"),
                                columns=[str(c) for c in g["wv3_columns"]])
    g["srf_s2"] = pd.DataFrame(g["s2_values"], index=pd.Index(g["s2_wl"], name="SR_WL"),
                               columns=[str(c) for c in g["s2_columns"]])
    return g
