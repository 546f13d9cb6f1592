"""Generates tests/golden/g12_mlr.npz by IMPORTING THE REFERENCE ITSELF (starcop/data/feature_extration.py; sklearn).

Run in the build container only (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mlr.py

Seeded WV3-like tiles (tests/mlr_util.py) -> the reference's ratio_MLR_local outputs for every division, on the float32 tiles
and on float64 copies of them, its LinearRegression coef_ / intercept_, and the FEATURES registry's keys and inputs.
Only DATA is written, compactly (read it with mlr_util.load_g12):
  * the tiles are quantised to 16-bit counts of 2^-14 (as sensor products are), stored as uint16; counts / 16384 is exact in
    float32 and is what the reference was run on;
  * the float64 run is stored as its float32 difference to the float32 run (|difference| ~1e-6, so the float64 values come
    back to ~1e-13);
  * autoclip=True is np.clip(c_matched_outliers, -0.2, 0.2) in the reference (feature_extration.py:107-108): it is derived
    from the stored c_matched_outliers outputs instead of being stored.
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))
sys.modules.setdefault("rasterio", types.ModuleType("rasterio"))

from sklearn.linear_model import LinearRegression  # noqa: E402
from starcop.data import feature_extration as ref_feat  # noqa: E402
from mlr_util import QUANT, wv3_tile  # noqa: E402

DIVISIONS = ("c_matched_outliers", "simple_plus", "residual")


def tiles():
    rng = np.random.default_rng(12)
    out = {"wv3a": wv3_tile(rng, 72, 72, border=4), "wv3b": wv3_tile(rng, 47, 61, border=3)}
    b, t = wv3_tile(rng, 48, 48, border=3)
    b[2] = np.float32(0.21)                      # a constant regressor band (nodata border included)
    out["const"] = (b, t)
    out["zero"] = (np.zeros((5, 32, 32), np.float32), np.zeros((32, 32), np.float32))
    out["k9"] = wv3_tile(rng, 56, 56, k=9, border=3)
    # 16-bit counts of 2^-14: the float32 tiles the reference runs on are counts / QUANT exactly
    return {k: (np.round(b * QUANT).astype(np.uint16), np.round(t * QUANT).astype(np.uint16)) for k, (b, t) in out.items()}


def main():
    data = {}
    names = []
    for name, (bands_q, target_q) in tiles().items():
        names.append(name)
        data[f"{name}_bands_q"], data[f"{name}_target_q"] = bands_q, target_q
        bands, target = bands_q.astype(np.float32) / np.float32(QUANT), target_q.astype(np.float32) / np.float32(QUANT)
        res = {}
        for tag, dt in (("f32", np.float32), ("f64", np.float64)):
            b, t = bands.astype(dt), target.astype(dt)
            for div in DIVISIONS:
                with np.errstate(invalid="ignore", divide="ignore"):
                    res[(tag, div)] = ref_feat.ratio_MLR_local(list(b.copy()), t.copy(), division=div)
            m = LinearRegression().fit(b.reshape(b.shape[0], -1).T, t.reshape(-1))
            data[f"{name}_{tag}_coef"] = np.asarray(m.coef_, dtype=np.float64)
            data[f"{name}_{tag}_intercept"] = np.float64(m.intercept_)
        for div in DIVISIONS:
            f32 = res[("f32", div)]
            assert f32.dtype == np.float32
            data[f"{name}_f32_{div}"] = f32
            with np.errstate(invalid="ignore"):
                data[f"{name}_d64_{div}"] = (res[("f64", div)] - f32.astype(np.float64)).astype(np.float32)
    data["names"] = np.array(names)
    keys = list(ref_feat.FEATURES)
    data["registry_keys"] = np.array(keys)
    data["registry_inputs"] = np.array([",".join(ref_feat.FEATURES[k]["inputs"]) for k in keys])
    np.savez_compressed(os.path.join(OUT, "g12_mlr.npz"), **data)


if __name__ == "__main__":
    main()
