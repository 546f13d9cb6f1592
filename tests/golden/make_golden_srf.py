"""Generates tests/golden/g13_srf.npz by RUNNING THE REFERENCE ITSELF (starcop/data/aviris.py: load_srf_wv3 / load_srf_s2 on local
CSVs, transform_to_srf / transform_to_worldview_3 / transform_to_sentinel_2 with resolution_dst=None).

Run in the build container only (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_srf.py

georeader, rasterio and rasterio.windows are stubbed as empty modules (plus a small GeoTensor with ``.load()``), and the AVIRIS
image is a duck-typed raster with ``.shape`` and ``.isel({"band": idx}).load()``.  The values it hands out record the float64
weight vector numpy multiplies them by, so the reference's own ``weight_per_aviris_band`` is stored next to its outputs.
The SRF tables are the synthetic ones of tests/srf_util.py (WV3 SWIR1..8 at the centres of aviris.py:51, the joint S2 table) in
the reference's CSV format, with rows at x.5 nm on band midpoints and rows between 1e-6 and 1e-4; the band grids are the G3
AVIRIS 425-band grid and the 285-band EMIT grid (non-integer spacing).  Only DATA is written.
"""
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))


class GeoTensor:
    def __init__(self, values, transform=None, crs=None, fill_value_default=None):
        self.values, self.transform, self.crs, self.fill_value_default = values, transform, crs, fill_value_default
        self.shape = np.shape(values)
        self.res = (5.0, 5.0)

    def load(self):
        return self


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


_stub("georeader", read=_stub("georeader.read"), window_utils=_stub("georeader.window_utils"))
_stub("georeader.abstract_reader", GeoData=object)
_stub("georeader.geotensor", GeoTensor=GeoTensor)
_stub("georeader.rasterio_reader", RasterioReader=object)
_stub("rasterio", windows=_stub("rasterio.windows", Window=object))

from starcop.data import aviris as ref  # noqa: E402
import srf_util as U  # noqa: E402

WEIGHTS = []


class Recorded(np.ndarray):
    """band values that record the float64 weights of ``w[:, None, None] * values``"""

    def __array_ufunc__(self, ufunc, method, *inputs, **kw):
        plain = [np.asarray(v) if isinstance(v, Recorded) else v for v in inputs]
        if ufunc is np.multiply and method == "__call__":
            WEIGHTS.append(np.asarray([v for v in inputs if not isinstance(v, Recorded)][0], dtype=np.float64).ravel().copy())
        return getattr(ufunc, method)(*plain, **kw)


class Raster:
    def __init__(self, values, fill):
        self.values, self.fill_value_default = values, fill
        self.shape = values.shape
        self.transform = self.crs = None
        self.res = (5.0, 5.0)
        self.bands = []

    def isel(self, sel):
        idx = np.asarray(sel["band"])
        self.bands.append(idx.astype(np.int32))
        return GeoTensor(self.values[idx].view(Recorded), fill_value_default=self.fill_value_default)


def cubes(rng):
    """(name, grid, (C, H, W) float32 cube, fill or None)"""
    out = []
    for name, grid, (H, W) in (("g3", U.g3_grid(), (6, 7)), ("emit", U.emit_grid(), (5, 6))):
        c = (rng.integers(0, 20 * 1024, size=(grid.size, H, W)) / 1024.0).astype(np.float32)
        pix = rng.integers(0, H * W, size=8)
        bnd = rng.integers(0, grid.size, size=8)
        c.reshape(grid.size, -1)[bnd, pix] = -9999.0          # scattered fill, inside and outside the supports
        c[:, 0, 0] = -9999.0                                  # a pixel that is fill in every band
        out.append((name, grid, c, -9999.0))
    grid = U.g3_grid()
    s = (rng.integers(0, 20 * 1024, size=(grid.size, 3, 4)) / 1024.0).astype(np.float32)
    s[:, 0, 1] = -0.0                                         # all -0.0: the sum stays -0.0
    s[360, 0, 2] = np.nan                                     # NaN inside a WV3 / S2 B12 support
    s[:, 1, 0] = 1.0e38                                       # near the float32 maximum
    s[::2, 1, 1] = -1.0e38
    s[200, 2, 3] = -9999.0
    s[361, 2, 2] = np.nan
    s[362, 2, 2] = -9999.0                                    # fill wins over NaN
    out.append(("special", grid, s, -9999.0))
    nf = (rng.integers(0, 20 * 1024, size=(grid.size, 4, 5)) / 1024.0).astype(np.float32)
    nf[250, 1, 1] = -9999.0                                   # no fill value: -9999 is an ordinary value
    out.append(("nofill", grid, nf, None))
    return out


def main():
    rng = np.random.default_rng(13)
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        U.wv3_table().to_csv(os.path.join(tmp, "wv3.csv"), index=False)
        U.s2_table().to_csv(os.path.join(tmp, "s2.csv"), index=False)
        ref.SRF_WV3 = ref.SRF_S2 = None
        srf_wv3 = ref.load_srf_wv3(cache=True, path_override=os.path.join(tmp, "wv3.csv"))
        srf_s2 = ref.load_srf_s2(cache=True, path_override=os.path.join(tmp, "s2.csv"))
    for key, t in (("wv3", srf_wv3), ("s2", srf_s2)):
        data[f"{key}_wl"] = t.index.values.astype(np.float64)
        data[f"{key}_values"] = t.values.astype(np.float64)
        data[f"{key}_columns"] = np.array(list(t.columns))
    names = []
    for name, grid, cube, fill in cubes(rng):
        names.append(name)
        data[f"{name}_grid"] = grid
        data[f"{name}_cube"] = cube
        data[f"{name}_fill"] = np.array([np.nan if fill is None else fill])
        for sensor in ("WV3", "S2A", "S2B"):
            bands = U.WV3_BANDS if sensor == "WV3" else U.S2_BANDS
            raster = Raster(cube, fill)
            WEIGHTS.clear()
            fdef = 0.0 if fill is None else fill
            if sensor == "WV3":
                res = ref.transform_to_worldview_3(raster, bands, resolution_dst=None, bands_nanometers_aviris=list(grid),
                                                   fill_value_default=fdef)
            else:
                res = ref.transform_to_sentinel_2(raster, bands, resolution_dst=None, sensor=sensor, bands_nanometers_aviris=list(grid),
                                                  fill_value_default=fdef)
            assert res.values.dtype == np.float32 and len(WEIGHTS) == len(bands) == len(raster.bands)
            data[f"{name}_{sensor}_out"] = res.values
            if name in ("g3", "emit"):                 # the weights depend on the grid only
                data[f"{name}_{sensor}_ptr"] = np.cumsum([0] + [len(b) for b in raster.bands]).astype(np.int32)
                data[f"{name}_{sensor}_band"] = np.concatenate(raster.bands).astype(np.int32)
                data[f"{name}_{sensor}_w"] = np.concatenate(WEIGHTS)
    data["names"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "g13_srf.npz"), **data)


if __name__ == "__main__":
    main()
