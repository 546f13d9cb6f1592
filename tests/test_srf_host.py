"""Host side of the simulated WV3 / S2 bands (starcop_amd.aviris): SRF loading, the CSR weights against the reference's own
weight_per_aviris_band (g13_srf.npz), the numpy oracle against the reference's outputs, and the sc_srf_args layout.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import srf_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g13():
    return U.load_g13()


def _sensor_srf(g, sensor):
    return g["srf_wv3"] if sensor == "WV3" else U.s2_sensor(g["srf_s2"], sensor)


@pytest.mark.parametrize("grid", ["g3", "emit"])
@pytest.mark.parametrize("sensor", ["WV3", "S2A", "S2B"])
def test_srf_weights_bit_equal_to_the_reference(g13, grid, sensor):
    from starcop_amd import aviris
    bands = U.WV3_BANDS if sensor == "WV3" else U.S2_BANDS
    p, b, w = aviris.srf_weights(bands, _sensor_srf(g13, sensor), g13[f"{grid}_grid"])
    assert p.dtype == np.int32 and b.dtype == np.int32 and w.dtype == np.float64
    assert np.array_equal(p, g13[f"{grid}_{sensor}_ptr"])
    assert np.array_equal(b, g13[f"{grid}_{sensor}_band"])
    assert np.array_equal(w.view(np.uint64), g13[f"{grid}_{sensor}_w"].view(np.uint64))


def test_golden_covers_midpoints_and_small_weights(g13):
    """the synthetic tables exercise what the issue asks for: x.5 nm rows on band midpoints of the G3 grid, rows between 1e-6
    and 1e-4 (kept by the loader, dropped from the weights)"""
    grid = g13["g3_grid"]
    mids = grid[:-1] / 2.0 + grid[1:] / 2.0
    assert np.isin(g13["wv3_wl"], mids).sum() >= 4 and np.isin(g13["s2_wl"], mids).sum() >= 4
    v = g13["wv3_values"]
    assert ((v > 1e-6) & (v <= 1e-4)).any()
    from starcop_amd import aviris
    near = aviris.nearest_band(grid, [1209.5, 1212.0, 1214.5, 1214.6])
    assert list(near) == [166, 167, 167, 168]                  # a midpoint goes to the lower band


def test_oracle_matches_the_reference_outputs(g13):
    """tests/srf_util.py's restatement == the reference's transform_to_srf on every golden cube (NaN positions by isnan)"""
    for name in g13["names"]:
        name = str(name)
        grid = g13[f"{name}_grid"]
        fill = float(g13[f"{name}_fill"][0])
        fill = None if np.isnan(fill) else fill
        for sensor in ("WV3", "S2A", "S2B"):
            bands = U.WV3_BANDS if sensor == "WV3" else U.S2_BANDS
            want = g13[f"{name}_{sensor}_out"]
            got = U.oracle_transform(g13[f"{name}_cube"], bands, _sensor_srf(g13, sensor), grid, fill)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (name, sensor)


def test_out_of_range_rows_raise():
    from starcop_amd import aviris
    srf = pd.DataFrame({"SWIR1": [0.5, 1.0, 0.5]}, index=pd.Index([1200.0, 1210.0, 2600.0], name="SR_WL"))
    with pytest.raises(ValueError):
        aviris.srf_weights(["SWIR1"], srf, U.g3_grid())
    srf.index = pd.Index([370.0, 1210.0, 1220.0], name="SR_WL")
    with pytest.raises(ValueError):
        aviris.srf_weights(["SWIR1"], srf, U.g3_grid())
    with pytest.raises(ValueError):
        aviris.nearest_band(U.g3_grid(), [2497.5])
    assert aviris.nearest_band(U.g3_grid(), [377.0, 2497.0]).tolist() == [0, 424]


def test_load_srf_local_csv(tmp_path, monkeypatch):
    from starcop_amd import aviris
    wv3 = U.wv3_table()
    wv3.loc[len(wv3)] = [2451.0] + [0.0] * 8                       # an all-zero row
    wv3.loc[len(wv3)] = [2452.0] + [5e-7] * 8                      # nothing above 1e-6
    p = tmp_path / "wv3.csv"
    wv3.to_csv(p, index=False)
    monkeypatch.setattr(aviris, "SRF_WV3", None)
    t = aviris.load_srf_wv3(cache=False, path_override=str(p))
    raw = pd.read_csv(p).set_index("SR_WL")
    assert 2451.0 not in t.index and 2452.0 not in t.index and len(t) == len(U.drop_zero_rows(wv3))
    pd.testing.assert_frame_equal(t, raw.loc[t.index])
    assert aviris.SRF_WV3 is None
    # the cache: filled by a cached load, then returned whatever the path
    t2 = aviris.load_srf_wv3(path_override=str(p))
    assert aviris.SRF_WV3 is t2 and aviris.load_srf_wv3(path_override="gs://elsewhere/x.csv") is t2
    # gs:// is refused before anything is read
    monkeypatch.setattr(aviris, "SRF_WV3", None)
    with pytest.raises(NotImplementedError):
        aviris.load_srf_wv3()
    monkeypatch.setattr(aviris, "SRF_S2", None)
    with pytest.raises(NotImplementedError):
        aviris.load_srf_s2(cache=False)

    s2p = tmp_path / "s2.csv"
    s2 = U.s2_table()
    s2.loc[len(s2)] = [411.0] + [0.0] * 26
    s2 = s2.sort_values("SR_WL", ignore_index=True)
    s2["S2A_SR_AV_B1"] += 2e-6                                      # every row kept: 411 .. 2320 nm
    s2.to_csv(s2p, index=False)
    full = aviris.load_srf_s2(cache=False, path_override=str(s2p))
    assert full.index[0] == 411.0 and len(full) == len(s2)
    cut = aviris.load_srf_s2(cache=False, path_override=str(s2p), drop_by_minimum=420)      # drops 411 .. 419 nm
    assert cut.index[0] == 420.0 and len(cut) == len(full) - 9 and aviris.SRF_S2 is None
    assert len(aviris.load_srf_s2(cache=False, path_override=str(s2p), drop_by_minimum=True)) == len(full)
    cached = aviris.load_srf_s2(path_override=str(s2p))
    assert aviris.SRF_S2 is cached
    s2a = aviris.sentinel_2_srf("S2B")
    assert list(s2a.columns) == U.S2_BANDS and np.array_equal(s2a["B8A"].values, cached["S2B_SR_AV_B8A"].values)


def test_transform_arguments_are_checked_before_the_device():
    from starcop_amd import aviris
    cube = np.zeros((425, 2, 2), np.float32)
    srf = U.drop_zero_rows(U.wv3_table())
    with pytest.raises(NotImplementedError):
        aviris.transform_to_srf(cube, ["SWIR1"], srf, bands_nanometers_aviris=U.g3_grid())          # resolution_dst=10
    with pytest.raises(ValueError):
        aviris.transform_to_srf(cube, ["SWIR1"], srf, resolution_dst=None)


def test_aviris_as_sensor_checks_its_arguments(tmp_path):
    from starcop_amd import pipeline
    with pytest.raises(NotImplementedError):
        pipeline.aviris_as_sensor(str(tmp_path), str(tmp_path / "out"), sensors=["WV3", "L8"])
    with pytest.raises(NotImplementedError):
        pipeline.aviris_as_sensor(str(tmp_path / "x.tif"), str(tmp_path / "out"))
    with pytest.raises(NotImplementedError):                        # no <name>_img: the one-file-per-band layout
        pipeline.aviris_as_sensor(str(tmp_path), str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()
    assert list(pipeline.BANDS_SENSOR) == ["S2A", "S2B", "WV3"] and pipeline.BANDS_SENSOR["WV3"] == U.WV3_BANDS


def test_srf_struct_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sc_srf_args as gcc lays it out == the ctypes mirror in _lib.py"""
    from starcop_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f for f, _ in _lib.sc_srf_args._fields_]
    assert fields == ["x", "line_stride", "sample_stride", "band_stride", "L", "S", "B", "n_out", "ptr", "band", "w", "ptr_host",
                      "band_host", "out", "out_plane_stride", "out_line_stride", "has_fill", "fill"]
    src = tmp_path / "srf.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){printf("%zu", sizeof(sc_srf_args));'
                   + "".join(f'printf(" %zu", offsetof(sc_srf_args, {f}));' for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "srf"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.sc_srf_args)] + [getattr(_lib.sc_srf_args, f).offset for f in fields]
