"""Host rules of the window cutter (starcop_amd/window_dataset.py, sampling_dataset.py:182-386 of the reference): padding, file
naming, the acquisition-date factor, the georeferencing of a window and the grouping of table rows into chunks.  No GPU."""
import ctypes
import datetime
import math

import numpy as np
import pandas as pd
import pytest

import window_cut_util as U
from starcop_amd import _lib, aviris, io_formats as io, sampling, window_dataset as wd


def test_padding_rule():
    # odd deficit: 32 - 15 = 17 -> 8 leading, 9 trailing; even deficit: 32 - 20 = 12 -> 6 and 6
    assert wd.pad_window_to_size((100, 50, 15, 20), (32, 32)) == (92, 44, 32, 32)
    assert wd.pad_window_to_size((3, 2, 15, 15), (32, 32)) == (-5, -6, 32, 32)          # across the upper-left edge
    assert wd.pad_window_to_size((7, 9, 32, 32), (32, 32)) == (7, 9, 32, 32)            # equal size: unchanged
    assert wd.pad_window_to_size((7, 9, 40, 16), (32, 32)) == (7, 1, 40, 32)            # a large enough dimension is unchanged
    for win in [(100, 50, 15, 20), (3, 2, 15, 15), (7, 9, 32, 32), (0, 0, 1, 31), (7, 9, 40, 16)]:
        assert wd.pad_window_to_size(win, (32, 32)) == U.pad_window(win, (32, 32))

    class Win:
        row_off, col_off, height, width = 10, 20, 31, 30
    assert wd.pad_window_to_size(Win(), (32, 32)) == (10, 19, 32, 32)


def test_file_naming_for_every_key_class():
    want = {"S2A_B12": "TOA_S2A_B12", "S2B_B1": "TOA_S2B_B1", "WV3_SWIR1": "TOA_WV3_SWIR1", "640nm": "TOA_AVIRIS_640nm",
            "37": "TOA_AVIRIS_37", "mag1c": "mag1c", "label_rgba": "label_rgba", "labelbinary": "labelbinary"}
    for k, v in want.items():
        assert wd.save_name(k, True) == v
        assert wd.save_name(k, False) == k


def test_product_ops():
    f = 3.25
    s, c = wd.product_ops("S2B_B1", True, f)
    assert s == f / 100 / aviris.SOLAR_IRRADIANCE["S2B"]["B01"] and c == (0.0, 2.0)          # B1 is looked up as B01
    s, c = wd.product_ops("S2A_B8A", True, f)
    assert s == f / 100 / aviris.SOLAR_IRRADIANCE["S2A"]["B8A"] and c == (0.0, 2.0)
    s, c = wd.product_ops("WV3_SWIR1", True, f)
    assert s == f / 100 / (477.8728 / 1000) and c == (0.0, 2.0)
    assert wd.product_ops("12", True, f) == (f, None)
    assert wd.product_ops("mag1c", True, f) == (None, (0.0, 10000.0))
    assert wd.product_ops("label_rgba", True, f) == (None, None)
    assert wd.product_ops("S2B_B1", False, None) == (None, None) and wd.product_ops("12", False, None) == (None, None)


def test_earth_sun_distance():
    # day 4: cos(0) = 1
    assert aviris.earth_sun_distance_correction_factor(datetime.datetime(2019, 1, 4)) == 1 - 0.01673
    # 2019-10-18 is day 291: by hand 1 - 0.01673 cos(0.0172 * 287)
    d = aviris.earth_sun_distance_correction_factor(datetime.datetime(2019, 10, 18, 14, 15, 49))
    assert abs(d - (1 - 0.01673 * math.cos(0.0172 * 287))) < 1e-15
    assert abs(d - 0.99628) < 1e-5          # 0.0172 * 287 = 4.9364 rad, cos = 0.2222, 0.01673 * 0.2222 = 0.003717


def test_observation_date_factor():
    when = datetime.datetime(2019, 10, 18, 14, 15, 49)
    d = aviris.earth_sun_distance_correction_factor(when)
    assert aviris.observation_date_correction_factor(when, 90.0) == np.pi * d ** 2 / np.cos(0.0)
    assert aviris.observation_date_correction_factor(when, 30.0) == np.pi * (d ** 2) / np.cos((90 - 30.0) / 180. * np.pi)
    assert abs(aviris.observation_date_correction_factor(when, 30.0) - 2 * np.pi * d ** 2) < 1e-12      # cos 60 deg = 1 / 2


def _table(**extra):
    t = pd.DataFrame({"folder": ["/nowhere/ang20191018t141549/", "/nowhere/ang20191018t141549/"],
                      "window": [(0, 0, 16, 16), (8, 8, 16, 16)]}, index=["a", "b"])
    for k, v in extra.items():
        t[k] = v
    return t


def test_missing_factor_is_a_value_error_in_the_constructor():
    with pytest.raises(ValueError) as e:
        wd.WindowDataset(_table(), ["mag1c", "label_rgba", "S2B_B1"])
    assert "toa_correction_factor" in str(e.value) and "solar_altitude" in str(e.value)
    with pytest.raises(ValueError):
        wd.WindowDataset(_table(), ["mag1c", "label_rgba"], wavelengths=[640.])
    # either source is enough, and nothing is needed without normalisation (no file is touched by the constructor)
    when = pd.Timestamp("2019-10-18T14:15:49Z")
    ds = wd.WindowDataset(_table(datetime=[when, when], solar_altitude=[30.0, 55.0]), ["mag1c", "label_rgba", "S2B_B1"])
    want = aviris.observation_date_correction_factor(when.to_pydatetime(), 30.0)            # the first row of the folder decides
    assert ds.toa_correction_factor == {"/nowhere/ang20191018t141549/": want}
    ds = wd.WindowDataset(_table(), ["mag1c", "label_rgba", "12"], toa_correction_factor={"/nowhere/ang20191018t141549/": 2.5})
    assert ds.toa_correction_factor == {"/nowhere/ang20191018t141549/": 2.5}
    assert len(wd.WindowDataset(_table(), ["mag1c", "label_rgba", "S2B_B1"], normalize_by_acquisition_date=False)) == 2
    assert sampling.WindowDataset is wd.WindowDataset


def test_constructor_rules():
    with pytest.raises(NotImplementedError):
        wd.WindowDataset(_table(), ["mag1c", "label_rgba"], read_label_path=True)
    with pytest.raises(NotImplementedError):
        wd.WindowDataset(_table(), ["mag1c", "label_rgba"], read_rgb_path=True)
    with pytest.raises(ValueError):
        wd.WindowDataset(_table(), ["mag1c", "label_rgba"], output_size=(8, 32))             # 16 rows do not fit 8
    t = _table()
    t["folder"] = ["gs://bucket/a/", "gs://bucket/a/"]
    with pytest.raises(NotImplementedError):
        wd.WindowDataset(t, ["mag1c", "label_rgba"])
    ds = wd.WindowDataset(_table(), ["mag1c", "label_rgba"], output_size=(32, 32))
    assert ds.windows == [(-8, -8, 32, 32), (0, 0, 32, 32)]
    with pytest.raises(NotImplementedError):
        ds.cache("gs://bucket/out", "train")


def test_window_geo_tags():
    keys = (3, (1, 1, 0, 1, 3072, 0, 1, 32613))
    tie = {33550: (12, (5.0, 4.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 600000.0, 3500000.0, 0.0)), 34735: keys,
           42113: (2, ("-9999",)), 42112: (2, ("<GDALMetadata/>",))}
    got = io.window_geo_tags(tie, -8, 6)
    assert got == {33550: (12, (5.0, 4.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 600000.0 + 6 * 5.0, 3500000.0 + 8 * 4.0, 0.0)), 34735: keys}
    # a tiepoint that is not at pixel (0, 0)
    tie[33922] = (12, (2.0, 1.0, 0.0, 600000.0, 3500000.0, 0.0))
    assert io.window_geo_tags(tie, 3, -2)[33922] == (12, (0.0, 0.0, 0.0, 600000.0 - 4 * 5.0, 3500000.0 - 2 * 4.0, 0.0))
    # ModelTransformation: x = a col + b row + d, y = e col + f row + h
    a, b, d, e, f, h = 4.0, 1.5, 1000.0, 1.25, -4.5, 9000.0
    mt = {34264: (12, (a, b, 0.0, d, e, f, 0.0, h, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)), 34735: keys}
    got = io.window_geo_tags(mt, -3, 7)
    assert got[34264] == (12, (a, b, 0.0, d + 7 * a - 3 * b, e, f, 0.0, h + 7 * e - 3 * f, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0))
    assert got[34735] == keys and set(got) == {34264, 34735}
    assert io.window_geo_tags({42113: (2, ("0",))}, 1, 2) == {}
    info = io.TiffInfo()
    info.tags = dict(tie)
    assert io.window_geo_tags(info, 0, 0)[33922][1][3:5] == (600000.0 - 2 * 5.0, 3500000.0 + 1 * 4.0)


def test_rows_are_grouped_into_flight_lines_and_chunks():
    rng = np.random.default_rng(5)
    folders = [("A/", "B/", "C/")[k] for k in rng.integers(0, 3, 40)]
    scene_rows = {"A/": 1000, "B/": 300, "C/": 64}
    row_bytes = {"A/": 1000, "B/": 10, "C/": 5}
    windows = [(int(rng.integers(-40, scene_rows[f] + 40)), int(rng.integers(-10, 50)), 64, 64) for f in folders]
    windows[3] = (-500, 0, 64, 64)                       # wholly above its flight line
    budget = 200 * 1000                                  # A/: at most 200 rows of source per chunk
    chunks = wd.plan_chunks(folders, windows, scene_rows, row_bytes, budget)
    seen = sorted(i for c in chunks for i in c["rows"])
    assert seen == list(range(40))                       # every row in exactly one chunk
    for c in chunks:
        f, (b0, b1) = c["folder"], c["band"]
        assert 0 <= b0 < b1 <= scene_rows[f]
        assert all(folders[i] == f for i in c["rows"])
        for i in c["rows"]:                              # the band covers what the window holds of the flight line
            r, _, h, _ = windows[i]
            lo, hi = max(r, 0), min(r + h, scene_rows[f])
            assert hi <= lo or (b0 <= lo and hi <= b1)
        assert len(c["rows"]) == 1 or (b1 - b0) * row_bytes[f] <= budget
        offs = [windows[i][0] for i in c["rows"]]
        assert offs == sorted(offs)
    assert sum(c["folder"] == "A/" for c in chunks) > 1 and sum(c["folder"] == "C/" for c in chunks) == 1
    # one chunk per flight line under a budget that holds everything
    assert len(wd.plan_chunks(folders, windows, scene_rows, row_bytes, 1 << 40)) == 3


def test_struct_layout_matches_the_c_compiler(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    A = _lib.sc_wcut_args
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sc_wcut_args), offsetof(sc_wcut_args, win_off_host), '
                   'offsetof(sc_wcut_args, src), offsetof(sc_wcut_args, col_stride), offsetof(sc_wcut_args, row0), '
                   'offsetof(sc_wcut_args, ops), offsetof(sc_wcut_args, clip_hi), offsetof(sc_wcut_args, out));return 0;}\n')
    exe = tmp_path / "sz"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(A), A.win_off_host.offset, A.src.offset, A.col_stride.offset, A.row0.offset, A.ops.offset,
                   A.clip_hi.offset, A.out.offset]


def test_host_argument_checks_need_no_device():
    """the checks that come before anything touches the device return SC_ERR_ARG on a box without a GPU too"""
    lib = _lib.load()
    off = np.zeros((1, 2), np.int32)
    a = _lib.sc_wcut_args()
    a.scene_rows, a.scene_cols, a.out_h, a.out_w, a.P, a.elem_bytes, a.n_win = 8, 8, 4, 4, 65, 4, 1
    a.win_off, a.win_off_host, a.out = 4096, off.ctypes.data, 4096
    assert lib.sc_window_cut(a, None) == -1 and b"P=65" in lib.sc_last_error()
    a.P, a.elem_bytes = 1, 1
    a.src[0], a.rows[0], a.cols[0], a.row_stride[0], a.col_stride[0] = 4096, 8, 8, 8, 1
    a.ops[0], a.scale[0] = _lib.WCUT_SCALE, 2.0
    assert lib.sc_window_cut(a, None) == -1 and b"scale" in lib.sc_last_error()
    a.ops[0], a.rows[0] = 0, 9
    assert lib.sc_window_cut(a, None) == -1 and b"scene" in lib.sc_last_error()
    a.rows[0], a.elem_bytes = 8, 8
    assert lib.sc_window_cut(a, None) == -1
    a.elem_bytes = 4
    off[0] = (2 ** 31 - 3, 0)
    assert lib.sc_window_cut(a, None) == -1 and b"int32" in lib.sc_last_error()
