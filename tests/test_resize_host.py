"""Host side of the anti-aliased resize (starcop_amd/resample.py, io_formats.scaled_geo_tags, the argument checks of the
transform_to_* functions): no GPU needed.  The tap tables, applied by the numpy restatement of the kernel's rounding contract, are held
against the operator's definition -- scipy's gaussian_filter + zoom in float64 (tests/resize_util.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import resize_util as R
import srf_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.SHAPES, ids=lambda c: "{}x{}-{}x{}-s{}".format(*c[:5]))
def test_taps_match_the_scipy_oracle(case, mode):
    from starcop_amd import resample
    H, W, oh, ow, sigma, cval = case
    x = R.make_plane(H, W, seed=H * 1000 + W, cval=cval if cval else None)
    want = R.oracle64(x, (oh, ow), sigma, mode, cval)
    got = R.restatement(x, (oh, ow), sigma, mode, cval)
    d = R.ulps(got, want, x, cval)
    print(f"{case} {mode}: {d:.3f} x 2^-24 M")
    assert got.shape == (oh, ow) and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - want).max() <= R.gate(x, cval), d
    for n, o in ((H, oh), (W, ow)):
        start, w, wc = resample.axis_taps(n, o, sigma, mode)
        T = w.shape[1]
        r = int(4.0 * sigma + 0.5)
        assert start.dtype == np.int32 and w.dtype == np.float64 and w.shape == (o, T) and wc.shape == (o,)
        assert 1 <= T <= min(n, 2 * r + 2)
        assert (start >= 0).all() and (start + T <= n).all()
        assert (w >= 0).all() and (wc >= 0).all()
        assert np.abs(w.sum(axis=1) + wc - 1.0).max() <= 1e-15 * T
        if mode != "constant":
            assert (wc == 0).all()


def test_anisotropic_sigma_and_identity():
    x = R.make_plane(30, 44, seed=5)
    want = R.oracle64(x, (10, 11), (2.5, 0.5), "reflect", 0.0)
    got = R.restatement(x, (10, 11), (2.5, 0.5), "reflect", 0.0)
    assert np.abs(got - want).max() <= R.gate(x, 0.0)
    same = R.restatement(x, (30, 44), 0.0, "constant", 7.0)
    assert np.array_equal(same.view(np.uint32), x.view(np.uint32))


def test_gaussian_kernel_is_scipys():
    from scipy.ndimage import gaussian_filter1d
    from starcop_amd import resample
    for sigma in (0.5, 1.0, 1.5, 2.5, 5.5):
        g, r = resample.gaussian_kernel(sigma)
        assert r == int(4.0 * sigma + 0.5) and g.shape == (2 * r + 1,)
        impulse = np.zeros(4 * r + 3)
        impulse[2 * r + 1] = 1.0                                       # its response is the kernel itself: products with 0 and 1 only
        assert np.array_equal(gaussian_filter1d(impulse, sigma, mode="constant")[r + 1:3 * r + 2], g)
    g, r = resample.gaussian_kernel(0.0)
    assert r == 0 and np.array_equal(g, [1.0])


def test_output_shape_for():
    from starcop_amd import resample
    f = resample.output_shape_for
    assert f((16384, 668), 5, 20) == (4096, 167) and f((16384, 668), 5, 60) == (1365, 56)
    assert f((13, 60, 36), 5.0, 10) == (30, 18)                       # only the last two axes count
    assert f((5, 7), 5, 10) == (2, 4)                                 # 2.5 -> 2 and 3.5 -> 4: numpy rounds halves to even
    assert f((3, 3), 5, 60) == (1, 1)                                 # never below one pixel
    assert f((40, 40), (5, 10), (20, 20)) == (10, 20)                 # (y, x) pixel sizes
    assert f((40, 40), -5, 20) == (10, 10)                            # a negative (north-up) pixel height counts by its size
    assert resample.default_sigma(668, 56) == (668 / 56 - 1) / 2 and resample.default_sigma(40, 40) == 0.0


def test_value_errors():
    from starcop_amd import resample
    x = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError):
        resample.resize_antialiased(x, (9, 4))                        # a larger output
    with pytest.raises(ValueError):
        resample.resize_antialiased(x, (4, 4), sigma=-0.5)
    with pytest.raises(ValueError):
        resample.resize_antialiased(x, (4, 4), sigma=np.array([[1.0, -1.0]]))
    with pytest.raises(ValueError):
        resample.resize_antialiased(x, (4, 4), mode="wrap")
    with pytest.raises(ValueError):
        resample.resize_antialiased(x[None], (4, 4), sigma=[1.0, 2.0])   # two sigmas for one plane
    with pytest.raises(ValueError):
        resample.axis_taps(8, 9, 1.0, "constant")
    with pytest.raises(ValueError):
        resample.axis_taps(8, 4, -1.0, "constant")
    with pytest.raises(ValueError):
        resample.axis_taps(8, 4, 1.0, "grid-wrap")


def test_transform_resampling_arguments_are_checked_before_the_device(monkeypatch):
    from starcop_amd import _lib, aviris

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "require_device", no_device)
    monkeypatch.setattr(aviris, "SRF_WV3", U.drop_zero_rows(U.wv3_table()))
    monkeypatch.setattr(aviris, "SRF_S2", U.drop_zero_rows(U.s2_table()))
    cube = np.zeros((425, 8, 8), np.float32)
    grid = U.g3_grid()
    srf = aviris.load_srf_wv3()
    for call in (lambda **k: aviris.transform_to_srf(cube, ["SWIR1"], srf, bands_nanometers_aviris=grid, **k),
                 lambda **k: aviris.transform_to_worldview_3(cube, ["SWIR1"], bands_nanometers_aviris=grid, **k),
                 lambda **k: aviris.transform_to_sentinel_2(cube, ["B11"], bands_nanometers_aviris=grid, **k)):
        with pytest.raises(NotImplementedError, match="resolution_src"):
            call()                                                    # the reference's default resolution_dst=10, no resolution_src
        with pytest.raises(NotImplementedError, match="resolution_src"):
            call(resolution_dst=20)
        with pytest.raises(ValueError):
            call(resolution_dst=2.5, resolution_src=5)                # upsampling
    with pytest.raises(ValueError):
        aviris.transform_to_srf(cube, ["SWIR1"], srf, resolution_dst=20, resolution_src=5, bands_nanometers_aviris=grid, mode="wrap")
    with pytest.raises(ValueError):
        aviris.transform_to_srf(cube, ["SWIR1"], srf, resolution_dst=20, resolution_src=5, bands_nanometers_aviris=grid,
                                sigma_bands=[-1.0])
    assert np.array_equal(aviris.sentinel_2_sigmas(["B2", "B11", "B1"], 5), [0.5, 1.5, 5.5])
    assert np.array_equal(aviris.sentinel_2_sigmas(["B2", "B12"], (4.0, 5.0)), [0.5, 1.5])
    assert np.array_equal(aviris.sentinel_2_sigmas(["B2"], 20), [0.0])


def test_aviris_as_sensor_resolution_arguments(tmp_path):
    from starcop_amd import pipeline
    with pytest.raises(ValueError):
        pipeline.aviris_as_sensor(str(tmp_path), str(tmp_path / "out"), sensors=["S2A", "WV3"], resolution_dst="native")
    with pytest.raises(ValueError):
        pipeline.aviris_as_sensor(str(tmp_path), str(tmp_path / "out"), sensors=["S2A"], resolution_dst="sensor")
    with pytest.raises(ValueError):
        pipeline.aviris_as_sensor(str(tmp_path), str(tmp_path / "out"), sensors=["S2A"], resolution_dst=20, mode="wrap")
    assert not (tmp_path / "out").exists()


def test_scaled_geo_tags():
    from starcop_amd import io_formats as io
    keys = (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32611))
    # pixel scale + tiepoint: 60 x 36 pixels of 5 m -> 15 x 9 (ratio 4) and -> 7 x 5 (ratios 60 / 7 and 36 / 5)
    north_up = {33550: (12, (5.0, 5.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0)), 34735: keys,
                42113: (2, ("-9999",))}
    s = io.scaled_geo_tags(north_up, 60 / 15, 36 / 9)
    assert s[33550] == (12, (20.0, 20.0, 0.0)) and s[33922] == north_up[33922] and s[34735] == keys and s[42113] == north_up[42113]
    s = io.scaled_geo_tags(north_up, 60 / 7, 36 / 5)
    assert s[33550][1] == (5.0 * (36 / 5), 5.0 * (60 / 7), 0.0) and s[33922] == north_up[33922]
    assert s[33550][1][0] * 5 == 36 * 5.0                                      # the full extent maps onto the full extent
    assert 33550 in north_up and north_up[33550][1] == (5.0, 5.0, 0.0)         # the input is not modified
    # a transformation matrix (rotated flight line): the column vectors scale, the translation (the corner) stays
    m = (4.89, -1.04, 0.0, 500000.0, -1.04, -4.89, 0.0, 4100000.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    rot = {34264: (12, m), 34735: keys}
    s = io.scaled_geo_tags(rot, 4.0, 2.0)
    assert s[34264][1] == (4.89 * 2.0, -1.04 * 4.0, 0.0, 500000.0, -1.04 * 2.0, -4.89 * 4.0, 0.0, 4100000.0) + m[8:]
    assert s[34735] == keys
    # composes with window_geo_tags: the window (2, 3) of the raster scaled by (4, 2) is the window (8, 6) of the source, scaled
    for tags in (north_up, rot):
        a = io.window_geo_tags(io.scaled_geo_tags(tags, 4.0, 2.0), 2, 3)
        b = io.scaled_geo_tags(io.window_geo_tags(tags, 8, 6), 4.0, 2.0)
        assert set(a) == set(b)
        for t in a:
            assert a[t][0] == b[t][0] and np.allclose(a[t][1], b[t][1], rtol=1e-15, atol=0.0), (t, a[t], b[t])
    # a tiepoint that is not at the corner keeps its place on the ground
    off = {33550: (12, (5.0, 5.0, 0.0)), 33922: (12, (8.0, 4.0, 0.0, 500040.0, 4099980.0, 0.0))}
    s = io.scaled_geo_tags(off, 4.0, 2.0)
    assert s[33922][1] == (4.0, 1.0, 0.0, 500040.0, 4099980.0, 0.0)
    assert io.window_geo_tags(s, 0, 0)[33922][1] == io.window_geo_tags(off, 0, 0)[33922][1]      # the same corner
    assert io.scaled_geo_tags({}, 2.0, 2.0) == {}


def test_resize_structs_match_the_c_compiler(tmp_path):
    """sizeof / offsetof of sc_resize_axis and sc_resize_args as gcc lays them out == the ctypes mirrors in _lib.py"""
    from starcop_amd import _lib
    assert shutil.which("gcc") is not None, "gcc is needed to lay out sc_resize_args as the C compiler does"
    assert "sc_resize_aa" in _lib.SIGNATURES and "sc_resize_workspace_bytes" in _lib.SIGNATURES
    prints = []
    for name, cls in (("sc_resize_axis", _lib.sc_resize_axis), ("sc_resize_args", _lib.sc_resize_args)):
        prints.append(f'printf("%zu", sizeof({name}));')
        prints += [f'printf(" %zu", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "rs.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){' + 'printf(" ");'.join(prints)
                   + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "rs"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for cls in (_lib.sc_resize_axis, _lib.sc_resize_args):
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want
