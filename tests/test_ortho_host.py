"""Host side of the GLT orthorectification (starcop_amd.ortho, mag1c.mag1c_emit, the georeferenced / out_folder arguments of the
EMIT pipeline): exports, the ctypes mirror of sc_ortho_args, the GeoTIFF tags of the orthorectified grid and the argument checks
that run before any device work.  No GPU."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import ortho_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)
WKT = 'GEOGCS["WGS 84",DATUM["WGS_1984",SPHEROID["WGS 84",6378137,298.257223563]],PRIMEM["Greenwich",0],UNIT["degree",0.0174532925199433]]'


def test_exports_and_signatures():
    from starcop_amd import _lib, mag1c, ortho, pipeline
    assert "sc_glt_ortho" in _lib.SIGNATURES and _lib.ORTHO_MAX_PLANES == 64
    p = inspect.signature(ortho.georeference).parameters
    assert list(p)[:6] == ["data", "glt_x", "glt_y", "fill_value_default", "absolute", "check"]
    assert p["fill_value_default"].default == -9999.0 and p["absolute"].default is False and p["check"].default is True
    assert list(inspect.signature(ortho.emit_geo_tags).parameters) == ["geotransform", "spatial_ref"]
    m = inspect.signature(mag1c.mag1c_emit).parameters
    assert list(m) == ["raw", "wavelengths", "fwhm", "fill_value", "glt_x", "glt_y", "georreferenced", "column_step", "num_iter",
                       "covariance_lerp_alpha", "use_wavelength_range"]
    assert m["georreferenced"].default is True and m["column_step"].default is None and m["num_iter"].default == 30
    assert m["covariance_lerp_alpha"].default == 1e-4 and tuple(m["use_wavelength_range"].default) == (2122, 2488)
    assert inspect.signature(pipeline.emit_scene_predict).parameters["georeferenced"].default is False
    g = inspect.signature(pipeline.emit_granule_predict).parameters
    assert g["georeferenced"].default is False and g["out_folder"].default is None and g["overwrite"].default is False
    assert g["geotransform"].default is None
    assert "ortho" in open(os.path.join(ROOT, "starcop_amd", "__init__.py")).read()


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from starcop_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(sc_ortho_args), offsetof(sc_ortho_args, src), '
                   'offsetof(sc_ortho_args, row_stride), offsetof(sc_ortho_args, plane_rows), offsetof(sc_ortho_args, plane_cols), '
                   'offsetof(sc_ortho_args, fill_bits), offsetof(sc_ortho_args, out), offsetof(sc_ortho_args, oob_count), '
                   'SC_ORTHO_MAX_PLANES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.sc_ortho_args
    assert got == [ctypes.sizeof(A), A.src.offset, A.row_stride.offset, A.plane_rows.offset, A.plane_cols.offset, A.fill_bits.offset,
                   A.out.offset, A.oob_count.offset, _lib.ORTHO_MAX_PLANES]


def test_emit_geo_tags_round_trip(tmp_path):
    from starcop_amd import io_formats as io, ortho
    tags = ortho.emit_geo_tags(GT, WKT)
    assert tags[33550] == (12, (GT[1], -GT[5], 0.0)) and tags[33922] == (12, (0.0, 0.0, 0.0, GT[0], GT[3], 0.0))
    assert tags[34735][1][-1] == 4326 and tags[34735][1][7] == 2          # GTModelType = geographic, WGS 84
    assert tags == ortho.emit_geo_tags(np.array(GT)) == ortho.emit_geo_tags(list(GT), WKT.encode())
    # the same keys io_formats.envi_geo_tags writes for an ENVI "Geographic Lat/Lon" map info of that grid
    envi = io.envi_geo_tags({"map info": ["Geographic Lat/Lon", "1", "1", repr(GT[0]), repr(GT[3]), repr(GT[1]), repr(-GT[5]), "WGS-84"]})
    assert envi == tags
    a = np.arange(60 * 70, dtype=np.float32).reshape(60, 70)
    path = str(tmp_path / "g.tif")
    io.write_tiff(path, a, blocksize=128, extra_tags={**tags, 42113: (2, ("-9999",))})
    info = io.tiff_info(path)
    geo = info.geo_tags()
    assert geo[33550] == tags[33550] and geo[33922] == tags[33922] and geo[34735] == tags[34735] and geo[42113][1][0] == "-9999"
    assert np.array_equal(io.read_tiff(path)[0], a)


def test_emit_geo_tags_refuses_what_it_cannot_express():
    from starcop_amd import ortho
    with pytest.raises(NotImplementedError):
        ortho.emit_geo_tags((GT[0], GT[1], 1e-6, GT[3], 0.0, GT[5]))
    with pytest.raises(NotImplementedError):
        ortho.emit_geo_tags((GT[0], GT[1], 0.0, GT[3], -1e-6, GT[5]))
    with pytest.raises(NotImplementedError):
        ortho.emit_geo_tags(GT, 'PROJCS["NAD27 / UTM zone 11N"]')
    with pytest.raises(ValueError):
        ortho.emit_geo_tags(GT[:5])


def test_mag1c_emit_needs_a_glt_to_georeference():
    from starcop_amd import mag1c
    raw = np.ones((4, 3, 285), dtype=np.float32)
    wl = np.linspace(381.0, 2493.0, 285)
    with pytest.raises(ValueError, match="glt"):
        mag1c.mag1c_emit(raw, wl, np.full(285, 8.0), -9999.0)
    with pytest.raises(ValueError, match="glt"):
        mag1c.mag1c_emit(raw, wl, np.full(285, 8.0), -9999.0, glt_x=np.ones((2, 2), np.int32))


def test_out_folder_argument_checks():
    from starcop_amd import pipeline
    nc = os.path.join(ROOT, "tests", "golden", "io", "emit_l1b_like_sb0.nc")
    with pytest.raises(NotImplementedError, match="gs://"):
        pipeline.emit_granule_predict(None, nc, georeferenced=True, out_folder="gs://bucket/products")
    with pytest.raises(ValueError, match="georeferenced"):
        pipeline.emit_granule_predict(None, nc, out_folder="/nonexistent/products")
    with pytest.raises(ValueError, match="rows"):
        pipeline.emit_granule_predict(None, nc, georeferenced=True, rows=slice(0, 8))
    with pytest.raises(ValueError, match="glt"):
        pipeline.emit_scene_predict(None, np.zeros((2, 2, 3), np.float32), [1.0, 2.0, 3.0], [1.0], georeferenced=True)


def test_wrapper_argument_checks_need_no_device():
    """everything the wrapper can refuse from shapes and dtypes alone is refused before the device is touched"""
    import torch
    from starcop_amd import ortho
    gx, gy = U.identity_glt(3, 4)
    with pytest.raises(ValueError, match="shape"):
        ortho.georeference([torch.zeros(3, 4), torch.zeros(2, 4)], gx, gy)
    with pytest.raises(ValueError, match="dtype"):
        ortho.georeference([torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.float64)], gx, gy)
    with pytest.raises(ValueError, match="not supported"):
        ortho.georeference(torch.zeros(3, 4, dtype=torch.complex64), gx, gy)
    with pytest.raises(ValueError, match="fill"):
        ortho.georeference(torch.zeros(3, 4, dtype=torch.uint8), gx, gy)          # -9999 does not fit uint8
    with pytest.raises(ValueError, match="fill values"):
        ortho.georeference(torch.zeros(2, 3, 4), gx, gy, fill_value_default=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="rows, cols"):
        ortho.georeference(torch.zeros(2, 2, 3, 4), gx, gy)


def test_oracle_is_the_restated_gather_and_fill_patterns_agree():
    """the oracle against a plain loop over the definition (1-based indices, 0 = no data, absolute for signed tables), and the
    bit patterns the wrapper hands the kernel for a fill value against what the oracle's np.full holds"""
    from starcop_amd import planes
    for dt, fills in (("float32", [-9999.0, float("nan"), -0.0, np.float32(1e-40)]), ("float64", [-9999.0, float("nan"), -0.0]),
                      ("uint8", [0, 255, 7.0]), ("int16", [-9999, -9999.0, 32767]), ("int32", [-9999.0, -2 ** 31])):
        for f in fills:
            held = np.full((1,), f, dtype=dt)
            assert planes.fill_bits(f, np.dtype(dt), "georeference") == int(held.view(f"u{held.itemsize}")[0]), (dt, f)
    rng = np.random.default_rng(3)
    src = rng.standard_normal((5, 7)).astype(np.float32)
    gx, gy = U.random_glt(rng, (6, 9), 5, 7, p_nodata=0.3)
    gx[0, 0], gy[0, 0] = 0, 3
    sgx = gx * rng.choice([-1, 1], size=gx.shape).astype(np.int32)
    want = np.full(gx.shape, -9999.0, dtype=np.float32)
    for i in range(6):
        for j in range(9):
            if gx[i, j] != 0 and gy[i, j] != 0:
                want[i, j] = src[gy[i, j] - 1, gx[i, j] - 1]
    assert U.same_bytes(U.oracle(src, gx, gy, -9999.0), want)
    assert U.same_bytes(U.oracle(src, sgx, gy, -9999.0, absolute=True), want)
    sx, sy = U.swath_glt(40, 30, 70, 80)
    hit = (sx != 0)
    assert 0.2 < hit.mean() < 0.8 and sx.max() == 30 and sy.max() == 40 and np.array_equal(hit, sy != 0)
    distinct = np.unique(np.stack([sx[hit], sy[hit]]), axis=1).shape[1]
    assert 0.9 * 40 * 30 < distinct <= 40 * 30 < hit.sum()                     # most source pixels are hit, some repeatedly


def test_argument_errors_are_reported_before_any_launch():
    """sc_glt_ortho checks its arguments on the host and returns the library's ValueError code without touching a device"""
    from starcop_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    buf = np.zeros(64, np.int32)

    def args(**kw):
        a = _lib.sc_ortho_args()
        a.glt_x = a.glt_y = a.out = buf.ctypes.data
        a.out_h = a.out_w = 4
        a.rows = a.cols = 8
        a.P, a.elem_bytes = 1, 4
        a.src[0] = buf.ctypes.data
        a.row_stride[0], a.col_stride[0] = 8, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, word):
        rc = lib.sc_glt_ortho(a, None)
        assert rc == -1
        with pytest.raises(ValueError, match=word):
            _lib.check(rc)

    refused(None, "null arguments")
    for kw, word in (({"P": 0}, "P=0"), ({"P": 65}, "P=65"), ({"P": -1}, "P=-1"), ({"elem_bytes": 3}, "element width 3"),
                     ({"elem_bytes": 16}, "element width 16"), ({"out_h": 0}, "bad dims"), ({"cols": -2}, "bad dims"),
                     ({"glt_x": None}, "null pointer"), ({"out": None}, "null pointer"), ({"out": buf.ctypes.data + 2}, "misaligned")):
        refused(args(**kw), word)
    a = args()
    a.src[0] = None
    refused(a, "null source plane 0")
    a = args()
    a.src[0] = buf.ctypes.data + 2
    refused(a, "not aligned")
    a = args()
    a.row_stride[0] = -8
    refused(a, "negative stride")
    a = args()
    a.plane_cols[0] = 9
    refused(a, "outside the 8 x 8 swath")
    a = args(P=2)
    refused(a, "null source plane 1")
