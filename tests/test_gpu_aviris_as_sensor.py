"""pipeline.aviris_as_sensor (starcop/process_aviris.py:26-90) end to end on the GPU: a synthetic AVIRIS-NG ENVI folder ->
34 WV3 / S2A / S2B GeoTIFFs, read back bit-equal to the numpy restatement of transform_to_srf (tests/srf_util.py)."""
import os

import numpy as np
import pytest
import torch

import srf_util as U

pytestmark = pytest.mark.gpu

NL, NS = 300, 96
MAP_INFO = "{UTM, 1, 1, 500000.0, 4100000.0, 5.0, 5.0, 11, North, WGS-84, units=Meters, rotation=-12.0}"


def _write_envi(folder, cube, interleave="bip", fill=-9999.0):
    """cube (lines, samples, bands) float32 -> {folder}/{name}_img + .hdr"""
    os.makedirs(folder, exist_ok=True)
    name = os.path.basename(folder)
    wl = U.g3_grid()
    raw = {"bip": cube, "bil": cube.transpose(0, 2, 1), "bsq": cube.transpose(2, 0, 1)}[interleave]
    np.ascontiguousarray(raw).tofile(os.path.join(folder, f"{name}_img"))
    extra = f"data ignore value = {fill:g}\n" if fill is not None else ""
    with open(os.path.join(folder, f"{name}_img.hdr"), "w") as f:
        f.write(f"ENVI\nsamples = {cube.shape[1]}\nlines = {cube.shape[0]}\nbands = {cube.shape[2]}\nheader offset = 0\ndata type = 4\n"
                f"interleave = {interleave}\nbyte order = 0\nmap info = {MAP_INFO}\nwavelength units = Nanometers\n"
                f"wavelength = {{ {', '.join(f'{v:.4f}' for v in wl)} }}\nfwhm = {{ {', '.join('5.5' for _ in wl)} }}\n{extra}")
    return str(folder)


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(21)
    cube = rng.uniform(0.0, 20.0, size=(NL, NS, 425)).astype(np.float32)
    cube[rng.random(cube.shape) < 5e-4] = -9999.0
    cube[:4, :10] = -9999.0                                        # a no-data corner
    return cube


@pytest.fixture()
def srf_cache(monkeypatch):
    from starcop_amd import aviris
    monkeypatch.setattr(aviris, "SRF_WV3", U.drop_zero_rows(U.wv3_table()))
    monkeypatch.setattr(aviris, "SRF_S2", U.drop_zero_rows(U.s2_table()))


def _want(cube, fill):
    wl = U.g3_grid()
    out = {}
    for sensor, (bands, srf) in U.all_sensor_weights().items():
        res = U.oracle_transform(cube.transpose(2, 0, 1), bands, srf, wl, fill)
        out.update({f"{sensor}_{b}": r for b, r in zip(bands, res)})
    return out


def _read_all(folder):
    from starcop_amd import io_formats as io
    return {f[:-4]: io.read_tiff(os.path.join(folder, f)) for f in sorted(os.listdir(folder)) if f.endswith(".tif")}


def test_envi_folder_to_34_tiffs(hip, tmp_path, scene, srf_cache):
    from starcop_amd import features, io_formats as io, pipeline
    src = _write_envi(str(tmp_path / "ang20200101t000000_rdn_v2"), scene)
    dst = str(tmp_path / "out")
    written = pipeline.aviris_as_sensor(src, dst)
    assert len(written) == 34 and len(os.listdir(dst)) == 34
    want = _want(scene, -9999.0)
    got = _read_all(dst)
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].shape == (1, NL, NS) and got[k].dtype == np.float32
        assert np.array_equal(got[k][0].view(np.uint32), v.view(np.uint32)), k
    hdr = io.read_envi_header(os.path.join(src, os.path.basename(src) + "_img.hdr"))
    geo = io.envi_geo_tags(hdr)
    for k in ("WV3_SWIR1", "S2A_B8A", "S2B_B12"):
        info = io.tiff_info(os.path.join(dst, f"{k}.tif"))
        assert info.block == (128, 128) and info.tags[42113][1][0] == "-9999"
        for t, v in geo.items():
            assert info.tags[t] == v, (k, t)
        assert f'role="description">{k.split("_", 1)[1]}</Item>' in info.tags[42112][1][0]
    assert (got["WV3_SWIR1"][0, :4, :10] == -9999).all()

    # chunks of 37 lines give the same bytes as one chunk; a BSQ copy of the file gives the same outputs
    for kw, cube_src in (({"lines_per_chunk": 37}, src),
                         ({}, _write_envi(str(tmp_path / "bsq" / "ang20200101t000000_rdn_v2"), scene, "bsq")),
                         ({"lines_per_chunk": 64}, _write_envi(str(tmp_path / "bil" / "ang20200101t000000_rdn_v2"), scene, "bil"))):
        d2 = str(tmp_path / f"out_{len(os.listdir(tmp_path))}")
        pipeline.aviris_as_sensor(cube_src, d2, **kw)
        for k in want:
            with open(os.path.join(dst, f"{k}.tif"), "rb") as a, open(os.path.join(d2, f"{k}.tif"), "rb") as b:
                assert a.read() == b.read(), (kw, cube_src, k)

    # an existing output keeps its bytes and mtime; only the missing files are written
    keep = os.path.join(dst, "WV3_SWIR3.tif")
    st = os.stat(keep)
    blob = open(keep, "rb").read()
    os.remove(os.path.join(dst, "S2B_B11.tif"))
    os.remove(os.path.join(dst, "WV3_SWIR8.tif"))
    again = pipeline.aviris_as_sensor(src, dst)
    assert sorted(os.path.basename(p) for p in again) == ["S2B_B11.tif", "WV3_SWIR8.tif"]
    assert os.stat(keep).st_mtime_ns == st.st_mtime_ns and open(keep, "rb").read() == blob
    assert np.array_equal(io.read_tiff(os.path.join(dst, "WV3_SWIR8.tif"))[0].view(np.uint32), want["WV3_SWIR8"].view(np.uint32))
    assert pipeline.aviris_as_sensor(src, dst) == []

    # the WV3 outputs feed the Sanchez-Garcia MLR ratio
    wv3 = [torch.from_numpy(io.read_tiff(os.path.join(dst, f"WV3_SWIR{i}.tif"))[0]).cuda() for i in range(1, 9)]
    r = features.ratio_MLR_local_5IN(*[wv3[int(n[-1]) - 1] for n in features._WV3_MLR_IN], wv3[7])
    assert tuple(r.shape) == (NL, NS) and bool(torch.isfinite(r).all())


def test_header_without_fill_masks_nothing(hip, tmp_path, scene, srf_cache):
    from starcop_amd import io_formats as io, pipeline
    cube = scene[:40].copy()
    cube[10, 10] = 5.0
    cube[10, 10, 165] = -9999.0                                    # one -9999 inside the SWIR1 support (bands 162..171)
    src = _write_envi(str(tmp_path / "ang20200102t000000_rdn_v2"), cube, fill=None)
    dst = str(tmp_path / "out")
    written = pipeline.aviris_as_sensor(src, dst, sensors=["WV3", "S2A"])
    assert len(written) == 21
    want = _want(cube, None)
    got = _read_all(dst)
    for k, v in got.items():
        assert np.array_equal(v[0].view(np.uint32), want[k].view(np.uint32)), k
        assert 42113 not in io.tiff_info(os.path.join(dst, f"{k}.tif")).tags
    assert -9999.0 < got["WV3_SWIR1"][0, 10, 10] < 0.0                # an ordinary weighted sum, not masked
