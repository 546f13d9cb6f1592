"""products.plan_rasters / write_rasters without a device: the tags of every file of the EMIT and AVIRIS tables restated file by
file, and the rules for which files a run writes."""
import os
import warnings

import numpy as np
import pytest

import plume_scene_util as S
from starcop_amd import io_formats as io, ortho, products

GT = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)
WKT = 'GEOGCS["WGS 84",DATUM["WGS_1984",SPHEROID["WGS 84",6378137,298.257223563]],PRIMEM["Greenwich",0],UNIT["degree",0.0174532925199433]]'
WL = np.array([2130.0, 2137.5])
NODATA = {42113: (2, ("-9999",))}
WARNING = "emit_granule_predict: no geotransform"


def _emit_plan(folder, overwrite=False, geotransform=GT):
    geo = ortho.emit_geo_tags(geotransform, WKT) if geotransform is not None else {}
    return products.plan_rasters(products.EMIT_RASTERS, str(folder), overwrite, geo, -9999.0, {"wavelengths": WL, "mag1c": "acrwl1mf"},
                                 no_geo_warning=WARNING)


def _same_tags(got, want):
    """equal, and laid out in the same order (the order of the tags decides where their values lie in the file)"""
    return got == want and list(got) == list(want)


def test_emit_plan_tags_file_by_file(tmp_path):
    geo = ortho.emit_geo_tags(GT, WKT)
    md = {"wavelengths": WL, "mag1c": "acrwl1mf"}
    rgb = ["Red (640 nm)", "Green (550 nm)", "Blue (460 nm)"]
    want = [("mag1c.tif", "mf", {**geo, **NODATA, **io.gdal_metadata_tag(md, ["CH4 Absorption (ppm x m)"])}, -9999.0),
            ("albedo.tif", "albedo", {**geo, **NODATA, **io.gdal_metadata_tag(md, ["Albedo"])}, -9999.0),
            ("pred.tif", "prediction", {**geo, **NODATA, **io.gdal_metadata_tag({}, ["Plume probability"])}, -9999.0),
            ("predbinary.tif", "pred_binary", {**geo, **io.gdal_metadata_tag({}, ["Plume mask"])}, None),
            ("rgb.tif", "rgb", {**geo, **NODATA, **io.gdal_metadata_tag({}, rgb)}, -9999.0)]
    plan = _emit_plan(tmp_path / "out")
    assert len(plan) == 5 and set(geo) == {33550, 33922, 34735}
    for (path, key, tags, nodata), (name, wkey, wtags, wnodata) in zip(plan, want):
        assert path == str(tmp_path / "out" / name) and key == wkey and nodata == wnodata, name
        assert _same_tags(tags, wtags), name
        xml = tags[42112][1][0]
        assert ('<Item name="mag1c">acrwl1mf</Item>' in xml) == ("2130.0" in xml) == (name in ("mag1c.tif", "albedo.tif")), name
        assert (42113 in tags) == (name != "predbinary.tif")
    assert [r.name for r in products.EMIT_RASTERS if r.uint8] == ["predbinary.tif"]
    # the fill value of the file keeps its formatter
    odd = products.plan_rasters(products.EMIT_RASTERS, str(tmp_path), True, geo, -3.4028234663852886e+38, md)
    assert odd[0][2][42113] == (2, (f"{-3.4028234663852886e+38:.9g}",)) and odd[0][3] == -3.4028234663852886e+38


def test_aviris_plan_tags_file_by_file(tmp_path):
    cube = np.ones((4, 5, 3), dtype=np.float32)
    folder = S.write_flight_line(str(tmp_path / "ang20190101t180000_rdn"), cube, [460.0, 550.0, 640.0])
    geo = io.envi_geo_tags(io.read_envi_header(os.path.join(folder, "ang20190101t180000_rdn_img.hdr")))
    assert set(geo) == {33550, 33922, 34735}
    out = str(tmp_path / "out")
    plan = products.plan_rasters(products.AVIRIS_RASTERS, out, False, geo, -9999)
    assert [(p, k, n) for p, k, _, n in plan] == [(os.path.join(out, "pred.tif"), "prediction", -9999),
                                                  (os.path.join(out, "predbinary.tif"), "pred_binary", None)]
    assert _same_tags(plan[0][2], {**geo, **NODATA, **io.gdal_metadata_tag({}, ["Plume probability"])})
    assert _same_tags(plan[1][2], {**geo, **io.gdal_metadata_tag({}, ["Plume mask"])})
    assert [r.uint8 for r in products.AVIRIS_RASTERS] == [False, True]
    # label.tif: like predbinary.tif
    (path, key, tags, nodata), = products.plan_rasters((products.LABEL,), out, False, geo)
    assert (path, key, nodata) == (os.path.join(out, "label.tif"), "label_mask", None) and products.LABEL.uint8
    assert _same_tags(tags, {**geo, **io.gdal_metadata_tag({}, ["Plume label"])})
    # the mag1c.tif a flight line run computes, and the same row under the file names aviris_scene_mag1c is given
    md = {"wavelengths": np.array([2130.0, 2135.0]), "mag1c": "acfwl1mf"}
    (path, key, tags, nodata), = products.plan_rasters((products.MAG1C,), out, False, geo, -9999, md)
    assert (path, key, nodata) == (os.path.join(out, "mag1c.tif"), "mf", -9999)
    want = {**geo, **NODATA, **io.gdal_metadata_tag(md, ["CH4 Absorption (ppm x m)"])}
    assert _same_tags(tags, want) and '<Item name="mag1c">acfwl1mf</Item>' in tags[42112][1][0]
    assert _same_tags(products.raster_tags(products.MAG1C, geo, -9999, md, None), want)
    extra = {270: (2, ("a note",))}
    assert _same_tags(products.raster_tags(products.ALBEDO, geo, -9999, md, extra), {**geo, **NODATA, **extra, **io.gdal_metadata_tag(md, ["Albedo"])})


def test_skip_rules(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    for name in ("albedo.tif", "predbinary.tif"):
        (out / name).write_bytes(b"kept")
    assert [os.path.basename(p[0]) for p in _emit_plan(out)] == ["mag1c.tif", "pred.tif", "rgb.tif"]
    assert [os.path.basename(p[0]) for p in _emit_plan(out, overwrite=True)] == ["mag1c.tif", "albedo.tif", "pred.tif", "predbinary.tif", "rgb.tif"]
    for name in ("mag1c.tif", "pred.tif", "rgb.tif"):
        (out / name).write_bytes(b"kept")
    assert _emit_plan(out) == []
    assert sorted(os.listdir(str(out))) == ["albedo.tif", "mag1c.tif", "pred.tif", "predbinary.tif", "rgb.tif"]
    # nothing to write: the folder is not made, and no image is looked at
    missing = tmp_path / "not" / "there"
    assert products.write_rasters({}, (), str(missing)) == [] and not missing.exists() and not (tmp_path / "not").exists()


def test_write_rasters_on_host_arrays_and_tensors(tmp_path):
    """the plain path needs no device: files in table order, uint8 where the row says so, the folder made on demand"""
    import torch
    rng = np.random.default_rng(3)
    out = {"prediction": torch.from_numpy(rng.random((9, 7)).astype(np.float32)), "pred_binary": torch.from_numpy(rng.integers(0, 2, (9, 7)))}
    assert out["pred_binary"].dtype == torch.int64
    folder = tmp_path / "a" / "b"
    files = products.write_rasters(out, products.AVIRIS_RASTERS, str(folder), geo_tags={}, nodata=-9999)
    assert files == [str(folder / "pred.tif"), str(folder / "predbinary.tif")]
    back = io.read_tiff(files[1])
    assert back.dtype == np.uint8 and np.array_equal(back[0], out["pred_binary"].numpy())
    assert np.array_equal(io.read_tiff(files[0])[0], out["prediction"].numpy()) and io.tiff_info(files[0]).tags[42113][1] == ("-9999",)
    assert products.write_rasters(out, products.AVIRIS_RASTERS, str(folder), geo_tags={}, nodata=-9999) == []
    products.write_raster(str(folder / "n.tif"), out["prediction"].numpy(), {})
    assert open(str(folder / "n.tif"), "rb").read() != b"" and np.array_equal(io.read_tiff(str(folder / "n.tif"))[0], out["prediction"].numpy())


def test_no_geotransform_warns_once_and_only_when_writing(tmp_path):
    out = tmp_path / "out"
    with pytest.warns(UserWarning, match=WARNING) as rec:
        plan = _emit_plan(out, geotransform=None)
    assert len(rec) == 1 and len(plan) == 5 and all(set(tags) <= {42112, 42113} for _, _, tags, _ in plan)
    out.mkdir()
    for row in products.EMIT_RASTERS:
        (out / row.name).write_bytes(b"kept")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert _emit_plan(out, geotransform=None) == []
    assert rec == []
    with warnings.catch_warnings(record=True) as rec:            # georeferenced: nothing to warn about
        warnings.simplefilter("always")
        assert len(_emit_plan(out, overwrite=True)) == 5
    assert rec == []
