"""The warp in the product paths: ``emit_granule_predict(..., georeferenced=True, crs=...)`` on the EMIT-like fixture granule and
``aviris_scene_predict(..., north_up=True)`` on a synthetic flight line whose ``map info`` is rotated.  Every warped product must be
``warp.reproject`` of the product the unchanged path gives, bit for bit; the defaults must leave that path as it is."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import plume_scene_util as P  # noqa: E402
from starcop_amd import io_formats as io, pipeline, plumes, warp  # noqa: E402
from test_gpu_plume_scene import _model  # noqa: E402  (the seeded 4-band model of the scene tests)

NC = os.path.join(os.path.dirname(__file__), "golden", "io", "emit_l1b_like_sb0.nc")
GT = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)      # the fixture carries no geotransform attribute
RES = 60.0


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def read_all(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


def test_emit_products_in_utm(hip, tmp_path):
    kw = dict(column_step=4, georeferenced=True, geotransform=GT, plumes=True, plume_outlines=True)
    # the seeded model of the scene tests, its head bias moved to minus the median logit of this granule: about half of the pixels are plume
    p = pipeline.emit_granule_predict(_model(0.0), NC, column_step=4)["prediction"].double().clamp(1e-6, 1 - 1e-6)
    model = _model(-float(torch.log(p / (1 - p)).median()))
    plain = pipeline.emit_granule_predict(model, NC, out_folder=str(tmp_path / "plain"), **kw)
    again = pipeline.emit_granule_predict(model, NC, out_folder=str(tmp_path / "again"), crs=None, **kw)
    first = read_all(str(tmp_path / "plain"))
    assert first == read_all(str(tmp_path / "again")) and {"mag1c.tif", "pred.tif", "predbinary.tif", "plumes.csv"} <= set(first)
    assert "geotransform" not in plain and "crs" not in plain and "ime_ppmm_m2" not in plain["plumes"].columns
    fill = plain["fill_value"]

    folder = str(tmp_path / "utm")
    out = pipeline.emit_granule_predict(model, NC, out_folder=folder, crs="utm", resolution=RES, **kw)
    h, w = plain["mf"].shape
    crs = warp.utm_crs_for(GT[0] + GT[1] * w / 2, GT[3] + GT[5] * h / 2)
    assert out["crs"] == crs == 32612
    shape, gt = warp.suggest_grid((h, w), GT, 4326, crs, RES)
    assert tuple(out["geotransform"]) == gt and gt[1] == RES and gt[5] == -RES
    # every product is reproject of the crs=None run's product
    for key in ("mf", "albedo", "prediction", "rgb", "pred_binary"):
        want = warp.reproject(plain[key], GT, 4326, gt, crs, shape, nodata=0 if key == "pred_binary" else fill)
        assert tuple(out[key].shape[-2:]) == shape and same_bits(out[key], want), key
        assert same_bits(out[key + "_raw"], plain[key + "_raw"]) if key != "rgb" else True
    assert 0 < int((out["mf"] != fill).sum()) < out["mf"].numel()          # the rotated footprint leaves fill at the corners
    # the files: UTM geo keys, one shape
    for name, key in (("pred.tif", "prediction"), ("predbinary.tif", "pred_binary"), ("mag1c.tif", "mf"), ("rgb.tif", "rgb")):
        info = io.tiff_info(os.path.join(folder, name))
        assert io.geo_from_tags(info) == (gt, crs) and (info.height, info.width) == shape, name
        assert info.tags[34735][1] == (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, crs)
        back = io.read_tiff(os.path.join(folder, name), info=info)
        want = out[key].cpu().numpy()
        want = (want if want.ndim == 3 else want[None]).astype(back.dtype)
        assert np.array_equal(back.view(np.uint8), want.view(np.uint8)), name
    # metric plume table
    table = out["plumes"]
    assert len(table) >= 1 and {"x", "y", "ime_ppmm_m2", "mag1c_sum"} <= set(table.columns)
    assert np.array_equal(table["ime_ppmm_m2"].to_numpy(), table["mag1c_sum"].to_numpy() * RES * RES)
    assert (table["x"] > gt[0]).all() and (table["x"] < gt[0] + RES * shape[1]).all() and (table["y"] < gt[3]).all()
    assert "ime_ppmm_m2" in open(os.path.join(folder, "plumes.csv")).readline()
    # bilinear for the float products, nearest for the mask
    smooth = pipeline.emit_granule_predict(model, NC, crs=crs, resolution=RES, resampling={"mf": "bilinear"}, **kw)
    assert same_bits(smooth["mf"], warp.reproject(plain["mf"], GT, 4326, gt, crs, shape, "bilinear", fill))
    assert same_bits(smooth["albedo"], out["albedo"]) and same_bits(smooth["pred_binary"], out["pred_binary"])
    # label polygons in another CRS
    x0, y0 = GT[0] + 20 * GT[1], GT[3] - 15 * GT[1]
    square = [[np.array([[x0, y0], [x0 + 30 * GT[1], y0], [x0 + 30 * GT[1], y0 - 25 * GT[1]], [x0, y0 - 25 * GT[1]], [x0, y0]])]]
    a = pipeline.emit_granule_predict(model, NC, crs=crs, resolution=RES, label_polygons=square, label_crs=4326, **kw)
    b = pipeline.emit_granule_predict(model, NC, crs=crs, resolution=RES, label_polygons=warp.transform_polygons(square, 4326, crs), **kw)
    assert a["label_mask"].dtype == torch.uint8 and 0 < int(a["label_mask"].sum()) < a["label_mask"].numel()
    assert torch.equal(a["label_mask"], b["label_mask"]) and tuple(a["label_mask"].shape) == shape
    with pytest.raises(ValueError, match="georeferenced"):
        pipeline.emit_granule_predict(model, NC, column_step=4, crs="utm")
    with pytest.raises(ValueError, match="geotransform"):
        pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, crs="utm")
    with pytest.raises(NotImplementedError, match="3857"):
        pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, geotransform=GT, crs=3857)


ROTATED = "{UTM, 1, 1, 500000.0, 4100000.0, 5.0, 5.0, 11, North, WGS-84, units=Meters, rotation=-12.0}"


def test_aviris_rotated_line_north_up(hip, tmp_path):
    """a 70 x 100 ENVI flight line with ``rotation=`` in its map info and a mag1c.tif beside it"""
    H, W = 70, 100
    model = _model(bias=-0.93)
    wl = np.array([440.0, 461.0, 500.0, 549.0, 600.0, 641.0, 700.0])
    valid = P.strip_mask(H, W, centre=30.0, slope=0.3, half_width=25.0)
    rng = np.random.default_rng(61)
    cube = rng.uniform(0.5, 12.0, size=(H, W, wl.size)).astype(np.float32)
    cube[~valid] = P.FILL
    mf = (600.0 * rng.standard_normal((H, W)) + 200.0).astype(np.float32)
    mf[~valid] = P.FILL
    folder = P.write_flight_line(str(tmp_path / "ang20190101t180000_rdn"), cube, wl, map_info=ROTATED)
    io.write_tiff(os.path.join(folder, "mag1c.tif"), mf, blocksize=128, extra_tags={42113: (2, ("-9999",))})
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32, plumes=True, plume_outlines=True)
    # as today: no coordinates for a rotated line, and the flag's default changes nothing
    old = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "old"), **kw)
    same = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "same"), north_up=False, **kw)
    assert "x" not in old["plumes"].columns and "geotransform" not in old and tuple(old["pred_binary"].shape) == (H, W)
    assert read_all(str(tmp_path / "old")) == read_all(str(tmp_path / "same"))
    assert 34264 in io.tiff_info(str(tmp_path / "old" / "pred.tif")).tags

    out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "up"), north_up=True, **kw)
    header = io.read_envi_header(os.path.join(folder, os.path.basename(folder) + "_img.hdr"))
    src_gt, epsg, rot = io.envi_geotransform(header)
    assert epsg == 32611 and rot == -12.0
    shape, gt = warp.suggest_grid((H, W), src_gt, epsg, epsg, 5.0)
    assert tuple(out["geotransform"]) == gt and out["crs"] == epsg and gt[2] == gt[4] == 0.0
    for key, nod in (("prediction", P.FILL), ("pred_binary", 0), ("mf", P.FILL)):
        assert same_bits(out[key], warp.reproject(old[key], src_gt, epsg, gt, epsg, shape, nodata=nod)), key
    mask = out["pred_binary"]
    assert 0 < int(mask.sum()) and abs(int(mask.sum()) - int(old["pred_binary"].sum())) <= 0.1 * int(mask.sum())      # same pixel size
    table = out["plumes"]
    assert len(table) >= 1 and {"x", "y", "ime_ppmm_m2"} <= set(table.columns)
    assert np.array_equal(table["ime_ppmm_m2"].to_numpy(), table["mag1c_sum"].to_numpy() * 25.0)
    # burning the outlines back on the new grid reproduces the warped mask
    burnt = plumes.rasterize_polygons(out["plume_outlines"], shape, geotransform=gt)
    assert torch.equal(burnt != 0, mask != 0)
    for name in ("pred.tif", "predbinary.tif"):
        info = io.tiff_info(str(tmp_path / "up" / name))
        assert io.geo_from_tags(info) == (gt, epsg) and (info.height, info.width) == shape and 33550 in info.tags
    assert os.path.exists(str(tmp_path / "up" / "plumes.geojson"))
    # label polygons in map coordinates can be burnt now
    ring = np.array([[gt[0] + 100.0, gt[3] - 100.0], [gt[0] + 300.0, gt[3] - 100.0], [gt[0] + 300.0, gt[3] - 250.0], [gt[0] + 100.0, gt[3] - 100.0]])
    lab = pipeline.aviris_scene_predict(model, folder, north_up=True, label_polygons=[[ring]], **kw)
    assert tuple(lab["label_mask"].shape) == shape and 0 < int(lab["label_mask"].sum())
    # a line without rotation is left as it is
    plain_folder = P.write_flight_line(str(tmp_path / "p" / "ang20190101t180000_rdn"), cube, wl)
    io.write_tiff(os.path.join(plain_folder, "mag1c.tif"), mf, blocksize=128, extra_tags={42113: (2, ("-9999",))})
    a = pipeline.aviris_scene_predict(model, plain_folder, str(tmp_path / "pa"), north_up=True, **kw)
    b = pipeline.aviris_scene_predict(model, plain_folder, str(tmp_path / "pb"), **kw)
    assert "geotransform" not in a and read_all(str(tmp_path / "pa")) == read_all(str(tmp_path / "pb"))
