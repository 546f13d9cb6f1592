"""sc_component_outlines / starcop_amd.plumes.component_outlines, plume_outlines and the plumes.geojson of the scene path against
the sequential restatement of tests/outlines_util.py.  Every comparison is exact: the operator is integer arithmetic.

Bernoulli masks: numpy default_rng with the seeds of outlines_util.SEEDS (p = 0.3: 301, 0.5: 502, 0.62: 623, 0.8: 804), 130258 for
the 130 x 258 image and 71 / 72 for the batch."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import outlines_util as U  # noqa: E402
from starcop_amd import _lib, plumes  # noqa: E402

DEV = "cuda"
FIELDS = plumes.OUTLINE_FIELDS
DTYPES = {"vertices": torch.int32, "ring_offsets": torch.int64, "ring_label": torch.int32, "ring_area2": torch.int64}
MASKS = U.all_small_masks()
GT = (500000.0, 5.0, 0.0, 4100000.0, 0.0, -5.0)


def _check(got, want, what):
    for f in FIELDS:
        assert got[f].is_cuda and got[f].dtype == DTYPES[f], (what, f, got[f].dtype)
        assert torch.equal(got[f].cpu(), torch.from_numpy(want[f])), (what, f)


def _both(lab, n, connectivity, what):
    """collinear=True and False against the restatement, and a second call against the first"""
    d_lab = torch.from_numpy(lab).to(DEV)
    stats = None
    for collinear in (True, False):
        want = U.outlines_ref(lab, connectivity, collinear)
        got = plumes.component_outlines(d_lab, n, connectivity=connectivity, collinear=collinear)
        _check(got, want, (what, connectivity, collinear))
        again = plumes.component_outlines(d_lab, n, connectivity=connectivity, collinear=collinear)
        for f in FIELDS:
            assert torch.equal(got[f], again[f]), (what, f, "two calls differ")
        stats = want
    return stats


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_component_outlines_small(hip, name, connectivity):
    lab, n = U.label(MASKS[name], connectivity)
    want = _both(lab, n, connectivity, name)
    if name == "empty":
        got = plumes.component_outlines(torch.from_numpy(lab).to(DEV), 0)
        assert got["vertices"].shape == (0, 2) and got["ring_offsets"].tolist() == [0] and got["ring_label"].numel() == 0
    if name == "spiral":
        assert want["longest"] == 1156 and hip.sc_component_outlines_rounds(want["n_edges"]) > 10


def test_component_outlines_large(hip):
    """130 x 258 at p = 0.62, connectivity 1: ragged against 64, 128 and 256, rings longer than the 256 edges of a work-group"""
    lab, n = U.label(U.bernoulli((130, 258), 0.62, U.SEED_LARGE), 1)
    want = _both(lab, n, 1, "large")
    assert want["longest"] > 256 and want["n_edges"] > 20000


def test_component_outlines_batch(hip):
    masks = np.stack([U.bernoulli((37, 70), 0.5, s) for s in U.SEED_BATCH])
    labs, counts = zip(*(U.label(m, 2) for m in masks))
    d_lab = torch.from_numpy(np.stack(labs)).to(DEV)
    got = plumes.component_outlines(d_lab, torch.tensor(counts, dtype=torch.int32, device=DEV))
    assert isinstance(got, list) and len(got) == 2
    for n in range(2):
        alone = plumes.component_outlines(d_lab[n], counts[n])
        _check(got[n], U.outlines_ref(labs[n], 2), ("batch", n))
        for f in FIELDS:
            assert torch.equal(got[n][f], alone[f]), (n, f)
    with pytest.raises(ValueError):
        plumes.component_outlines(d_lab, torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        plumes.component_outlines(d_lab, connectivity=3)


def _same_polygons(got, want):
    assert sorted(got) == sorted(want)
    for key in want:
        assert len(got[key]) == len(want[key]), key
        for a, b in zip(got[key], want[key]):
            assert a.dtype == np.float64 and np.array_equal(a, b), key


@pytest.mark.parametrize("connectivity", [1, 2])
def test_plume_outlines(hip, connectivity):
    mask = U.bernoulli((37, 70), 0.5, U.SEEDS[0.5])
    lab, n = U.label(mask, connectivity)
    ref = U.outlines_ref(lab, connectivity)
    want = plumes.polygons_from_rings(*(ref[f] for f in FIELDS), geotransform=GT)
    _same_polygons(plumes.plume_outlines(mask.astype(np.uint8), connectivity=connectivity, geotransform=GT), want)
    _same_polygons(plumes.plume_outlines(torch.from_numpy(mask).to(DEV), connectivity=connectivity),
                   plumes.polygons_from_rings(*(ref[f] for f in FIELDS)))
    # a batch: items keyed by their index
    both = plumes.plume_outlines(np.stack([mask, mask[::-1]]).astype(np.uint8), connectivity=connectivity, geotransform=GT)
    _same_polygons({k: v for k, v in both.items() if k[0] == 0}, want)
    lab1, _ = U.label(mask[::-1], connectivity)
    ref1 = U.outlines_ref(lab1, connectivity)
    _same_polygons({k: v for k, v in both.items() if k[0] == 1},
                   plumes.polygons_from_rings(*(ref1[f] for f in FIELDS), geotransform=GT, item=1))
    with pytest.raises(NotImplementedError):
        plumes.plume_outlines(mask.astype(np.uint8), geotransform=(0.0, 1.0, 0.5, 0.0, 0.0, -1.0))


@pytest.mark.parametrize("connectivity", [1, 2])
def test_plume_outlines_min_area_and_areas(hip, connectivity):
    mask = U.bernoulli((37, 70), 0.3, U.SEEDS[0.3]).astype(np.uint8)
    table = plumes.plume_table(mask, connectivity=connectivity)
    big = plumes.plume_table(mask, connectivity=connectivity, min_area=5)
    assert 0 < len(big) < len(table)
    polys = plumes.plume_outlines(mask, connectivity=connectivity)
    assert sorted(polys) == [(int(i), int(k)) for i, k in zip(table["item"], table["plume_id"])]
    for key, area in zip(sorted(polys), table["area_px"]):
        a2 = [plumes._shoelace(r) for r in polys[key]]
        assert a2[0] > 0 and all(v < 0 for v in a2[1:]) and sum(a2) == 2 * int(area), key                # exterior minus holes
    kept = plumes.plume_outlines(mask, connectivity=connectivity, min_area=5)
    assert sorted(kept) == [(int(i), int(k)) for i, k in zip(big["item"], big["plume_id"])]


def test_outline_refusals(hip):
    a = _lib.sc_outline_args()
    lab = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    a.labels, a.H, a.W, a.connectivity = lab.data_ptr(), 1 << 15, 1 << 14, 2
    assert hip.sc_component_outlines(a, _lib.OUTLINE_COUNT, _lib.stream()) == -1 and b"4*H*W" in hip.sc_last_error()
    a.H, a.W, a.E = 4, 4, 8                                       # TRACE without a workspace
    assert hip.sc_component_outlines(a, _lib.OUTLINE_TRACE, _lib.stream()) == -1 and b"workspace" in hip.sc_last_error()
    assert hip.sc_component_outlines(a, 7, _lib.stream()) == -1
    torch.cuda.synchronize()


def test_emit_granule_predict_outlines(hip, tmp_path):
    """the EMIT fixture granule, orthorectified: plumes.geojson holds the outline of every row of the table"""
    from starcop_amd import model_module as mm, pipeline
    nc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "io", "emit_l1b_like_sb0.nc")
    gt = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1)).to(DEV).eval()
    out = pipeline.emit_granule_predict(model, nc, column_step=4, georeferenced=True, out_folder=str(tmp_path / "o"), geotransform=gt,
                                        plumes=True, plume_outlines=True)
    assert [os.path.basename(p) for p in out["files"]][-2:] == ["plumes.csv", "plumes.geojson"]
    lab, n = U.label(out["pred_binary"].cpu().numpy(), 2)
    ref = U.outlines_ref(lab, 2)
    want = plumes.polygons_from_rings(*(ref[f] for f in FIELDS), geotransform=gt)
    _same_polygons(out["plume_outlines"], want)
    feats = json.load(open(str(tmp_path / "o" / "plumes.geojson")))["features"]
    assert len(feats) == len(out["plumes"]) == n >= 1 and all(f["geometry"]["type"] == "Polygon" for f in feats)
    with pytest.raises(ValueError):
        pipeline.emit_granule_predict(model, nc, column_step=4, plume_outlines=True)


def test_aviris_scene_predict_outlines(hip, tmp_path):
    """the 70 x 100 flight line of the scene tests: plumes.geojson holds one Polygon per row of plumes.csv, each the outline of that
    plume of predbinary; without the flag no such file is written"""
    import plume_scene_util as S
    from starcop_amd import io_formats, pipeline
    from test_gpu_plume_scene import _model
    H, W = 70, 100
    model = _model(bias=-0.93)
    wl = np.array([440.0, 461.0, 500.0, 549.0, 600.0, 641.0, 700.0])
    valid = S.strip_mask(H, W, centre=30.0, slope=0.3, half_width=25.0)
    rng = np.random.default_rng(61)
    cube = rng.uniform(0.5, 12.0, size=(H, W, wl.size)).astype(np.float32)
    cube[~valid] = S.FILL
    mf = (600.0 * rng.standard_normal((H, W)) + 200.0).astype(np.float32)
    mf[~valid] = S.FILL
    folder = S.write_flight_line(str(tmp_path / "ang20190101t180000_rdn"), cube, wl)
    io_formats.write_tiff(os.path.join(folder, "mag1c.tif"), mf, blocksize=128, extra_tags={42113: (2, ("-9999",))})
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32)
    out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "a"), plumes=True, plume_outlines=True, **kw)
    assert sorted(os.path.basename(p) for p in out["files"]) == ["plumes.csv", "plumes.geojson", "pred.tif", "predbinary.tif"]
    rows = open(str(tmp_path / "a" / "plumes.csv")).read().strip().split("\n")[1:]
    feats = json.load(open(str(tmp_path / "a" / "plumes.geojson")))["features"]
    assert len(feats) == len(rows) == len(out["plumes"]) >= 1
    mask = out["pred_binary"].cpu().numpy()
    lab, n = U.label(mask, 2)
    ref = U.outlines_ref(lab, 2)
    want = plumes.polygons_from_rings(*(ref[f] for f in FIELDS), geotransform=GT)
    _same_polygons(out["plume_outlines"], want)
    for f, k in zip(feats, out["plumes"]["plume_id"]):
        assert f["geometry"]["type"] == "Polygon" and f["properties"]["plume_id"] == int(k)
        rings = f["geometry"]["coordinates"]
        assert len(rings) == len(want[(0, int(k))])
        assert np.array_equal(np.array(rings[0]), want[(0, int(k))][0][::-1])                             # north up: reversed
    # the overwrite rule holds for the new file; without the flag it is not written
    again = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "a"), plumes=True, plume_outlines=True, **kw)
    assert again["files"] == []
    plain = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "b"), plumes=True, **kw)
    assert "plume_outlines" not in plain and sorted(os.listdir(str(tmp_path / "b"))) == ["plumes.csv", "pred.tif", "predbinary.tif"]
    with pytest.raises(ValueError):
        pipeline.aviris_scene_predict(model, folder, plume_outlines=True, **kw)
