"""sc_rasterize_polygons / starcop_amd.plumes.rasterize_polygons, match_plumes_polygons and the label_polygons of the scene paths.
Every comparison is exact: against the label image the outlines came from (rasterize(outlines(labels)) == labels ties the two
operators and scipy.ndimage.label together) and against the numpy float64 restatement of tests/rasterize_util.py, bit for bit.

Bernoulli masks: numpy default_rng with the seeds of outlines_util; the general polygons: rasterize_util.SEED_GENERAL."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import outlines_util as OU  # noqa: E402
import rasterize_util as R  # noqa: E402
from starcop_amd import _lib, io_formats, plumes  # noqa: E402

DEV = "cuda"
CASES = dict(R.bernoulli_cases())


def _equal(got, want, what=None):
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == tuple(want.shape), what
    assert torch.equal(got, torch.from_numpy(np.array(want)).to(DEV)), what


# ---- 1. round trip ----

@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_round_trip(hip, name, connectivity):
    mask = CASES[name]
    lab, n = OU.label(mask, connectivity)
    d_mask = torch.from_numpy(mask).to(DEV)
    polys = plumes.plume_outlines(d_mask, connectivity=connectivity, geotransform=R.GT)
    assert len(polys) == n
    _equal(plumes.rasterize_polygons(polys, lab.shape, geotransform=R.GT), lab, (name, "geotransform"))
    plain = plumes.plume_outlines(d_mask, connectivity=connectivity)
    _equal(plumes.rasterize_polygons(plain, lab.shape), lab, (name, "pixel coordinates"))


def test_round_trip_large(hip):
    """130 x 258 at p = 0.62, connectivity 1: the device result is the label image and the restatement's"""
    lab, n = OU.label(OU.bernoulli((130, 258), 0.62, OU.SEED_LARGE), 1)
    polys = plumes.plume_outlines(torch.from_numpy(lab).to(DEV), connectivity=1, geotransform=R.GT)
    keys = list(polys)
    assert len(keys) == n
    got = plumes.rasterize_polygons(polys, lab.shape, geotransform=R.GT)
    _equal(got, lab)
    _equal(got, R.raster_ref([R.to_pixel(polys[k], R.GT) for k in keys], [k[1] for k in keys], *lab.shape))


# ---- 2. general polygons, bit-equal ----

@pytest.mark.parametrize("shape", R.SHAPES_GENERAL)
def test_general_polygons(hip, shape):
    polys = R.general_polygons(shape)
    ref = R.general_ref(shape)
    assert len(set(ref.ravel().tolist())) > 5                               # several polygons show, none covers everything
    _equal(plumes.rasterize_polygons(polys, shape), ref)
    # every polygon on its own as well: nothing hides under a later one
    for i, rings in enumerate(polys):
        _equal(plumes.rasterize_polygons([rings], shape, values=[i + 1]), R.raster_ref([rings], [i + 1], *shape), i)


def test_tie_cases(hip):
    ties = R.tie_polygons()
    for name, rings in ties.items():
        want = R.raster_ref([rings], [1], 30, 50)
        assert want.any(), name
        _equal(plumes.rasterize_polygons([rings], (30, 50)), want, name)
    sq = np.zeros((30, 50), dtype=np.int32)
    sq[2:6, 2:6] = 1                                                        # rows 2..5, columns 2..5, not 6
    _equal(plumes.rasterize_polygons([ties["half_integer_square"]], (30, 50)), sq)


# ---- 3. order and values ----

def _square(c0, r0, c1, r1):
    return [np.array([(c0, r0), (c1, r0), (c1, r1), (c0, r1)], dtype=np.float64)]


def test_order_and_values(hip):
    a, b, other = _square(2, 2, 10, 10), _square(6, 6, 14, 14), _square(20, 3, 25, 8)
    tri = [np.array([(16.0, 12.0), (30.0, 12.0), (23.0, 19.0)])]
    for order in ([a, b, other, tri], [other, a, tri, b], [tri, other, a, b]):
        got = plumes.rasterize_polygons(order, (20, 32)).cpu().numpy()
        ia, ib = [x is a for x in order].index(True) + 1, [x is b for x in order].index(True) + 1
        assert ia < ib and (got[6:10, 6:10] == ib).all() and (got[2:6, 2:10] == ia).all() and (got[10:14, 6:14] == ib).all()
        _equal(plumes.rasterize_polygons(order, (20, 32)), R.raster_ref(order, range(1, 5), 20, 32))
    got = plumes.rasterize_polygons([b, a], (20, 32)).cpu().numpy()
    assert (got[6:10, 6:10] == 2).all() and (got[10:14, 10:14] == 1).all()  # the other way round: a is later and wins
    values = [-5, 7, 7, 2 ** 31 - 1]
    _equal(plumes.rasterize_polygons([a, b, other, tri], (20, 32), values=values), R.raster_ref([a, b, other, tri], values, 20, 32))
    _equal(plumes.rasterize_polygons([a, b], (20, 32), values=np.array([0, -2 ** 31])), R.raster_ref([a, b], [0, -2 ** 31], 20, 32))
    with pytest.raises(ValueError):
        plumes.rasterize_polygons([a, b], (20, 32), values=[1])
    with pytest.raises(ValueError):
        plumes.rasterize_polygons([a, b], (20, 32), values=[1.5, 2.0])


def test_dict_values_and_item(hip):
    d = {(0, 7): _square(1, 1, 5, 5), (1, 3): _square(0, 0, 8, 8), (0, 2): _square(3, 3, 9, 7), (1, 9): _square(6, 2, 8, 4)}
    want0 = R.raster_ref([d[(0, 7)], d[(0, 2)]], [7, 2], 8, 10)
    assert want0[3, 3] == 2 and want0[1, 1] == 7                            # dict order: plume 2 is later than plume 7
    _equal(plumes.rasterize_polygons(d, (8, 10)), want0)
    _equal(plumes.rasterize_polygons(d, (8, 10), item=1), R.raster_ref([d[(1, 3)], d[(1, 9)]], [3, 9], 8, 10))
    _equal(plumes.rasterize_polygons(d, (8, 10), item=1, values=[4, 4]), R.raster_ref([d[(1, 3)], d[(1, 9)]], [4, 4], 8, 10))
    assert not plumes.rasterize_polygons(d, (8, 10), item=2).any()


# ---- 4. no cap on crossings ----

def test_no_cap_on_crossings(hip):
    H, W = 8, 4100
    poly = R.comb(1000, W, H)
    x0, y0, x1, y1 = R.ring_edges(poly)
    for r in (1, 2, 3, 4):
        assert int(((y0 <= r + 0.5) != (y1 <= r + 0.5)).sum()) >= 2000
    want = R.raster_ref([poly], [1], H, W)
    assert W % 64 != 0 and 1000 < int(want[2].sum()) < W - 1000
    _equal(plumes.rasterize_polygons([poly], (H, W)), want)


def test_box_wider_than_the_bitmap(hip):
    """66000 columns: the box is burnt in two column chunks (65536 columns each); a hole across the chunk border, crossings in
    both chunks, a crossing left of the second chunk carried into it"""
    H, W = 3, 66000
    big = [np.array([(10.3, -1.0), (65990.7, -1.0), (65990.7, 2.2), (10.3, 2.2)]),
           np.array([(65500.4, 0.2), (65600.6, 0.2), (65580.1, 1.7), (65520.9, 1.7)])]
    tri = [np.array([(65530.0, -4.0), (65999.0, 0.9), (65700.5, 5.0)])]
    polys = [big, tri]
    want = R.raster_ref(polys, [1, 2], H, W)
    assert want[0, 65535] == 0 and want[0, 65537] == 0 and want[0, 65499] == 1 and (want[:, 65536:] == 2).any() and want[2, 12000] == 0
    _equal(plumes.rasterize_polygons(polys, (H, W)), want)


def test_more_jobs_than_the_grid(hip):
    """2^20 + 100 rows of one polygon: more (polygon, row) jobs than work-groups are launched, every row still burnt"""
    H, W = (1 << 20) + 100, 2
    want = np.zeros((H, W), dtype=np.int32)
    want[5:H - 7, 1] = 4                                                   # rows with 5 <= r + 0.5 < H - 7, the column with 1 <= 1.5 < 2
    _equal(plumes.rasterize_polygons([_square(1, 5, 2, H - 7)], (H, W), values=[4]), want)


# ---- 5. clipping and empties ----

def test_clipping_and_empties(hip):
    shape = (11, 13)
    outside = [np.array([(20.0, 20.0), (30.0, 20.0), (25.0, 40.0)])]
    left = [np.array([(-30.0, 2.0), (-3.0, 2.0), (-3.0, 9.0)])]
    around = [np.array([(-1e6, -1e6), (1e6, -1e6), (1e6, 1e6), (-1e6, 1e6)])]
    for p in (outside, left):
        got = plumes.rasterize_polygons([p], shape)
        assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == shape and not got.any()
    _equal(plumes.rasterize_polygons([around], shape, values=[3]), np.full(shape, 3, dtype=np.int32))
    _equal(plumes.rasterize_polygons([around, outside, None, left], shape), np.full(shape, 1, dtype=np.int32))
    for empty in ([], {}, [None]):
        got = plumes.rasterize_polygons(empty, shape)
        assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == shape and not got.any()
    # a frame around the raster with the raster in its hole: nothing; straddling the edge: clipped by rows and columns
    frame = [around[0], np.array([(-2.0, -2.0), (15.0, -2.0), (15.0, 13.0), (-2.0, 13.0)])]
    assert not plumes.rasterize_polygons([frame], shape).any()
    straddle = [np.array([(-4.3, -2.2), (6.4, 3.3), (17.9, -1.0), (9.2, 14.6), (-6.0, 8.1)])]
    _equal(plumes.rasterize_polygons([straddle], shape), R.raster_ref([straddle], [1], *shape))
    # 1 x 1
    _equal(plumes.rasterize_polygons([_square(0, 0, 1, 1)], (1, 1)), np.ones((1, 1), dtype=np.int32))
    _equal(plumes.rasterize_polygons([_square(0.5, 0.5, 3, 3)], (1, 1)), np.ones((1, 1), dtype=np.int32))      # the centre is top-left: in
    _equal(plumes.rasterize_polygons([_square(-3, -3, 0.5, 0.5)], (1, 1)), np.zeros((1, 1), dtype=np.int32))   # bottom-right: out


def test_refusals_before_any_launch(hip):
    ok = np.array([(1.0, 1.0), (5.0, 1.0), (5.0, 5.0)])
    bad = {"nan": ok.copy(), "inf": ok.copy(), "huge": ok.copy(), "two": ok[:2], "repeated": ok[[0, 1, 0, 1]]}
    bad["nan"][0, 0] = np.nan
    bad["inf"][1, 1] = np.inf
    bad["huge"][2, 0] = 2.0 ** 31
    for name, ring in bad.items():
        with pytest.raises(ValueError):
            plumes.rasterize_polygons([[ok], [ring]], (8, 8))
    with pytest.raises(ValueError):
        plumes.rasterize_polygons([[ok]], (1 << 16, 1 << 15))
    with pytest.raises(ValueError):
        plumes.rasterize_polygons([[ok * 1e9]], (8, 8), geotransform=(0.0, 0.25, 0.0, 0.0, 0.0, -0.25))          # 4e9 pixels away
    with pytest.raises(NotImplementedError):
        plumes.rasterize_polygons([[ok]], (8, 8), geotransform=(0.0, 1.0, 0.5, 0.0, 0.0, -1.0))
    # the entry point itself refuses a table that leaves the raster or the edge array, and an inconsistent job index
    out = torch.full((8, 8), -1, dtype=torch.int32, device=DEV)
    edges, table = plumes.polygon_edges([[ok]], (8, 8))
    for col, value, text in ((3, 9, b"leaves"), (1, 4, b"edges"), (6, 1, b"job0")):
        t = table.copy()
        t[0, col] = value
        ops = plumes.rasterize_upload(edges, t)
        with pytest.raises(ValueError):
            plumes.rasterize_launch(ops, (8, 8), out=out)
        assert text in hip.sc_last_error()
    ops = plumes.rasterize_upload(edges, table)
    ops["buffer"] = ops["buffer"][8:]                                       # edges that are not 16-byte aligned
    with pytest.raises(ValueError):
        plumes.rasterize_launch(ops, (8, 8), out=out)
    assert b"aligned" in hip.sc_last_error()
    a = _lib.sc_rast_args()
    a.out, a.H, a.W = out.data_ptr(), 1 << 16, 1 << 15
    assert hip.sc_rasterize_polygons(a, _lib.stream()) == -1 and b"H*W" in hip.sc_last_error()
    torch.cuda.synchronize()
    assert (out == -1).all()                                                # nothing was written, not even the clearing


# ---- 6. determinism ----

def test_two_calls_identical_bytes(hip):
    shape = R.SHAPES_GENERAL[0]
    polys = R.general_polygons(shape)
    first = plumes.rasterize_polygons(polys, shape)
    second = plumes.rasterize_polygons(polys, shape)
    plumes.rasterize_polygons([R.comb(50, 300, 8)], (8, 300))                # an unrelated call in between
    torch.zeros(1 << 20, device=DEV).sum()
    third = plumes.rasterize_polygons(polys, shape)
    assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes() == third.cpu().numpy().tobytes()


# ---- 7. match_plumes_polygons ----

def test_match_plumes_polygons(hip):
    """labelled with connectivity 2, no two components touch, not even at a corner: the polygons are the components"""
    label = OU.bernoulli((37, 53), 0.3, OU.SEEDS[0.3]).astype(np.uint8)
    pred = OU.bernoulli((37, 53), 0.5, OU.SEEDS[0.5]).astype(np.uint8)
    polys = plumes.plume_outlines(label, connectivity=2, geotransform=R.GT)
    for kw in ({}, {"min_overlap_px": 3, "min_area": 4}):
        want = plumes.match_plumes(pred, label, connectivity=2, **kw)
        got = plumes.match_plumes_polygons(pred, polys, geotransform=R.GT, **kw)
        assert (got["tp"], got["fp"], got["fn"]) == (want["tp"], want["fp"], want["fn"]) and want["tp"] > 0 and want["fn"] > 0, kw
        assert got["pred"].equals(want["pred"]), kw
        for c in ("plume_id", "area_px", "row_min", "row_max", "col_min", "col_max", "overlap_px"):
            assert got["label"][c].tolist() == want["label"][c].tolist(), (kw, c)
        if not kw:
            assert got["precision"] == want["precision"] and got["recall"] == want["recall"]
            # the same polygons as a plain list in pixel coordinates
            plain = plumes.plume_outlines(label, connectivity=2)
            again = plumes.match_plumes_polygons(pred, list(plain.values()))
            assert (again["tp"], again["fp"], again["fn"]) == (got["tp"], got["fp"], got["fn"]) and again["label"].equals(got["label"])


def test_match_plumes_polygons_keeps_touching_polygons_apart(hip):
    a, b = _square(1, 1, 5, 5), _square(5, 1, 9, 5)                         # share the edge x = 5
    pred = np.zeros((8, 12), dtype=np.uint8)
    pred[2:4, 6:11] = 1                                                     # overlaps b only
    union = np.zeros((8, 12), dtype=np.uint8)
    union[1:5, 1:9] = 1
    got = plumes.match_plumes_polygons(pred, [a, b])
    want = plumes.match_plumes(pred, union)
    assert len(want["label"]) == 1 and len(got["label"]) == 2
    assert got["label"]["area_px"].tolist() == [16, 16] and got["label"]["overlap_px"].tolist() == [0, 6]
    assert (got["tp"], got["fp"], got["fn"]) == (1, 0, 1) and (want["tp"], want["fp"], want["fn"]) == (1, 0, 0)
    with pytest.raises(ValueError):
        plumes.match_plumes_polygons(np.zeros((2, 8, 12), dtype=np.uint8), [a, b])


# ---- 8. the scene paths ----

def _tags(path):
    info = io_formats.tiff_info(path)
    assert info.tiled and info.block == (128, 128) and 42113 not in info.tags
    return {k: info.tags[k] for k in (33550, 33922, 34264, 34735, 34736, 34737) if k in info.tags}


def test_emit_granule_predict_label_polygons(hip, tmp_path):
    from starcop_amd import model_module as mm, pipeline
    nc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "io", "emit_l1b_like_sb0.nc")
    gt = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1)).to(DEV).eval()
    kw = dict(column_step=4, georeferenced=True, geotransform=gt, plumes=True, plume_outlines=True)
    first = pipeline.emit_granule_predict(model, nc, out_folder=str(tmp_path / "a"), **kw)
    assert "label_mask" not in first and "plume_match" not in first
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["albedo.tif", "mag1c.tif", "plumes.csv", "plumes.geojson", "pred.tif",
                                                       "predbinary.tif", "rgb.tif"]
    geojson = str(tmp_path / "a" / "plumes.geojson")
    out = pipeline.emit_granule_predict(model, nc, out_folder=str(tmp_path / "b"), label_polygons=geojson, **kw)
    assert set(out) - set(first) == {"label_mask", "plume_match"}
    assert out["label_mask"].is_cuda and out["label_mask"].dtype == torch.uint8
    assert torch.equal(out["label_mask"].to(torch.int64), out["pred_binary"].to(torch.int64)) and out["label_mask"].any()
    m = out["plume_match"]
    assert m["tp"] == len(out["plumes"]) >= 1 and m["fp"] == 0 and m["fn"] == 0 and len(m["label"]) == len(out["plumes"])
    names = [os.path.basename(p) for p in out["files"]]
    assert sorted(names) == ["albedo.tif", "label.tif", "mag1c.tif", "plumes.csv", "plumes.geojson", "pred.tif", "predbinary.tif", "rgb.tif"]
    lab = io_formats.read_tiff(str(tmp_path / "b" / "label.tif"))
    assert lab.dtype == np.uint8 and np.array_equal(lab.reshape(lab.shape[-2:]), out["label_mask"].cpu().numpy())
    assert _tags(str(tmp_path / "b" / "label.tif")) == _tags(str(tmp_path / "b" / "predbinary.tif")) != {}
    # polygons given as such; the overwrite rule; no grid without georeferencing
    again = pipeline.emit_granule_predict(model, nc, out_folder=str(tmp_path / "b"), label_polygons=out["plume_outlines"], **kw)
    assert again["files"] == [] and torch.equal(again["label_mask"], out["label_mask"])
    with pytest.raises(ValueError):
        pipeline.emit_granule_predict(model, nc, column_step=4, label_polygons=geojson)


def test_aviris_scene_predict_label_polygons(hip, tmp_path):
    import plume_scene_util as S
    from starcop_amd import pipeline
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
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32, plumes=True, plume_outlines=True)
    first = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "a"), **kw)
    assert "label_mask" not in first and "plume_match" not in first
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["plumes.csv", "plumes.geojson", "pred.tif", "predbinary.tif"]
    geojson = str(tmp_path / "a" / "plumes.geojson")
    out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "b"), label_polygons=geojson, **kw)
    assert set(out) - set(first) == {"label_mask", "plume_match"}
    assert out["label_mask"].dtype == torch.uint8 and out["label_mask"].any()
    assert torch.equal(out["label_mask"].to(torch.int64), out["pred_binary"].to(torch.int64))
    m = out["plume_match"]
    assert m["tp"] == len(out["plumes"]) >= 1 and m["fp"] == 0 and m["fn"] == 0
    assert sorted(os.path.basename(p) for p in out["files"]) == ["label.tif", "plumes.csv", "plumes.geojson", "pred.tif", "predbinary.tif"]
    lab = io_formats.read_tiff(str(tmp_path / "b" / "label.tif"))
    assert lab.dtype == np.uint8 and np.array_equal(lab.reshape(lab.shape[-2:]), out["label_mask"].cpu().numpy())
    assert _tags(str(tmp_path / "b" / "label.tif")) == _tags(str(tmp_path / "b" / "predbinary.tif")) != {}
    again = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "b"), label_polygons=out["plume_outlines"], **kw)
    assert again["files"] == [] and torch.equal(again["label_mask"], out["label_mask"])
    # without plumes=True the label mask and the match are still there
    bare = pipeline.aviris_scene_predict(model, folder, label_polygons=geojson, toa_correction_factor=1.037, tile=32, halo=32)
    assert torch.equal(bare["label_mask"], out["label_mask"]) and bare["plume_match"]["tp"] == m["tp"] and "plumes" not in bare
