"""The host half of the polygon burn: read_plumes against write_plumes, the numpy restatement of tests/rasterize_util.py against
cases worked by hand, and polygon_edges (the geotransform conversion, the closing edge, the boxes, the refusals).  No device."""
import json

import numpy as np
import pytest

import outlines_util as OU
import rasterize_util as R
from starcop_amd import plumes


def _table():
    import pandas as pd
    return pd.DataFrame({"item": [0, 0], "plume_id": [1, 2], "area_px": [12, 3], "row_min": [1, 6], "row_max": [4, 6],
                         "col_min": [1, 2], "col_max": [4, 4], "centroid_row": [2.5, 6.0], "centroid_col": [2.5, 3.0],
                         "prob_mean": [0.75, float("nan")], "x": [500012.5, 500015.0], "y": [3599987.5, 3599970.0]})


def _outlines():
    ext = np.array([(1.0, 1.0), (5.0, 1.0), (5.0, 5.0), (1.0, 5.0), (1.0, 1.0)])
    hole = np.array([(2.0, 2.0), (2.0, 4.0), (4.0, 4.0), (4.0, 2.0), (2.0, 2.0)])
    bar = np.array([(2.0, 6.0), (5.0, 6.0), (5.0, 7.0), (2.0, 7.0), (2.0, 6.0)])
    def geo(r):
        return np.stack([R.GT[0] + r[:, 0] * R.GT[1], R.GT[3] + r[:, 1] * R.GT[5]], 1)
    return {(0, 1): [geo(ext), geo(hole)], (0, 2): [geo(bar)]}


def _same_properties(table, want_rows):
    assert len(table) == len(want_rows)
    for got, row in zip(table.to_dict("records"), want_rows):
        want = plumes._properties(row)
        assert set(got) == set(want)
        for k, v in want.items():
            g = got[k]
            if v is None:
                assert g is None or (isinstance(g, float) and np.isnan(g)), k
            else:
                assert g == v, k


def test_read_plumes_polygons_round_trip(tmp_path):
    table, outlines = _table(), _outlines()
    path = plumes.write_plumes(table, str(tmp_path / "p.geojson"), outlines=outlines)
    got_table, got = plumes.read_plumes(path)
    _same_properties(got_table, table.to_dict("records"))
    assert len(got) == 2
    for rings, key in zip(got, [(0, 1), (0, 2)]):
        assert len(rings) == len(outlines[key])
        for a, b in zip(rings, outlines[key]):
            assert a.dtype == np.float64 and R.same_rings(a, b)


def test_read_plumes_points_and_multipolygon(tmp_path):
    table = _table()
    path = plumes.write_plumes(table, str(tmp_path / "pts.geojson"))
    got_table, got = plumes.read_plumes(path)
    assert got == [None, None]
    _same_properties(got_table, table.to_dict("records"))
    a = [[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0], [0.0, 0.0]]
    h = [[1.0, 1.0], [1.0, 2.0], [2.0, 2.0], [2.0, 1.0], [1.0, 1.0]]
    b = [[6.0, 0.0, 9.5], [8.0, 0.0, 9.5], [8.0, 3.0, 9.5], [6.0, 0.0, 9.5]]                    # with a height: dropped
    doc = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "geometry": {"type": "MultiPolygon", "coordinates": [[a, h], [b]]}, "properties": {"name": "two parts", "n": 2}},
        {"type": "Feature", "geometry": {"type": "Point", "coordinates": [1.0, 2.0]}, "properties": {"name": "a point", "n": 0}}]}
    mp = tmp_path / "multi.geojson"
    mp.write_text(json.dumps(doc))
    t, polys = plumes.read_plumes(str(mp))
    assert t["name"].tolist() == ["two parts", "a point"] and t["n"].tolist() == [2, 0]
    assert polys[1] is None and len(polys[0]) == 3
    for got_ring, want in zip(polys[0], (a, h, [p[:2] for p in b])):
        assert np.array_equal(got_ring, np.array(want))
    # the multi-polygon burns as one object: both parts, the hole left out
    ref = R.raster_ref(polys, [7, 9], 5, 9)
    want = np.zeros((5, 9), dtype=np.int32)
    want[0:4, 0:4] = 7
    want[1, 1] = 0
    want[0, 6:8] = 7; want[1, 7] = 7                              # the triangle (6,0) (8,0) (8,3): centres right of its hypotenuse
    assert np.array_equal(ref, want)
    doc["features"][1]["geometry"] = {"type": "LineString", "coordinates": [[0, 0], [1, 1]]}
    mp.write_text(json.dumps(doc))
    with pytest.raises(ValueError):
        plumes.read_plumes(str(mp))
    with pytest.raises(NotImplementedError):
        plumes.read_plumes("gs://bucket/plumes.geojson")
    with pytest.raises(ValueError):
        plumes.read_plumes(str(tmp_path / "plumes.csv"))


def test_raster_ref_hand_cases():
    # 1. the half-integer square: corners on pixel centres, top-left rule -> rows 2..5, columns 2..5, not 6
    sq = [np.array([(2.5, 2.5), (6.5, 2.5), (6.5, 6.5), (2.5, 6.5)])]
    want = np.zeros((9, 9), dtype=np.int32)
    want[2:6, 2:6] = 1
    assert np.array_equal(R.raster_ref([sq], [1], 9, 9), want)
    # 2. a right triangle (0,0) (6,0) (0,6): the centre (c + 0.5, r + 0.5) is inside iff c + r + 1 < 6; on the hypotenuse
    #    (c + r = 5) the crossing is at xs = c + 0.5 exactly and toggles pixel c OFF: not covered
    tri = [np.array([(0.0, 0.0), (6.0, 0.0), (0.0, 6.0)])]
    rr, cc = np.indices((7, 7))
    assert np.array_equal(R.raster_ref([tri], [5], 7, 7), np.where(rr + cc < 5, 5, 0).astype(np.int32))
    # 3. exterior with a hole and a later polygon over both: even-odd leaves the hole open, the later value wins where it covers
    ext = np.array([(1.0, 1.0), (7.0, 1.0), (7.0, 6.0), (1.0, 6.0), (1.0, 1.0)])
    hole = np.array([(3.0, 2.0), (3.0, 5.0), (5.0, 5.0), (5.0, 2.0)])
    late = [np.array([(4.0, 0.0), (9.0, 0.0), (9.0, 3.0), (4.0, 3.0)])]
    want = np.zeros((7, 10), dtype=np.int32)
    want[1:6, 1:7] = -3
    want[2:5, 3:5] = 0
    want[0:3, 4:9] = 8
    assert np.array_equal(R.raster_ref([[ext, hole], late], [-3, 8], 7, 10), want)
    # the same two in the other order: the first burn shows through the hole only where the later one does not cover
    want2 = np.zeros((7, 10), dtype=np.int32)
    want2[0:3, 4:9] = 8
    want2[1:6, 1:7] = -3
    want2[2:5, 3:5] = 0
    want2[2, 4] = 8
    assert np.array_equal(R.raster_ref([late, [ext, hole]], [8, -3], 7, 10), want2)


@pytest.mark.parametrize("connectivity", [1, 2])
def test_raster_ref_inverts_the_outline_restatement(connectivity):
    """the rings of outlines_ref through polygons_from_rings and back to pixel coordinates burn back to the label image"""
    mask = OU.bernoulli((37, 53), 0.5, OU.SEEDS[0.5])
    lab, n = OU.label(mask, connectivity)
    ref = OU.outlines_ref(lab, connectivity)
    polys = plumes.polygons_from_rings(*(ref[f] for f in plumes.OUTLINE_FIELDS), geotransform=R.GT)
    keys = list(polys)
    back = R.raster_ref([R.to_pixel(polys[k], R.GT) for k in keys], [k[1] for k in keys], *lab.shape)
    assert np.array_equal(back, lab)


def test_polygon_edges_geotransform_boxes_and_closing():
    ring_px = np.array([(2.5, 2.5), (6.5, 2.5), (6.5, 6.5), (2.5, 6.5)])
    ring_xy = np.stack([R.GT[0] + ring_px[:, 0] * R.GT[1], R.GT[3] + ring_px[:, 1] * R.GT[5]], 1)
    e_px, t_px = plumes.polygon_edges([[ring_px]], (9, 12))
    e_xy, t_xy = plumes.polygon_edges([[ring_xy]], (9, 12), geotransform=R.GT)
    assert e_px.dtype == np.float64 and e_px.shape == (4, 4) and np.array_equal(e_px, e_xy) and np.array_equal(t_px, t_xy)
    assert np.array_equal(e_px[:, :2], ring_px) and np.array_equal(e_px[:, 2:], np.roll(ring_px, -1, axis=0))      # closed by the last edge
    closed = np.concatenate([ring_px, ring_px[:1]])
    assert np.array_equal(plumes.polygon_edges([[closed]], (9, 12))[0], e_px)                      # no edge added twice
    e0, e1, r0, r1, c0, c1, job0, _ = t_px[0].tolist()
    assert (e0, e1, job0) == (0, 4, 0) and r0 <= 2 and r1 >= 6 and c0 <= 2 and c1 >= 6
    # boxes are clipped to the raster; a polygon outside has none and takes no job; None has no edges
    far = [np.array([(-1e6, -1e6), (1e6, -1e6), (0.0, 1e6)])]
    out = [np.array([(20.0, 1.0), (25.0, 1.0), (25.0, 5.0)])]
    e, t = plumes.polygon_edges([far, out, None, [ring_px]], (9, 12))
    assert t.dtype == np.int32 and t.shape == (4, 8) and e.shape == (3 + 3 + 4, 4)
    assert t[0, 2:6].tolist() == [0, 9, 0, 12] and t[1, 2:6].tolist() == [0, 0, 0, 0] and t[2, :2].tolist() == [6, 6]
    assert t[:, 6].tolist() == [0, 9, 9, 9]
    with pytest.raises(NotImplementedError):
        plumes.polygon_edges([[ring_xy]], (9, 12), geotransform=(500000.0, 5.0, 0.1, 3600000.0, 0.0, -5.0))
    with pytest.raises(ValueError):
        plumes.polygon_edges([[ring_xy]], (9, 12), geotransform=(500000.0, 5.0, 0.0, 3600000.0))


@pytest.mark.parametrize("bad", ["nan", "inf", "huge", "two_points", "repeated", "shape", "hw"])
def test_polygon_edges_refusals(bad):
    ring = np.array([(1.0, 1.0), (5.0, 1.0), (5.0, 5.0)])
    shape = (8, 8)
    if bad == "nan":
        ring[1, 0] = np.nan
    elif bad == "inf":
        ring[2, 1] = -np.inf
    elif bad == "huge":
        ring[0, 0] = -2.0 ** 31
    elif bad == "two_points":
        ring = ring[:2]
    elif bad == "repeated":
        ring = ring[[0, 1, 0, 1, 0]]
    elif bad == "shape":
        ring = np.zeros((4, 3))
    else:
        shape = (1 << 16, 1 << 15)
    with pytest.raises(ValueError):
        plumes.polygon_edges([[ring]], shape)
