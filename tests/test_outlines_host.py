"""The sequential restatement of the component outlines (tests/outlines_util.py) against its invariants, and the host half of
starcop_amd.plumes on its rings: polygons_from_rings and write_plumes(..., outlines=).  No device."""
import json

import numpy as np
import pandas as pd
import pytest

import outlines_util as U
from starcop_amd import plumes

MASKS = U.all_small_masks()
GT_NORTH_UP = (500000.0, 5.0, 0.0, 4100000.0, 0.0, -5.0)
GT_SOUTH_UP = (500000.0, 5.0, 0.0, 4100000.0, 0.0, 5.0)


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_restatement_invariants(name, connectivity):
    lab, n = U.label(MASKS[name], connectivity)
    full = U.outlines_ref(lab, connectivity, collinear=True)
    U.check_invariants(lab, n, full)
    assert full["vertices"].shape[0] == full["n_edges"]
    corners = U.outlines_ref(lab, connectivity, collinear=False)
    U.check_invariants(lab, n, corners)
    assert np.array_equal(corners["ring_label"], full["ring_label"]) and np.array_equal(corners["ring_area2"], full["ring_area2"])
    if n:
        assert corners["vertices"].shape[0] < full["vertices"].shape[0] or name in ("checkerboard", "one_pixel", "diagonal_pair")
        assert np.diff(corners["ring_offsets"]).min() >= 4


def test_restatement_known_cases():
    m = U.hand_masks()
    lab, n = U.label(m["diagonal_pair"], 2)
    out = U.outlines_ref(lab, 2)
    assert n == 1 and out["ring_area2"].tolist() == [4] and out["ring_offsets"].tolist() == [0, 8]       # one ring that touches itself
    lab, n = U.label(m["diagonal_pair"], 1)
    out = U.outlines_ref(lab, 1)
    assert n == 2 and out["ring_area2"].tolist() == [2, 2]
    lab, n = U.label(m["one_pixel"], 2)
    assert U.outlines_ref(lab, 2)["vertices"].tolist() == [[2, 3], [2, 4], [3, 4], [3, 3]]
    # the component's pixels meet diagonally at corner (5, 5): connectivity 2 crosses there, which keeps the two background squares
    # apart; connectivity 1 turns back, which joins them into one hole ring that touches itself at that corner
    lab, n = U.label(m["pinched_hole"], 1)
    out = U.outlines_ref(lab, 1)
    assert n == 1 and out["ring_area2"].tolist() == [2 * 72, -2 * 8]
    assert (out["vertices"][out["ring_offsets"][1]:] == [5, 5]).all(1).sum() == 2
    out2 = U.outlines_ref(U.label(m["pinched_hole"], 2)[0], 2)
    assert out2["ring_area2"].tolist() == [2 * 72, -2 * 4, -2 * 4]
    lab, n = U.label(U.spiral(), 1)
    out = U.outlines_ref(lab, 1, collinear=True)
    assert n == 1 and out["longest"] == 1156 == out["n_edges"]
    assert U.outlines_ref(U.label(m["empty"], 2)[0], 2)["ring_offsets"].tolist() == [0]


def _rings(name, connectivity):
    lab, n = U.label(MASKS[name], connectivity)
    return lab, n, U.outlines_ref(lab, connectivity)


def _poly(out, **kw):
    return plumes.polygons_from_rings(out["vertices"], out["ring_offsets"], out["ring_label"], out["ring_area2"], **kw)


def test_polygons_from_rings():
    lab, n, out = _rings("island_in_hole", 2)
    polys = _poly(out)
    assert sorted(polys) == [(0, 1), (0, 2)]
    assert len(polys[(0, 1)]) == 2 and len(polys[(0, 2)]) == 1
    for rings in polys.values():
        for q, ring in enumerate(rings):
            assert ring.dtype == np.float64 and ring.shape[1] == 2 and np.array_equal(ring[0], ring[-1])
            assert (plumes._shoelace(ring) > 0) == (q == 0)                                              # exterior first, then holes
    off = out["ring_offsets"]
    first = out["vertices"][off[0]:off[1]]
    assert np.array_equal(polys[(0, 1)][0][:-1], first[:, ::-1].astype(np.float64))                      # (x, y) = (col, row)
    assert sorted(_poly(out, item=3)) == [(3, 1), (3, 2)]


def test_polygons_min_area():
    lab, n, out = _rings("bernoulli_0.3", 1)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    for min_area in (1, 2, 5, 40):
        want = [(0, k) for k in range(1, n + 1) if area[k] >= min_area]
        assert sorted(_poly(out, min_area=min_area)) == want
    assert 0 < len(_poly(out, min_area=5)) < n


@pytest.mark.parametrize("gt", [GT_NORTH_UP, GT_SOUTH_UP, (3.0, 0.25, 0.0, -7.0, 0.0, 0.125)])
def test_polygons_geotransform(gt):
    lab, n, out = _rings("square_ring", 2)
    polys = _poly(out, geotransform=gt)
    off = out["ring_offsets"]
    for q, ring in enumerate(polys[(0, 1)]):
        v = out["vertices"][off[q]:off[q + 1]].astype(np.float64)
        v = np.concatenate([v, v[:1]])
        assert np.array_equal(ring[:, 0], gt[0] + v[:, 1] * gt[1]) and np.array_equal(ring[:, 1], gt[3] + v[:, 0] * gt[5])


def test_polygons_refuse_rotation():
    lab, n, out = _rings("one_pixel", 2)
    with pytest.raises(NotImplementedError):
        _poly(out, geotransform=(0.0, 1.0, 0.1, 0.0, 0.0, -1.0))
    with pytest.raises(NotImplementedError):
        _poly(out, geotransform=(0.0, 1.0, 0.0, 0.0, 0.2, -1.0))
    with pytest.raises(ValueError):
        _poly(out, geotransform=(0.0, 1.0, 0.0))


def _table(lab, n, gt):
    """the columns of plume_table a writer needs, from the label image"""
    rows = []
    for k in range(1, n + 1):
        r, c = np.nonzero(lab == k)
        rows.append({"item": 0, "plume_id": k, "area_px": r.size, "row_min": r.min(), "row_max": r.max(), "col_min": c.min(),
                     "col_max": c.max(), "centroid_row": r.mean(), "centroid_col": c.mean(), "mag1c_mean": np.nan if k == 1 else 1.5 * k,
                     "x": gt[0] + (c.mean() + 0.5) * gt[1], "y": gt[3] + (r.mean() + 0.5) * gt[5]})
    return pd.DataFrame(rows)


@pytest.mark.parametrize("gt", [GT_NORTH_UP, GT_SOUTH_UP])
def test_write_plumes_polygons(tmp_path, gt):
    lab, n, out = _rings("island_in_hole", 2)
    table = _table(lab, n, gt)
    polys = _poly(out, geotransform=gt)
    pts = json.load(open(plumes.write_plumes(table, str(tmp_path / "points.geojson"))))
    got = json.load(open(plumes.write_plumes(table, str(tmp_path / "polygons.geojson"), outlines=polys)))
    assert got["type"] == "FeatureCollection" and len(got["features"]) == n == 2
    for f, g, k in zip(got["features"], pts["features"], range(1, n + 1)):
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon" and g["geometry"]["type"] == "Point"
        assert f["properties"] == g["properties"] and f["properties"]["plume_id"] == k and "bbox_px" in f["properties"]
        rings = [np.array(r) for r in f["geometry"]["coordinates"]]
        assert len(rings) == len(polys[(0, k)])
        for q, ring in enumerate(rings):
            assert np.array_equal(ring[0], ring[-1])
            sh = np.sum(ring[:-1, 0] * ring[1:, 1] - ring[1:, 0] * ring[:-1, 1])
            assert (sh > 0) if q == 0 else (sh < 0)                                                       # RFC 7946 winding
            src = polys[(0, k)][q]
            assert np.array_equal(ring, src[::-1] if gt[1] * gt[5] < 0 else src)
    assert got["features"][0]["properties"]["mag1c_mean"] is None
    # a table without x / y (no geotransform) still writes polygons, in pixel corners
    bare = json.load(open(plumes.write_plumes(table.drop(columns=["x", "y"]), str(tmp_path / "bare.geojson"), outlines=_poly(out))))
    assert bare["features"][1]["geometry"]["coordinates"][0][0] == [5.0, 5.0]
    with pytest.raises(ValueError):
        plumes.write_plumes(table, str(tmp_path / "missing.geojson"), outlines={(0, 1): polys[(0, 1)]})


def test_write_plumes_without_outlines_is_unchanged(tmp_path):
    lab, n, out = _rings("island_in_hole", 2)
    table = _table(lab, n, GT_NORTH_UP)
    a = open(plumes.write_plumes(table, str(tmp_path / "a.geojson")), "rb").read()
    b = open(plumes.write_plumes(table, str(tmp_path / "b.geojson"), outlines=None), "rb").read()
    feats = []                                                   # the Point writer as it stood before `outlines` existed
    for row in table.to_dict("records"):
        props = {}
        for c, v in row.items():
            if c in ("x", "y"):
                continue
            v = v.item() if hasattr(v, "item") else v
            props[c] = None if isinstance(v, float) and not np.isfinite(v) else v
        props["bbox_px"] = [int(row["row_min"]), int(row["col_min"]), int(row["row_max"]), int(row["col_max"])]
        feats.append({"type": "Feature", "geometry": {"type": "Point", "coordinates": [float(row["x"]), float(row["y"])]},
                      "properties": props})
    assert a == b == json.dumps({"type": "FeatureCollection", "features": feats}).encode()
    c = open(plumes.write_plumes(table, str(tmp_path / "c.csv"), outlines=_poly(out)), "rb").read()
    d = open(plumes.write_plumes(table, str(tmp_path / "d.csv")), "rb").read()
    assert c == d
    with pytest.raises(ValueError):
        plumes.write_plumes(table.drop(columns=["x"]), str(tmp_path / "e.geojson"))


def test_outline_abi_without_a_device():
    """the size guard and the round count are host arithmetic"""
    from starcop_amd import _lib
    lib = _lib.load()
    assert lib.sc_component_outlines_workspace_bytes(1 << 15, 1 << 14, 16) == 0                         # 4 * H * W = 2^31
    assert lib.sc_component_outlines_workspace_bytes(37, 70, 0) == 0 * 45
    assert 45 * 2654 <= lib.sc_component_outlines_workspace_bytes(37, 70, 2654) <= 45 * 2654 + 9 * 256
    assert lib.sc_component_outlines_workspace_bytes(4, 4, 65) == 0                                      # more edges than sides
    assert [lib.sc_component_outlines_rounds(e) for e in (4, 1156, 2654, 1 << 20)] == [3, 12, 13, 21]
    a = _lib.sc_outline_args()
    a.labels, a.H, a.W, a.connectivity = 1, 1 << 15, 1 << 14, 2                                         # refused before anything is read
    assert lib.sc_component_outlines(a, _lib.OUTLINE_COUNT, None) == -1
    assert b"4*H*W" in lib.sc_last_error()
    a.H, a.W, a.connectivity = 8, 8, 3
    assert lib.sc_component_outlines(a, _lib.OUTLINE_COUNT, None) == -1
