"""Host side of starcop_amd.plumes: table assembly, the writers, argument checks, and the oracle of the GPU tests pinned by hand."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import plumes_util as pu
from starcop_amd import plumes


def _stats(N, M, P):
    st = {f: np.zeros((N, M), np.int64) for f in pu.COMPONENT_FIELDS}
    st.update(n_finite=np.zeros((N, M, P), np.int64), sum=np.zeros((N, M, P)), max=np.zeros((N, M, P), np.float32),
              min=np.zeros((N, M, P), np.float32), argmax=np.zeros((N, M, P), np.int64))
    return st


def _hand_stats():
    """two images, M = 3: image 0 has components of 4 and 1 pixels, image 1 one of 6 pixels whose mag1c is all NaN"""
    st = _stats(2, 3, 2)
    st["area"][:] = [[4, 1, 0], [6, 0, 0]]
    st["row_min"][:] = [[2, 7, 0], [0, 0, 0]]
    st["row_max"][:] = [[3, 7, 0], [1, 0, 0]]
    st["col_min"][:] = [[10, 0, 0], [3, 0, 0]]
    st["col_max"][:] = [[11, 0, 0], [5, 0, 0]]
    st["sum_row"][:] = [[10, 7, 0], [3, 0, 0]]
    st["sum_col"][:] = [[42, 0, 0], [24, 0, 0]]
    st["n_other"][:] = [[3, 0, 0], [6, 0, 0]]
    st["n_finite"][0, 0], st["n_finite"][0, 1], st["n_finite"][1, 0] = [3, 4], [1, 1], [0, 6]
    st["sum"][0, 0], st["sum"][0, 1], st["sum"][1, 0] = [900.0, 2.0], [250.0, 0.75], [0.0, 3.0]
    st["max"][0, 0], st["max"][0, 1], st["max"][1, 0] = [500.0, 0.75], [250.0, 0.75], [np.nan, 0.5]
    st["argmax"][0, 0], st["argmax"][0, 1], st["argmax"][1, 0] = [3 * 20 + 11, 0], [7 * 20, 0], [-1, 0]
    return st


def test_table_from_hand_written_stats():
    gt = (-103.5, 0.001, 0.0, 32.25, 0.0, -0.002)
    t = plumes.table_from_stats(_hand_stats(), [2, 1], 20, ("mag1c", "prob"), with_other=True, geotransform=gt, pixel_area_m2=3600.0)
    assert list(t.columns) == ["item", "plume_id", "area_px", "row_min", "row_max", "col_min", "col_max", "centroid_row",
                               "centroid_col", "mag1c_sum", "mag1c_mean", "mag1c_max", "mag1c_max_row", "mag1c_max_col",
                               "ime_ppmm_m2", "prob_mean", "prob_max", "overlap_px", "x", "y"]
    assert t["item"].tolist() == [0, 0, 1] and t["plume_id"].tolist() == [1, 2, 1] and t["area_px"].tolist() == [4, 1, 6]
    assert t["row_min"].tolist() == [2, 7, 0] and t["col_max"].tolist() == [11, 0, 5]
    assert t["centroid_row"].tolist() == [2.5, 7.0, 0.5] and t["centroid_col"].tolist() == [10.5, 0.0, 4.0]
    assert t["centroid_row"].dtype == np.float64 and t["area_px"].dtype == np.int64
    assert t["mag1c_sum"].tolist()[:2] == [900.0, 250.0] and t["mag1c_mean"].tolist()[:2] == [300.0, 250.0]      # over FINITE pixels
    assert t["mag1c_max_row"].tolist() == [3, 7, -1] and t["mag1c_max_col"].tolist() == [11, 0, -1]
    assert np.isnan(t["mag1c_mean"][2]) and np.isnan(t["mag1c_max"][2]) and t["mag1c_sum"][2] == 0.0
    assert t["ime_ppmm_m2"].tolist() == [900.0 * 3600.0, 250.0 * 3600.0, 0.0]
    assert t["prob_mean"].tolist() == [0.5, 0.75, 0.5] and t["prob_max"].tolist() == [0.75, 0.75, 0.5]
    assert t["overlap_px"].tolist() == [3, 0, 6]
    # pixel centres: gt[0] + (col + 0.5) * gt[1]
    assert t["x"].tolist() == [-103.5 + 11.0 * 0.001, -103.5 + 0.5 * 0.001, -103.5 + 4.5 * 0.001]
    assert t["y"].tolist() == [32.25 + 3.0 * -0.002, 32.25 + 7.5 * -0.002, 32.25 + 1.0 * -0.002]


def test_table_min_area_and_optional_columns():
    st = _hand_stats()
    t = plumes.table_from_stats(st, [2, 1], 20, min_area=2)
    assert list(t.columns) == ["item", "plume_id", "area_px", "row_min", "row_max", "col_min", "col_max", "centroid_row", "centroid_col"]
    assert t["plume_id"].tolist() == [1, 1] and t["item"].tolist() == [0, 1]
    assert len(plumes.table_from_stats(st, [2, 1], 20, min_area=7)) == 0
    # rows at or above counts[n] never appear, whatever they hold
    st["area"][1, 1] = 9
    assert plumes.table_from_stats(st, [2, 1], 20)["area_px"].tolist() == [4, 1, 6]
    # a value no pixel carries (area 0) is not a plume
    assert plumes.table_from_stats(st, [3, 1], 20)["area_px"].tolist() == [4, 1, 6]
    with pytest.raises(NotImplementedError):
        plumes.table_from_stats(st, [2, 1], 20, geotransform=(0, 1, 0.1, 0, 0, -1))
    with pytest.raises(ValueError):
        plumes.table_from_stats(st, [2, 1], 20, geotransform=(0, 1, 0))


def test_write_csv_and_geojson_round_trip(tmp_path):
    gt = (500000.0, 60.0, 0.0, 4100000.0, 0.0, -60.0)
    t = plumes.table_from_stats(_hand_stats(), [2, 1], 20, ("mag1c", "prob"), with_other=True, geotransform=gt)
    p = plumes.write_plumes(t, tmp_path / "plumes.csv")
    back = pd.read_csv(p, float_precision="round_trip")
    assert list(back.columns) == list(t.columns)
    for c in t.columns:
        assert np.array_equal(back[c].to_numpy(), t[c].to_numpy(), equal_nan=True), c
        assert back[c].dtype == t[c].dtype, c
    p = plumes.write_plumes(t, str(tmp_path / "plumes.geojson"))
    gj = json.load(open(p))
    assert gj["type"] == "FeatureCollection" and len(gj["features"]) == 3
    for f, (_, row) in zip(gj["features"], t.iterrows()):
        assert f["type"] == "Feature" and f["geometry"] == {"type": "Point", "coordinates": [row["x"], row["y"]]}
        pr = f["properties"]
        assert pr["bbox_px"] == [row["row_min"], row["col_min"], row["row_max"], row["col_max"]]
        assert pr["area_px"] == row["area_px"] and pr["plume_id"] == row["plume_id"] and pr["overlap_px"] == row["overlap_px"]
        assert "x" not in pr and "y" not in pr
    assert gj["features"][2]["properties"]["mag1c_max"] is None and gj["features"][0]["properties"]["mag1c_max"] == 500.0


def test_write_errors(tmp_path):
    t = plumes.table_from_stats(_hand_stats(), [2, 1], 20)
    with pytest.raises(ValueError, match="x / y"):
        plumes.write_plumes(t, tmp_path / "p.geojson")
    with pytest.raises(NotImplementedError):
        plumes.write_plumes(t, "gs://bucket/plumes.csv")
    with pytest.raises(ValueError):
        plumes.write_plumes(t, tmp_path / "p.parquet")
    assert not list(tmp_path.iterdir())


def test_argument_checks_come_before_the_device():
    lab = torch.zeros((2, 8, 9), dtype=torch.int32)
    cnt = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 8"):
        plumes.component_stats(lab, cnt, [torch.zeros(2, 8, 9)] * 9)
    with pytest.raises(ValueError, match="plane 1"):
        plumes.component_stats(lab, cnt, [torch.zeros(2, 8, 9), torch.zeros(2, 9, 8)])
    with pytest.raises(ValueError, match="other"):
        plumes.component_stats(lab, cnt, other=torch.zeros(8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="counts"):
        plumes.component_stats(lab, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="labels"):
        plumes.component_stats(torch.zeros(8, dtype=torch.int32), 0)
    m = np.zeros((8, 9), bool)
    with pytest.raises(ValueError, match="mag1c"):
        plumes.plume_table(m, mag1c=np.zeros((9, 8), np.float32))
    with pytest.raises(ValueError, match="prob"):
        plumes.plume_table(m, prob=np.zeros((1, 8, 9), np.float32))
    with pytest.raises(ValueError, match="label_mask"):
        plumes.plume_table(m, label_mask=np.zeros((8, 10), bool))
    with pytest.raises(ValueError, match="mask"):
        plumes.plume_table(np.zeros(8, bool))


def test_oracle_on_a_hand_derived_case():
    """6 x 6 labels written by hand (label 2 in two pieces, label 4 absent, a stray 9 and -1 to ignore), one plane with a
    plateau of maxima, a NaN, an inf and a component that is all NaN; every expected number below is derived on paper"""
    lab = np.array([[1, 1, 0, 2, 0, 9],
                    [1, 0, 0, 0, 0, 0],
                    [0, 0, 3, 3, 0, 0],
                    [0, 0, 3, 0, 0, 2],
                    [5, 0, 0, 0, 0, 2],
                    [5, -1, 0, 0, 0, 0]])
    nan, inf = np.nan, np.inf
    v = np.array([[1, 5, 0, -2, 0, 7],
                  [5, 0, 0, 0, 0, 0],
                  [0, 0, 4, inf, 0, 0],
                  [0, 0, nan, 0, 0, -8],
                  [nan, 0, 0, 0, 0, -2],
                  [nan, 0, 0, 0, 0, 0]], dtype=np.float32)
    other = np.zeros((6, 6), np.uint8)
    other[0, :2] = 7
    other[3:, 5] = 1
    st = pu.oracle_stats(lab, 5, [v], other)
    assert st["area"].tolist() == [3, 3, 3, 0, 2]
    assert st["row_min"].tolist() == [0, 0, 2, 0, 4] and st["row_max"].tolist() == [1, 4, 3, 0, 5]
    assert st["col_min"].tolist() == [0, 3, 2, 0, 0] and st["col_max"].tolist() == [1, 5, 3, 0, 0]
    assert st["sum_row"].tolist() == [1, 7, 7, 0, 9] and st["sum_col"].tolist() == [1, 13, 7, 0, 0]
    assert st["first_pixel"].tolist() == [0, 3, 14, -1, 24]
    assert st["n_other"].tolist() == [2, 2, 0, 0, 0]
    assert st["n_finite"][:, 0].tolist() == [3, 3, 1, 0, 0]
    assert st["sum"][:, 0].tolist() == [11.0, -12.0, 4.0, 0.0, 0.0]
    assert st["sum_abs"][:, 0].tolist() == [11.0, 12.0, 4.0, 0.0, 0.0]
    assert st["argmax"][:, 0].tolist() == [1, 3, 14, -1, -1]           # label 1: 5 at raster 1 and 6 -> the first; label 2: all negative
    assert np.array_equal(st["max"][:, 0], np.array([5, -2, 4, nan, nan], np.float32), equal_nan=True)
    assert np.array_equal(st["min"][:, 0], np.array([1, -8, 4, nan, nan], np.float32), equal_nan=True)
    # a tie: the first raster index, where scipy.ndimage.maximum_position answers (0, 2)
    tie = pu.oracle_stats(np.ones((2, 3), int), 1, [np.array([[1, 5, 5], [5, 0, 2]], np.float32)])
    assert tie["argmax"][0, 0] == 1


def test_shared_masks():
    s = pu.spiral(65)
    lab, n = pu.scipy_label(s, 1)
    assert n == 1 and s[0].all() and s[:, -1].all() and s[-1].all() and 65 * 65 // 3 < s.sum() < 65 * 65 * 0.6
    assert pu.scipy_label(s, 2)[1] == 1
    d = pu.diagonal_stripes(40, 50)
    assert pu.scipy_label(d, 2)[1] == 23 and pu.scipy_label(d, 1)[1] == int(d.sum())
