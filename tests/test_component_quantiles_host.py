"""Host side of the per-plume order statistics: the argument checks that come before the device, the table columns of
``background_stat="median"`` / ``percentiles=`` from synthetic host inputs, and the byte identity of the table without them."""
import numpy as np
import pytest
import torch

import component_quantiles_util as cq
from starcop_amd import _lib, plumes, products


def _stats(N, M):
    st = {f: np.zeros((N, M), np.int64) for f in plumes.COMPONENT_FIELDS}
    st.update(n_finite=np.zeros((N, M, 1), np.int64), sum=np.zeros((N, M, 1)), max=np.zeros((N, M, 1), np.float32),
              min=np.zeros((N, M, 1), np.float32), argmax=np.zeros((N, M, 1), np.int64))
    return st


def _case():
    """one image, three plumes of 4, 9 and 2 finite pixels; rings of 10, 0 and 5 finite pixels"""
    st = _stats(1, 3)
    st["area"][:] = [[4, 9, 2]]
    st["n_finite"][0, :, 0] = [4, 9, 2]
    st["sum"][0, :, 0] = [900.0, 1800.0, 10.0]
    st["max"][0, :, 0] = [500.0, 400.0, 6.0]
    ring = _stats(1, 3)
    ring["n_finite"][0, :, 0] = [10, 0, 5]
    ring["sum"][0, :, 0] = [200.0, 0.0, 15.0]
    rq = {"median": np.array([[12.5, np.nan, 3.0]], np.float32), "mad": np.array([[8.0, np.nan, 0.0]], np.float32)}
    return st, ring, rq


def test_bad_q_is_refused_before_the_device():
    lab = torch.zeros((4, 5), dtype=torch.int32)
    plane = torch.zeros((4, 5))
    for q in [(), (1,) * 9, (-0.5,), (100.5,), (float("nan"),), ("mean",), "median", 50, (None,)]:
        with pytest.raises(ValueError):
            plumes.component_quantiles(lab, 1, plane, q)
    with pytest.raises(ValueError):
        plumes.component_quantiles(lab.numpy(), 1, plane, ("median",))                     # not a tensor
    with pytest.raises(ValueError):
        plumes.component_quantiles(lab, 1, torch.zeros((4, 6)), ("median",))               # shape mismatch
    with pytest.raises(ValueError):
        plumes.component_quantiles(lab, torch.zeros(2, dtype=torch.int32), plane)           # two counts for one image
    with pytest.raises(ValueError):
        plumes.component_quantiles(lab, 1, plane, center=torch.zeros((2, 3)))               # centres of another batch
    with pytest.raises(ValueError):
        plumes.component_quantiles(lab, 1, plane, center=torch.zeros((1, 3)), M=4)


def test_fractions_are_the_float32_quotients():
    fr = plumes.quantile_fractions((0, 2.5, 33.3, "median", 99.9, 100), "t")
    want = [np.float32(0) / np.float32(100), np.float32(2.5) / np.float32(100), np.float32(33.3) / np.float32(100), np.float32(-1),
            np.float32(99.9) / np.float32(100), np.float32(1)]
    assert all(type(f) is np.float32 for f in fr) and [f.tobytes() for f in fr] == [w.tobytes() for w in want]
    assert plumes.quantile_names((5, "median", 95, 2.5, 99.9)) == ["mag1c_p5", "mag1c_median", "mag1c_p95", "mag1c_p2.5", "mag1c_p99.9"]
    assert _lib.CQUANT_MAX_Q == 8 and _lib.CQUANT_SMALL_MAX & (_lib.CQUANT_SMALL_MAX - 1) == 0


def test_plume_table_checks_come_before_the_device():
    mask = np.zeros((8, 8), np.uint8)
    mag = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError, match="background_ring_px"):
        plumes.plume_table(mask, mag1c=mag, background_stat="median")
    with pytest.raises(ValueError, match="background_stat"):
        plumes.plume_table(mask, mag1c=mag, background_ring_px=4, background_stat="mode")
    with pytest.raises(ValueError, match="mag1c"):
        plumes.plume_table(mask, percentiles=(5, 95))
    with pytest.raises(ValueError):
        plumes.plume_table(mask, mag1c=mag, percentiles=(5, 101))
    with pytest.raises(ValueError):
        plumes.plume_table(mask, mag1c=mag, percentiles=())
    with pytest.raises(ValueError):
        plumes.fetch_profiles(mask, mag, {"wind_speed_m_s": 3.0}, pixel_area_m2=900.0, background_stat="median")


def test_plume_background_keys():
    assert products.BACKGROUND_KEYS == ("ring_px", "gap_px", "stat")
    assert products.check_plume_background({"ring_px": 8, "gap_px": 2, "stat": "median"}, "t") == \
        {"background_ring_px": 8, "background_gap_px": 2, "background_stat": "median"}
    assert products.check_plume_background({"ring_px": 8, "stat": "mean"}, "t") == \
        {"background_ring_px": 8, "background_gap_px": 0.0, "background_stat": "mean"}
    assert products.check_plume_background({"ring_px": 8}, "t") == {"background_ring_px": 8, "background_gap_px": 0.0}
    for bad in [{"ring_px": 8, "stat": "mode"}, {"ring_px": 8, "statistic": "median"}, {"stat": "median"}, {"ring_px": 8, "radius": 1}]:
        with pytest.raises(ValueError):
            products.check_plume_background(bad, "t")


def test_table_columns_of_the_median_background():
    st, ring, rq = _case()
    base = plumes.table_from_stats(st, [3], 20, ("mag1c",), pixel_area_m2=900.0, ring_stats=ring)
    t = plumes.table_from_stats(st, [3], 20, ("mag1c",), pixel_area_m2=900.0, ring_stats=ring, ring_quantiles=rq)
    new = ["mag1c_bg_median", "mag1c_bg_mad", "mag1c_bg_sigma", "ime_sigma_ppmm_m2", "snr"]
    assert list(t.columns) == list(base.columns) + new
    assert list(base.columns)[-4:] == ["bg_px", "mag1c_bg_mean", "mag1c_sum_bgsub", "ime_bgsub_ppmm_m2"]
    n = np.array([4.0, 9.0, 2.0])
    med, mad = np.array([12.5, np.nan, 3.0]), np.array([8.0, np.nan, 0.0])
    s = np.array([900.0, 1800.0, 10.0])
    # bg_px and the ring mean stay; what is subtracted is the median
    assert t["bg_px"].tolist() == [10, 0, 5] and np.array_equal(t["mag1c_bg_mean"], base["mag1c_bg_mean"], equal_nan=True)
    assert np.array_equal(t["mag1c_bg_mean"], [20.0, np.nan, 3.0], equal_nan=True)
    assert np.array_equal(t["mag1c_sum_bgsub"], s - med * n, equal_nan=True) and np.isnan(t["mag1c_sum_bgsub"][1])
    assert np.array_equal(base["mag1c_sum_bgsub"], s - np.array([20.0, np.nan, 3.0]) * n, equal_nan=True)
    assert np.array_equal(t["ime_bgsub_ppmm_m2"], (s - med * n) * 900.0, equal_nan=True)
    assert t["mag1c_bg_median"].dtype == np.float64 and np.array_equal(t["mag1c_bg_median"], med, equal_nan=True)
    assert np.array_equal(t["mag1c_bg_mad"], mad, equal_nan=True)
    assert np.array_equal(t["mag1c_bg_sigma"], 1.4826 * mad, equal_nan=True)
    assert np.array_equal(t["ime_sigma_ppmm_m2"], 1.4826 * mad * np.sqrt(n) * 900.0, equal_nan=True)
    # snr: NaN without a ring (row 1) and where sigma is 0 (row 2)
    assert t["snr"][0] == (900.0 - 12.5 * 4.0) / (1.4826 * 8.0 * 2.0) and np.isnan(t["snr"][1]) and np.isnan(t["snr"][2])
    # without a pixel area the two area columns are absent, the rest stays
    t2 = plumes.table_from_stats(st, [3], 20, ("mag1c",), ring_stats=ring, ring_quantiles=rq)
    assert list(t2.columns)[-7:] == ["bg_px", "mag1c_bg_mean", "mag1c_sum_bgsub", "mag1c_bg_median", "mag1c_bg_mad", "mag1c_bg_sigma", "snr"]
    with pytest.raises(ValueError):
        plumes.table_from_stats(st, [3], 20, ("mag1c",), ring_quantiles=rq)                 # needs ring_stats


def test_table_columns_of_the_percentiles():
    st, ring, rq = _case()
    pq = {"q": (5, "median", 99.9), "quantile": np.arange(9, dtype=np.float32).reshape(1, 3, 3) + np.float32(0.25)}
    base = plumes.table_from_stats(st, [3], 20, ("mag1c",))
    t = plumes.table_from_stats(st, [3], 20, ("mag1c",), plume_quantiles=pq)
    assert list(t.columns) == list(base.columns) + ["mag1c_p5", "mag1c_median", "mag1c_p99.9"]
    assert t["mag1c_p5"].tolist() == [0.25, 3.25, 6.25] and t["mag1c_p99.9"].tolist() == [2.25, 5.25, 8.25]
    assert t["mag1c_median"].dtype == np.float64
    # min_area filters the rows of the new columns with the others
    assert plumes.table_from_stats(st, [3], 20, ("mag1c",), min_area=3, plume_quantiles=pq)["mag1c_median"].tolist() == [1.25, 4.25]
    # after the ring columns, before prob
    st2 = {f: (np.concatenate([v, v], 2) if v.ndim == 3 else v) for f, v in st.items()}
    both = plumes.table_from_stats(st2, [3], 20, ("mag1c", "prob"), ring_stats=ring, ring_quantiles=rq, plume_quantiles=pq)
    cols = list(both.columns)
    assert cols.index("snr") < cols.index("mag1c_p5") < cols.index("mag1c_p99.9") < cols.index("prob_mean")
    with pytest.raises(ValueError):
        plumes.table_from_stats(st, [3], 20, (), plume_quantiles=pq)


def test_table_without_the_new_inputs_is_byte_identical():
    st, ring, _ = _case()
    for kw in [{}, {"ring_stats": ring}, {"ring_stats": ring, "pixel_area_m2": 900.0}]:
        a = plumes.table_from_stats(st, [3], 20, ("mag1c",), **kw)
        b = plumes.table_from_stats(st, [3], 20, ("mag1c",), ring_quantiles=None, plume_quantiles=None, **kw)
        assert a.equals(b) and a.to_csv(index=False) == b.to_csv(index=False)
    t = plumes.table_from_stats(st, [3], 20, ("mag1c",), ring_stats=ring, pixel_area_m2=900.0)
    assert list(t.columns)[-4:] == ["bg_px", "mag1c_bg_mean", "mag1c_sum_bgsub", "ime_bgsub_ppmm_m2"]
    assert np.array_equal(t["mag1c_sum_bgsub"], [900.0 - 20.0 * 4, np.nan, 10.0 - 3.0 * 2], equal_nan=True)


def test_oracle_on_hand_derived_cases():
    lab = np.array([[1, 1, 1, 2], [1, 0, 2, 2], [3, 3, 0, 5]], np.int32)
    plane = np.array([[4.0, -1.0, np.nan, 7.0], [2.0, 9.0, np.inf, -3.0], [np.nan, np.nan, 0.0, 1.0]], np.float32)
    nf, qs = cq.oracle(lab, [4], plane, (0, "median", 100, 25))
    assert nf.tolist() == [[3, 2, 0, 0]] and qs.dtype == np.float32 and qs.shape == (1, 4, 4)
    assert qs[0, 0].tolist() == [-1.0, 2.0, 4.0, 0.5] and qs[0, 1].tolist() == [-3.0, 2.0, 7.0, -0.5]
    assert np.isnan(qs[0, 2:]).all()                                                          # all NaN; a value no pixel carries
    nf, med, mad = cq.median_mad(lab, [4], plane)
    assert med[0, :2].tolist() == [2.0, 2.0] and mad[0, :2].tolist() == [2.0, 5.0] and nf.tolist() == [[3, 2, 0, 0]]
    # a centre that is not finite drops the whole row
    nf, qs = cq.oracle(lab, [2], plane, ("median",), center=np.array([[np.nan, 1.0]], np.float32))
    assert nf.tolist() == [[0, 2]] and np.isnan(qs[0, 0, 0]) and qs[0, 1, 0] == 5.0
    assert cq.same(np.array([0.0, np.nan], np.float32), np.array([-0.0, np.nan], np.float32))
    assert not cq.same(np.array([1.0], np.float32), np.array([np.nextafter(np.float32(1), np.float32(2))], np.float32))
