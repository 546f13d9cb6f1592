"""starcop_amd.quantify: the host side of the plume quantification (numpy only), and the validation of the ``plume_quantify=``
dict in starcop_amd.products.  No device involved."""
import numpy as np
import pytest

from starcop_amd import products, quantify as qf


def test_kg_per_ppmm_m2_is_the_ideal_gas_formula():
    assert qf.kg_per_ppmm_m2() == 1e-6 * 0.01604246 * 101325.0 / (8.314462618 * 288.15)
    assert qf.kg_per_ppmm_m2(300.0, 90000.0) == 1e-6 * 0.01604246 * 90000.0 / (8.314462618 * 300.0)
    assert abs(qf.kg_per_ppmm_m2() - 6.785e-7) < 1e-10          # 0.6785 g of methane per m2 in a 1000 ppm m column
    for bad in ((0.0, 101325.0), (288.15, -1.0), (float("nan"), 101325.0), (288.15, float("inf"))):
        with pytest.raises(ValueError):
            qf.kg_per_ppmm_m2(*bad)


def moments(mask):
    """the six integer sums of the pixels of a mask, as Python integers"""
    rr, cc = (v.astype(np.int64) for v in np.nonzero(mask))
    return [int(rr.size)], [int(rr.sum())], [int(cc.sum())], [int((rr * rr).sum())], [int((cc * cc).sum())], [int((rr * cc).sum())]


def eigh_shape(mask):
    """axes and orientation from numpy.linalg.eigh of the covariance of the pixel centres"""
    rr, cc = (v.astype(np.float64) for v in np.nonzero(mask))
    cov = np.cov(np.stack([rr, cc]), bias=True)
    w, v = np.linalg.eigh(cov)
    major, minor = 4.0 * np.sqrt(max(w[1], 0.0)), 4.0 * np.sqrt(max(w[0], 0.0))
    vr, vc = v[0, 1], v[1, 1]                       # the eigenvector of the larger eigenvalue, (row, col)
    if vr < 0 or (vr == 0 and vc < 0):
        vr, vc = -vr, -vc
    return major, minor, np.arctan2(vc, vr)


def rotated_rectangle(angle_deg, half_long=30.0, half_short=7.0, size=101):
    rr, cc = np.indices((size, size)).astype(np.float64) - size // 2
    t = np.deg2rad(angle_deg)
    along = rr * np.cos(t) + cc * np.sin(t)         # the long side makes `angle` with the row axis, towards increasing columns
    across = -rr * np.sin(t) + cc * np.cos(t)
    return (np.abs(along) <= half_long) & (np.abs(across) <= half_short)


@pytest.mark.parametrize("angle", [0.0, 25.0, 45.0, 80.0, -30.0, -75.0])
def test_shape_of_a_rotated_rectangle_against_eigh(angle):
    mask = rotated_rectangle(angle)
    major, minor, orient = (v[0] for v in qf.shape_from_moments(*moments(mask)))
    w_major, w_minor, w_orient = eigh_shape(mask)
    assert abs(major - w_major) <= 1e-9 * w_major and abs(minor - w_minor) <= 1e-9 * w_major
    assert abs(orient - w_orient) <= 1e-9
    assert abs(orient - np.deg2rad(angle)) < 0.03 and 55.0 < major < 75.0 and 13.0 < minor < 20.0


def test_shape_of_lines_squares_and_the_degenerate_rules():
    n = 17
    line = np.zeros((5, 40), bool)
    line[3, 4:4 + n] = True                         # 1 x n along the column axis: +pi/2, never -pi/2
    major, minor, orient = (v[0] for v in qf.shape_from_moments(*moments(line)))
    assert major == 4.0 * np.sqrt((n * n - 1) / 12.0) and minor == 0.0 and orient == np.pi / 2
    major, minor, orient = (v[0] for v in qf.shape_from_moments(*moments(line.T)))        # n x 1 along the row axis
    assert major == 4.0 * np.sqrt((n * n - 1) / 12.0) and minor == 0.0 and orient == 0.0
    square = np.zeros((30, 30), bool)
    square[5:16, 9:20] = True                       # isotropic: orientation 0, equal axes
    major, minor, orient = (v[0] for v in qf.shape_from_moments(*moments(square)))
    assert major == minor == 4.0 * np.sqrt((11 * 11 - 1) / 12.0) and orient == 0.0
    w_major, w_minor, _ = eigh_shape(square)
    assert abs(major - w_major) < 1e-12 and abs(minor - w_minor) < 1e-12
    single = np.zeros((4, 4), bool)
    single[2, 1] = True
    assert [v[0] for v in qf.shape_from_moments(*moments(single))] == [0.0, 0.0, 0.0]
    diag = np.eye(9, dtype=bool)                    # mu_rr == mu_cc: the sign of mu_rc decides
    assert qf.shape_from_moments(*moments(diag))[2][0] == np.pi / 4
    assert qf.shape_from_moments(*moments(diag[::-1]))[2][0] == -np.pi / 4
    assert qf.shape_from_moments(*moments(diag))[1][0] == 0.0
    empty = qf.shape_from_moments([0], [0], [0], [0], [0], [0])
    assert all(np.isnan(v[0]) for v in empty)
    # sums near 2^62: the products need more than 64 bits and stay exact
    big = qf.shape_from_moments([2 ** 30], [2 ** 44], [2 ** 44], [2 ** 58 + 2 ** 50], [2 ** 58 + 2 ** 50], [2 ** 58])
    assert big[0][0] == big[1][0] == 4.0 * np.sqrt(2.0 ** 20) and big[2][0] == 0.0
    several = qf.shape_from_moments(*[a + b for a, b in zip(moments(line), moments(square))])
    assert several[0].shape == (2,) and several[2].tolist() == [np.pi / 2, 0.0]


def test_fetch_profile_is_the_cumulative_sum_without_the_overflow_bin():
    cnt = np.array([[1, 2, 0, 4, 9], [0, 0, 3, 0, 0]])
    s = np.array([[1.5, 2.0, 0.0, -4.0, 100.0], [0.0, 0.0, 6.0, 0.0, 7.0]])
    p = qf.fetch_profile(cnt, s)
    assert p["n"].tolist() == [[1, 3, 3, 7], [0, 0, 3, 3]] and p["sum"].tolist() == [[1.5, 3.5, 3.5, -0.5], [0, 0, 6, 6]]
    assert p["sum_bgsub"] is None and p["n"].dtype == np.float64
    p = qf.fetch_profile(cnt, s, np.array([0.5, np.nan]))
    assert p["sum_bgsub"][0].tolist() == [1.0, 2.0, 2.0, -4.0] and np.isnan(p["sum_bgsub"][1]).all()
    with pytest.raises(ValueError):
        qf.fetch_profile(cnt, s[:, :4])
    with pytest.raises(ValueError):
        qf.fetch_profile(cnt, s, np.zeros(3))


def test_emission_rates_radius_selection():
    radii = np.array([10.0, 20.0, 30.0, 40.0, 50.0])
    prof = np.array([[1.0, 3.0, 6.0, 8.0, 8.0]] * 6)
    fetch_max = np.array([35.0, 30.0, 5.0, 500.0, np.nan, 0.0])
    out = qf.emission_rates(prof, radii, fetch_max, np.full(6, 400.0), np.full(6, 8.0), 2.0)
    q = 3600.0 * 2.0 * prof[0] / radii
    assert np.array_equal(out["q_kg_h"][0], q)
    # 35 m: 30 < 35 so the 40 m circle, the first that holds the plume, is the last one used; 30 m: the 30 m circle is
    assert out["used"].tolist() == [[True] * 4 + [False], [True] * 3 + [False] * 2, [True] + [False] * 4, [True] * 5, [False] * 5,
                                    [True] + [False] * 4]
    assert out["q_fetch_n"].tolist() == [4, 3, 1, 5, 0, 1] and out["q_fetch_n"].dtype == np.int64
    assert out["q_fetch_kg_h"][0] == q[:4].sum() / 4 and out["q_fetch_kg_h"][1] == q[:3].sum() / 3 and out["q_fetch_kg_h"][2] == q[0]
    assert out["q_fetch_std_kg_h"][0] == np.sqrt(((q[:4] - q[:4].sum() / 4) ** 2).sum() / 4) and out["q_fetch_std_kg_h"][2] == 0.0
    assert abs(out["q_fetch_std_kg_h"][3] - np.std(q)) < 1e-12 * np.std(q)
    assert np.isnan(out["q_fetch_kg_h"][4]) and np.isnan(out["q_fetch_std_kg_h"][4])                   # n == 0: NaN
    assert np.array_equal(out["q_sqrt_area_kg_h"], np.full(6, 3600.0 * 2.0 * 8.0 / 20.0))
    # min_fetch_m leaves the small circles out; beyond every used circle nothing is left
    out = qf.emission_rates(prof, radii, fetch_max, np.full(6, 400.0), np.full(6, 8.0), 2.0, min_fetch_m=20.0)
    assert out["q_fetch_n"].tolist() == [3, 2, 0, 4, 0, 0]
    assert out["q_fetch_kg_h"][0] == q[1:4].sum() / 3 and np.isnan(out["q_fetch_kg_h"][2]) and np.isnan(out["q_fetch_kg_h"][5])
    # a NaN inside the used part (no background) is not hidden, outside it is
    holed = prof.copy()
    holed[0, 1], holed[1, 4] = np.nan, np.nan
    out = qf.emission_rates(holed, radii, fetch_max, np.full(6, 400.0), np.full(6, 8.0), 2.0)
    assert np.isnan(out["q_fetch_kg_h"][0]) and out["q_fetch_n"][0] == 4 and out["q_fetch_kg_h"][1] == q[:3].sum() / 3
    for bad in (dict(radii_m=[10.0, 10.0, 30.0, 40.0, 50.0]), dict(radii_m=[0.0, 20.0, 30.0, 40.0, 50.0]), dict(radii_m=radii[:4]),
                dict(fetch_max_m=fetch_max[:5]), dict(wind_speed_m_s=[1.0, 2.0])):
        kw = dict(ime_profile_kg=prof, radii_m=radii, fetch_max_m=fetch_max, area_m2=np.full(6, 400.0), ime_kg=np.full(6, 8.0),
                  wind_speed_m_s=2.0)
        with pytest.raises(ValueError):
            qf.emission_rates(**{**kw, **bad})


def test_emission_rates_per_row_wind_speeds():
    radii = np.array([5.0, 10.0])
    prof = np.array([[2.0, 4.0], [2.0, 4.0], [2.0, 4.0]])
    wind = np.array([1.0, 2.5, 0.0])
    out = qf.emission_rates(prof, radii, np.full(3, 7.0), np.full(3, 100.0), np.full(3, 4.0), wind)
    one = qf.emission_rates(prof[:1], radii, [7.0], [100.0], [4.0], 1.0)
    for c in ("q_sqrt_area_kg_h", "q_fetch_kg_h", "q_fetch_std_kg_h"):
        assert np.array_equal(out[c], one[c][0] * wind), c
    assert out["q_fetch_n"].tolist() == [2, 2, 2] and out["q_fetch_kg_h"][0] == 3600.0 * (2.0 / 5.0 + 4.0 / 10.0) / 2


def test_radii_and_squared_edges():
    radii_m, radii_px = qf.radii_for({"wind_speed_m_s": 1.0}, 5.0)          # 150 m / 5 m: 30 circles
    assert radii_px.tolist() == list(range(1, 31)) and radii_m.tolist() == [5.0 * j for j in range(1, 31)]
    assert len(qf.radii_for({"wind_speed_m_s": 1.0}, 1.0)[0]) == 64                           # never more than 64
    assert qf.radii_for({"wind_speed_m_s": 1.0, "max_fetch_m": 61.0}, 60.0)[0].tolist() == [60.0]
    radii_m, radii_px = qf.radii_for({"wind_speed_m_s": 1.0, "radii_m": [7.5, 30.0]}, 5.0)
    assert radii_px.tolist() == [1.5, 6.0]
    for bad in ({"max_fetch_m": 59.0}, {"radii_m": []}, {"radii_m": [10.0, 10.0]}, {"radii_m": [-1.0]}, {"max_fetch_m": 0.0},
                {"radii_m": list(np.arange(1.0, 67.0) * 60)}):
        with pytest.raises(ValueError):
            qf.radii_for({"wind_speed_m_s": 1.0, **bad}, 60.0)
    assert qf.squared_edges([4.99, 5.0, 5.5], "t", 2 ** 31 - 2) == [24, 25, 30]              # floor(r^2), no epsilon
    for bad in ([], list(range(1, 66)), [1.0, 1.2], [2.0, 1.0], [0.0], [float("inf")], [2.0 ** 15.5]):
        with pytest.raises(ValueError):
            qf.squared_edges(bad, "t", 2 ** 31 - 2)


def test_plume_quantify_dict_validation():
    assert products.check_plume_quantify(None, "test") == {}
    q = {"wind_speed_m_s": 3.0, "max_fetch_m": 100.0, "min_fetch_m": 10.0, "temperature_k": 280.0, "pressure_pa": 9e4, "origin": "max"}
    assert products.check_plume_quantify(q, "test") == {"quantify": q}
    assert products.check_plume_quantify({"wind_speed_m_s": [1.0, 2.0], "origin": np.zeros((2, 2)), "origin_xy": True,
                                          "radii_m": [10.0, 20.0], "kg_per_ppmm_m2": 6.8e-7}, "test")["quantify"]["radii_m"] == [10.0, 20.0]
    for bad in ({}, {"max_fetch_m": 100.0}, {"wind_speed_m_s": 3.0, "u10": 1.0}, [3.0], 3.0, {"wind_speed_m_s": -1.0},
                {"wind_speed_m_s": float("nan")}, {"wind_speed_m_s": [[1.0]]}, {"wind_speed_m_s": 3.0, "origin": "upwind"},
                {"wind_speed_m_s": 3.0, "origin": np.zeros((3, 3))}, {"wind_speed_m_s": 3.0, "origin_xy": True},
                {"wind_speed_m_s": 3.0, "radii_m": [10.0], "max_fetch_m": 100.0}, {"wind_speed_m_s": 3.0, "min_fetch_m": -1.0},
                {"wind_speed_m_s": 3.0, "temperature_k": 0.0}, {"wind_speed_m_s": 3.0, "kg_per_ppmm_m2": 0.0},
                {"wind_speed_m_s": 3.0, "kg_per_ppmm_m2": 6.8e-7, "pressure_pa": 9e4}):
        with pytest.raises(ValueError):
            products.check_plume_quantify(bad, "test")
    with pytest.raises(ValueError):                 # before anything else is looked at, the device included
        products.annotate({}, np.zeros((4, 4), bool), None, None, plumes=True, plume_quantify={"wind_speed_m_s": 3.0, "u10": 1.0})
    with pytest.raises(ValueError, match="utm"):    # a grid without a pixel area (longitude / latitude)
        products.annotate({}, np.zeros((4, 4), bool), np.zeros((4, 4), np.float32), None, (-103.0, 5e-4, 0.0, 32.0, 0.0, -5e-4), None,
                          plumes=True, plume_quantify={"wind_speed_m_s": 3.0})


def test_quantify_columns_from_host_arrays():
    """the table columns from planted host arrays: one plume of two pixels, 4 m pixels, origin at its first pixel"""
    q = {"wind_speed_m_s": 2.0, "kg_per_ppmm_m2": 0.5}
    radial = {"bin_count": np.array([[1, 1, 0]]), "bin_sum": np.array([[3.0, 5.0, 0.0]]), "d2_max": np.array([1]),
              "sum_rr": np.array([2 * 49]), "sum_cc": np.array([9 + 16]), "sum_rc": np.array([21 + 28]), "origin": np.array([[7, 3]])}
    cols, curves = qf.quantify_columns(q, [4.0, 8.0], 4.0, np.array([2]), np.array([14]), np.array([7]), np.array([8.0]), np.array([2]), radial)
    assert list(cols) == list(qf.QUANTIFY_COLUMNS)
    assert (cols["origin_row"][0], cols["origin_col"][0], cols["fetch_max_m"][0]) == (7, 3, 4.0)
    assert (cols["major_axis_m"][0], cols["minor_axis_m"][0], cols["orientation_rad"][0]) == (4.0 * 0.5 * 4.0, 0.0, np.pi / 2)
    assert cols["ime_kg"][0] == 8.0 * 16.0 * 0.5 and curves["ime_kg"].tolist() == [[24.0, 64.0]]
    assert cols["q_sqrt_area_kg_h"][0] == 3600.0 * 2.0 * 64.0 / np.sqrt(32.0)
    assert cols["q_fetch_n"][0] == 1 and cols["q_fetch_kg_h"][0] == 3600.0 * 2.0 * 24.0 / 4.0 and cols["q_fetch_std_kg_h"][0] == 0.0
    ringed, _ = qf.quantify_columns(q, [4.0, 8.0], 4.0, np.array([2]), np.array([14]), np.array([7]), np.array([8.0]), np.array([2]), radial,
                                    bg_mean=np.array([1.0]))
    assert ringed["ime_kg"][0] == 6.0 * 16.0 * 0.5 and ringed["q_fetch_kg_h"][0] == 3600.0 * 2.0 * (2.0 * 16.0 * 0.5) / 4.0
    skipped = dict(radial, origin=np.array([[-1, -1]]), d2_max=np.array([-1]), bin_count=np.zeros((1, 3), np.int64), bin_sum=np.zeros((1, 3)))
    cols, _ = qf.quantify_columns(q, [4.0, 8.0], 4.0, np.array([2]), np.array([14]), np.array([7]), np.array([8.0]), np.array([2]), skipped)
    assert cols["origin_row"][0] == -1 and np.isnan(cols["fetch_max_m"][0]) and np.isnan(cols["q_fetch_kg_h"][0]) and cols["q_fetch_n"][0] == 0
    assert np.isnan(cols["major_axis_m"][0]) and cols["ime_kg"][0] == 64.0
