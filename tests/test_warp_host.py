"""The host side of the warp (starcop_amd.warp, io_formats.geo_from_tags): the Krueger series against Snyder's independent series, round
trips, zones, suggested grids, tags and polygons.  No device."""
import numpy as np
import pytest

import warp_util as U
from starcop_amd import io_formats as io, warp

# Measured with these 200 000 seeded points (profiles/warp_parity.txt): the largest distance between the Krueger series to n^6 and
# Snyder's series is 0.956 mm in northing and 0.279 mm in easting -- the truncation error of Snyder's series at 3.5 degrees from the
# central meridian, a property of the two series and not of rounding.  The gates are twice that (the margin covers another seed);
# a wrong coefficient of either series shows up at metres.
SNYDER_GATE_NORTHING_M = 2 * 0.956e-3
SNYDER_GATE_EASTING_M = 2 * 0.279e-3


def per_zone(fn, a, b, epsg, to_utm):
    x, y = np.empty_like(a), np.empty_like(a)
    for code in np.unique(epsg):
        m = epsg == code
        x[m], y[m] = fn(a[m], b[m], 4326, int(code)) if to_utm else fn(a[m], b[m], int(code), 4326)
    return x, y


@pytest.fixture(scope="module")
def points():
    lon, lat, lon0, epsg = U.seeded_points()
    e, n = per_zone(warp.transform_points, lon, lat, epsg, True)
    return lon, lat, lon0, epsg, e, n


def test_projection_against_snyder(points):
    lon, lat, lon0, epsg, e, n = points
    assert lon.size == 200_000 and np.isfinite(e).all() and np.isfinite(n).all()
    se, sn = U.snyder_forward(lon, lat, lon0, np.where(lat < 0, 10_000_000.0, 0.0))
    de, dn = float(np.abs(e - se).max()), float(np.abs(n - sn).max())
    print(f"Krueger n^6 vs Snyder 8-9..8-15: max |dE| = {de * 1e3:.4f} mm, max |dN| = {dn * 1e3:.4f} mm")
    assert de <= SNYDER_GATE_EASTING_M and dn <= SNYDER_GATE_NORTHING_M


def test_round_trips(points):
    lon, lat, lon0, epsg, e, n = points
    lo, la = per_zone(warp.transform_points, e, n, epsg, False)
    d_deg = max(float(np.abs(lo - lon).max()), float(np.abs(la - lat).max()))
    e2, n2 = per_zone(warp.transform_points, lo, la, epsg, True)
    d_m = max(float(np.abs(e2 - e).max()), float(np.abs(n2 - n).max()))
    print(f"forward -> inverse: {d_deg:.3g} degrees; inverse -> forward: {d_m:.3g} m")
    assert d_deg <= 1e-9 and d_m <= 1e-6


def test_zones_and_constants():
    e, n = warp.transform_points(-105.0, 0.0, 4326, 32613)                # the central meridian of zone 13 at the equator
    assert float(e) == 500000.0 and float(n) == 0.0
    e, n = warp.transform_points(-105.0, 0.0, 4326, 32713)                # the southern false northing
    assert float(e) == 500000.0 and float(n) == 10_000_000.0
    assert warp.utm_crs_for(-103.5, 31.9) == 32613
    assert warp.utm_crs_for(-103.5, -31.9) == 32713 and warp.utm_crs_for(179.9, 10) == 32660 and warp.utm_crs_for(-180.0, 10) == 32601
    # zone A -> zone B equals the route through longitude / latitude
    rng = np.random.default_rng(3)
    e13, n13 = rng.uniform(300e3, 700e3, 1000), rng.uniform(3.0e6, 4.5e6, 1000)
    e14, n14 = warp.transform_points(e13, n13, 32613, 32614)
    via = warp.transform_points(*warp.transform_points(e13, n13, 32613, 4326), 4326, 32614)
    assert np.array_equal(e14, via[0]) and np.array_equal(n14, via[1]) and np.isfinite(e14).all()
    assert float(np.abs(e14 - e13).min()) > 1e5                           # the zones are 6 degrees apart
    # beyond 30 degrees of the central meridian and past the poles there are no coordinates; same CRS is the identity
    x, y = warp.transform_points([-105.0 + 30.5, -105.0 + 29.5, -105.0], [10.0, 10.0, 91.0], 4326, 32613)
    assert np.isnan(x).tolist() == [True, False, True] and np.isnan(y).tolist() == [True, False, True]
    x, y = warp.transform_points([1.5, 2.5], [3.0, 4.0], 1234, 1234)
    assert x.tolist() == [1.5, 2.5] and y.tolist() == [3.0, 4.0] and x.dtype == np.float64
    with pytest.raises(NotImplementedError, match="3857"):
        warp.transform_points(0.0, 0.0, 4326, 3857)
    with pytest.raises(NotImplementedError, match="32661"):
        warp.transform_points(0.0, 0.0, 32661, 4326)


GT_GEO = (-104.03127, 5.4223e-4, 0.0, 32.51731, 0.0, -5.4223e-4)


def test_suggest_grid():
    shape = (211, 173)
    (H, W), gt = warp.suggest_grid(shape, GT_GEO, 4326, 32613, resolution=60.0)
    assert gt[1] == 60.0 and gt[5] == -60.0 and gt[2] == gt[4] == 0.0
    assert gt[0] % 60.0 == 0.0 and gt[3] % 60.0 == 0.0                    # the origin is a multiple of the resolution
    r, c = np.mgrid[0:shape[0], 0:shape[1]]
    x, y = warp.transform_points(*warp.apply_geotransform(GT_GEO, c + 0.5, r + 0.5), 4326, 32613)
    inv = warp.invert_geotransform(gt)
    u, v = inv[0] + x * inv[1] + y * inv[2], inv[3] + x * inv[4] + y * inv[5]
    assert u.min() >= 0 and u.max() < W and v.min() >= 0 and v.max() < H   # every source pixel centre is inside
    assert u.min() < 2 and v.min() < 2 and u.max() > W - 2 and v.max() > H - 2      # and the grid is not larger than it must be
    # an overlapping source: the lattices differ by whole pixels
    other = (GT_GEO[0] + 37.3 * GT_GEO[1], GT_GEO[1], 0.0, GT_GEO[3] - 51.7 * GT_GEO[1], 0.0, GT_GEO[5])
    _, gt2 = warp.suggest_grid((190, 201), other, 4326, 32613, resolution=60.0)
    for a, b in ((gt[0], gt2[0]), (gt[3], gt2[3])):
        assert (a - b) / 60.0 == round((a - b) / 60.0)
    # default resolution: the pixel count along the diagonal is kept
    (H3, W3), gt3 = warp.suggest_grid(shape, GT_GEO, 4326, 32613)
    assert 50.0 < gt3[1] < 61.0 and abs(np.hypot(H3, W3) / np.hypot(*shape) - 1) < 0.02
    # same CRS, rotated source -> north-up grid at its own pixel size
    th = np.radians(17.0)
    rot = (500000.0, 5 * np.cos(th), 5 * np.sin(th), 4100000.0, 5 * np.sin(th), -5 * np.cos(th))
    (H4, W4), gt4 = warp.suggest_grid((40, 30), rot, 32611, 32611, resolution=5.0)
    assert gt4[2] == gt4[4] == 0.0 and H4 * W4 > 40 * 30
    with pytest.raises(ValueError, match="2\\^31"):
        warp.suggest_grid((4000, 4000), GT_GEO, 4326, 32613, resolution=0.001)


@pytest.mark.parametrize("crs", [4326, 32613, 32721])
def test_geo_tags_round_trip(crs, tmp_path):
    gt = GT_GEO if crs == 4326 else (593940.0, 60.0, 0.0, 3598080.0, 0.0, -60.0)
    tags = warp.geo_tags(gt, crs)
    assert set(tags) == {33550, 33922, 34735}
    assert io.geo_from_tags(tags) == (tuple(gt), crs)
    path = str(tmp_path / "t.tif")
    io.write_tiff(path, np.zeros((5, 7), dtype=np.float32), extra_tags=tags)
    assert io.geo_from_tags(io.tiff_info(path)) == (tuple(gt), crs)
    # the key layouts are the ones the ENVI and EMIT paths write
    from starcop_amd.ortho import emit_geo_tags
    if crs == 4326:
        assert tags == emit_geo_tags(gt)
    else:
        zone, hemi = crs % 100, "North" if crs < 32700 else "South"
        hdr = {"map info": ["UTM", "1", "1", str(gt[0]), str(gt[3]), "60.0", "60.0", str(zone), hemi, "WGS-84", "units=Meters"]}
        assert tags == io.envi_geo_tags(hdr)


def test_geo_tags_rotated():
    hdr = {"map info": ["UTM", "1", "1", "500000.0", "4100000.0", "5.0", "5.0", "11", "North", "WGS-84", "units=Meters", "rotation=-12.0"]}
    want = io.envi_geo_tags(hdr)
    gt, epsg, rot = io.envi_geotransform(hdr)
    assert epsg == 32611 and rot == -12.0 and gt[2] != 0.0 and gt[4] != 0.0
    tags = warp.geo_tags(gt, epsg)
    assert tags == want and 34264 in tags and 33550 not in tags          # one sign convention: the tags envi_geo_tags writes
    assert io.geo_from_tags(tags) == (gt, 32611)
    assert io.geo_from_tags({}) == (None, None)
    assert 34735 not in warp.geo_tags(gt, None) and 34735 not in warp.geo_tags(gt, 3857)
    inv = warp.invert_geotransform(gt)
    x, y = warp.apply_geotransform(gt, 12.25, 31.5)
    assert abs(inv[0] + x * inv[1] + y * inv[2] - 12.25) < 1e-8 and abs(inv[3] + x * inv[4] + y * inv[5] - 31.5) < 1e-8


def test_transform_polygons():
    sq = np.array([[-104.0, 32.0], [-103.9, 32.0], [-103.9, 32.1], [-104.0, 32.1], [-104.0, 32.0]])
    hole = np.array([[-103.98, 32.02], [-103.95, 32.02], [-103.95, 32.05], [-103.98, 32.02]])
    polys = [[sq, hole], [sq + 0.2]]
    out = warp.transform_polygons(polys, 4326, 32613)
    assert [len(p) for p in out] == [2, 1]
    for rings_in, rings_out in zip(polys, out):
        for a, b in zip(rings_in, rings_out):
            assert b.shape == a.shape and np.array_equal(b[0], b[-1])      # closed rings stay closed
            x, y = warp.transform_points(a[:, 0], a[:, 1], 4326, 32613)
            assert np.array_equal(b[:, 0], x) and np.array_equal(b[:, 1], y)
    as_dict = warp.transform_polygons({7: [sq, hole], 9: [sq + 0.2]}, 4326, 32613)
    assert sorted(as_dict) == [7, 9] and np.array_equal(as_dict[7][1], out[0][1])
    back = warp.transform_polygons(out, 32613, 4326)
    assert max(float(np.abs(b - a).max()) for p, q in zip(polys, back) for a, b in zip(p, q)) < 1e-9
    with pytest.raises(ValueError, match="no coordinates"):
        warp.transform_polygons([[sq + 60.0]], 4326, 32613)
    with pytest.raises(NotImplementedError, match="3857"):
        warp.transform_polygons(polys, 4326, 3857)


def test_reproject_refusals():
    """what is refused before a device is needed"""
    a = np.zeros((4, 5), dtype=np.uint8)
    with pytest.raises(ValueError, match="bilinear"):
        warp.reproject(a, GT_GEO, 4326, GT_GEO, 4326, (4, 5), resampling="bilinear")
    with pytest.raises(NotImplementedError, match="3857"):
        warp.reproject(a, GT_GEO, 4326, GT_GEO, 3857, (4, 5))
    with pytest.raises(NotImplementedError, match="27700"):
        warp.reproject(a, GT_GEO, 27700, GT_GEO, 32613, (4, 5))
    with pytest.raises(ValueError, match="resampling"):
        warp.reproject(a, GT_GEO, 4326, GT_GEO, 4326, (4, 5), resampling="cubic")
    with pytest.raises(ValueError, match="singular"):
        warp.reproject(a, (0, 1, 0, 0, 2, 0), None, GT_GEO, None, (4, 5))
    with pytest.raises(ValueError, match="None"):
        warp.reproject(a, GT_GEO, None, GT_GEO, 4326, (4, 5))


def test_warp_args_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sc_warp_args as gcc lays it out == the ctypes mirror in _lib.py"""
    import ctypes
    import os
    import shutil
    import subprocess
    from starcop_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = ("src_inv", "dst_crs", "P", "flags", "src", "row_stride", "col_stride", "nodata_bits", "out", "coords", "oob_count")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){printf("%zu %d", sizeof(sc_warp_args), '
                   'SC_WARP_MAX_PLANES);' + "".join(f'printf(" %zu", offsetof(sc_warp_args, {f}));' for f in fields) + "return 0;}\n")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_lib.sc_warp_args), _lib.WARP_MAX_PLANES] + [getattr(_lib.sc_warp_args, f).offset for f in fields]
    assert got == want
