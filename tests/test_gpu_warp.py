"""The warp on the GPU (sc_warp through the C ABI, warp.source_coords, warp.reproject) against the numpy restatements of
tests/warp_util.py.  Coordinates within 1e-6 source pixels (fp64: an ulp at 10^7 m is 2e-9 m, a few hundred operations give at most
~1e-7 m = 1e-7 px at 1 m pixels; the gate leaves ten times that), nearest bit-equal outside the pixels whose restated (u, v) lies
within 1e-6 px of a cell boundary, bilinear within one float32 rounding doubled."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import warp_util as U  # noqa: E402
from hip_ops import DEV  # noqa: E402
from starcop_amd import _lib, warp  # noqa: E402

COORD_GATE_PX = 1e-6
TH = math.radians(17.0)
PX = 5.4e-4
#        name: (dst_shape, dst_gt, dst_crs, src_shape, src_gt, src_crs): offsets that look irrational keep pixel centres off cell boundaries
GRIDS = {
    "utm_over_geo": ((37, 53), (600123.37, 60.0, 0.0, 3590456.71, 0.0, -60.0), 32613,
                     (60, 90), (-103.94127, PX, 0.0, 32.45231, 0.0, -PX), 4326),
    "geo_over_utm": ((37, 53), (-103.93127, PX, 0.0, 32.44731, 0.0, -PX), 4326,
                     (50, 60), (600123.37, 60.0, 0.0, 3590856.71, 0.0, -60.0), 32613),
    "zone13_to_14": ((37, 53), (221003.37, 60.0, 0.0, 3590456.71, 0.0, -60.0), 32614,
                     (64, 90), (785011.13, 60.0, 0.0, 3590907.29, 0.0, -60.0), 32613),
    "south": ((37, 53), (368523.37, 60.0, 0.0, 6171956.71, 0.0, -60.0), 32721,
              (60, 90), (-58.43127, PX, 0.0, -34.58731, 0.0, -PX), 4326),
    "rotated17": ((37, 53), (499990.77, 5.0, 0.0, 4100050.31, 0.0, -5.0), 32611,
                  (40, 30), (500001.37, 5.0 * math.cos(TH), 5.0 * math.sin(TH), 4100002.71, 5.0 * math.sin(TH), -5.0 * math.cos(TH)), 32611),
    # a destination width that is a multiple of the vector (16-byte stores), more than one tile each way
    "vector": ((37, 72), (600123.37, 60.0, 0.0, 3590456.71, 0.0, -60.0), 32613,
               (60, 90), (-103.94127, PX, 0.0, 32.45231, 0.0, -PX), 4326),
    # the destination hangs over the source's left and upper edge: about half of it is outside
    "half_outside": ((37, 72), (598623.37, 60.0, 0.0, 3591756.71, 0.0, -60.0), 32613,
                     (60, 90), (-103.94127, PX, 0.0, 32.45231, 0.0, -PX), 4326),
    "all_outside": ((37, 53), (650123.37, 60.0, 0.0, 3590456.71, 0.0, -60.0), 32613,
                    (60, 90), (-103.94127, PX, 0.0, 32.45231, 0.0, -PX), 4326),
    "one_pixel": ((1, 1), (600923.37, 60.0, 0.0, 3589456.71, 0.0, -60.0), 32613,
                  (2, 2), (-103.92727, 20 * PX, 0.0, 32.44931, 0.0, -20 * PX), 4326),
}
NP_DTYPES = ("uint8", "int16", "float32", "float64")


@functools.lru_cache(maxsize=None)
def coords_ref(name):
    """the restated (u, v) of a case, clipped to the source; computed once, never modified"""
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    uv = U.source_coords_ref(ds, dgt, dcrs, sgt, scrs, ss)
    uv.setflags(write=False)
    return uv


def compared(name):
    """the pixels that take part in a comparison: all but those within 1e-6 px of a cell boundary; at most 0.1 % may be left out
    (asserted on the restatement alone; with these geotransforms none is)"""
    near = U.near_boundary(coords_ref(name))
    assert near.mean() <= 1e-3, (name, near.mean())
    return ~near


def source_planes(name, dt, P, seed=0):
    """(P, Hs, Ws) seeded planes of dtype dt; floats carry NaNs with payloads, -0.0 and infinities"""
    Hs, Ws = GRIDS[name][3]
    rng = np.random.default_rng(seed)
    nd = np.dtype(dt)
    if nd.kind == "f":
        a = rng.standard_normal((P, Hs, Ws)).astype(nd) * 100
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=max(4, flat.size // 20), replace=False)
        flat[idx[0::4]] = np.nan
        flat[idx[1::4]] = -0.0
        flat[idx[2::4]] = np.inf
        u = flat.view(f"u{nd.itemsize}")
        u[idx[3::4]] = (np.array(np.nan, dtype=nd).view(f"u{nd.itemsize}") | 0x1234)      # a NaN with a payload
        return a
    info = np.iinfo(nd)
    return rng.integers(info.min, info.max, size=(P, Hs, Ws), endpoint=True).astype(nd)


def nodata_for(dt, P):
    if np.dtype(dt).kind == "f":
        return [(-9999.0, float("nan"), -0.0)[p % 3] for p in range(P)]
    return [{"uint8": (255, 0, 7), "int16": (-9999, 0, 32767)}[dt][p % 3] for p in range(P)]


def check_nearest(got, planes, name, nodata, what):
    want = U.nearest_ref(planes, coords_ref(name), nodata)
    keep = compared(name)
    bad = U.mismatching_bytes(got[:, keep], want[:, keep])
    print(f"{what}: {got.dtype} {got.shape}, {int((~keep).sum())} pixels left out, mismatching bytes {bad} of {want[:, keep].nbytes}")
    assert got.dtype == want.dtype and got.shape == want.shape and bad == 0, what


def reproject(name, data, **kw):
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    return warp.reproject(data, sgt, scrs, dgt, dcrs, ds, **kw)


# ------------------------------------------------------------------------------------------------ coordinates
@pytest.mark.parametrize("name", ["utm_over_geo", "geo_over_utm", "zone13_to_14", "south", "rotated17", "vector", "half_outside"])
def test_source_coords(hip, name):
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    got = warp.source_coords(ds, dgt, dcrs, sgt, scrs, src_shape=ss)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,) + ds and got.is_cuda
    got, want = got.cpu().numpy(), coords_ref(name)
    nan = np.isnan(want[0])
    assert np.array_equal(np.isnan(got[0]), nan) and np.array_equal(np.isnan(got[1]), nan), name
    err = float(np.abs(got - want)[:, ~nan].max())
    print(f"{name}: {nan.mean():.1%} outside, max |(u, v) - restatement| = {err:.3g} px")
    assert not nan.all() and err <= COORD_GATE_PX
    if name in ("utm_over_geo", "geo_over_utm", "zone13_to_14"):
        assert not nan.any()                                              # the source covers these destinations
    # without a source shape nothing is clipped: the projection places every point of these grids
    free = warp.source_coords(ds, dgt, dcrs, sgt, scrs).cpu().numpy()
    ref = U.source_coords_ref(ds, dgt, dcrs, sgt, scrs)
    assert np.isfinite(free).all() and float(np.abs(free - ref).max()) <= COORD_GATE_PX
    assert np.array_equal(free[:, ~nan], got[:, ~nan])


def test_source_coords_outside_the_zone(hip):
    """more than 30 degrees from the central meridian there are no coordinates: NaN with and without a source shape"""
    dgt = (-140.0 + 0.123, 1.0, 0.0, 40.0, 0.0, -1.0)                     # 1 degree pixels from 140 W to 70 W; zone 13 is centred on 105 W
    got = warp.source_coords((2, 70), dgt, 4326, (500000.0, 1000.0, 0.0, 5000000.0, 0.0, -1000.0), 32613).cpu().numpy()
    ref = U.source_coords_ref((2, 70), dgt, 4326, (500000.0, 1000.0, 0.0, 5000000.0, 0.0, -1000.0), 32613)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and 0.1 < np.isnan(ref).mean() < 0.2
    assert float(np.nanmax(np.abs(got - ref))) <= COORD_GATE_PX


# ------------------------------------------------------------------------------------------------ nearest
@pytest.mark.parametrize("dt", NP_DTYPES)
@pytest.mark.parametrize("name", ["utm_over_geo", "vector", "half_outside", "all_outside", "one_pixel"])
def test_nearest_bit_equal(hip, name, dt):
    planes, nod = source_planes(name, dt, 3), nodata_for(dt, 3)
    got = reproject(name, torch.from_numpy(planes).to(DEV), nodata=nod)
    assert got.is_contiguous()
    check_nearest(got.cpu().numpy(), planes, name, nod, f"{name} {dt}")
    outside = np.isnan(coords_ref(name)[0])
    if name == "all_outside":
        assert outside.all()
    if name == "half_outside":
        assert 0.3 < outside.mean() < 0.7
    # numpy in, numpy out; a 2-D input gives a 2-D result
    one = reproject(name, planes[1], nodata=nod[1])
    assert isinstance(one, np.ndarray) and one.shape == GRIDS[name][0]
    check_nearest(one[None], planes[1:2], name, nod[1:2], f"{name} {dt} numpy 2-D")


@pytest.mark.parametrize("P", [1, warp.MAX_PLANES + 1])
def test_nearest_plane_counts(hip, P):
    planes, nod = source_planes("utm_over_geo", "float32", P, seed=P), nodata_for("float32", P)
    got = reproject("utm_over_geo", [torch.from_numpy(p).to(DEV) for p in planes], nodata=nod)
    check_nearest(got.cpu().numpy(), planes, "utm_over_geo", nod, f"P = {P}")


@pytest.mark.parametrize("dt", ["uint8", "float32"])
def test_nearest_interleaved_cube_in_place(hip, dt):
    planes = source_planes("vector", dt, 5, seed=9)
    cube = torch.from_numpy(np.ascontiguousarray(planes.transpose(1, 2, 0))).to(DEV)         # (Hs, Ws, 5), pixel-interleaved
    view = cube.permute(2, 0, 1)
    assert not view.is_contiguous() and view.stride(2) == 5
    nod = nodata_for(dt, 5)
    got = reproject("vector", view, nodata=nod)
    check_nearest(got.cpu().numpy(), planes, "vector", nod, f"interleaved {dt}")
    cols = reproject("vector", view[1:4], nodata=nod[1:4])                        # a slice of the planes
    check_nearest(cols.cpu().numpy(), planes[1:4], "vector", nod[1:4], f"interleaved {dt} [1:4]")


def call_abi(hip, name, src, dst, P=None, elem=None, mode=0, uv=None, **over):
    """one raw sc_warp call on a stacked (P, Hs, Ws) device tensor; returns the status code"""
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    a = _lib.sc_warp_args()
    inv = warp.invert_geotransform(sgt)
    for i in range(6):
        a.dst_gt[i], a.src_inv[i] = dgt[i], inv[i]
    a.dst_crs, a.src_crs = dcrs, scrs
    a.out_h, a.out_w = ds
    a.src_h, a.src_w = ss
    a.P = src.shape[0] if P is None else P
    a.elem_bytes = src.element_size() if elem is None else elem
    a.resampling = mode
    for p in range(min(max(a.P, 0), _lib.WARP_MAX_PLANES)):
        q = min(p, src.shape[0] - 1)
        a.src[p] = src[q].data_ptr()
        a.row_stride[p], a.col_stride[p] = src.stride(1), src.stride(2)
        a.nodata_bits[p] = 0
    a.out = dst.data_ptr() if dst is not None else None
    a.coords = uv.data_ptr() if uv is not None else None
    for k, v in over.items():                                              # any field of the struct, by name
        setattr(a, k, v)
    rc = hip.sc_warp(a, _lib.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dt", ["uint8", "float32", "float64"])
def test_nearest_misaligned_output_takes_the_scalar_variant(hip, dt):
    """the same (vector-width) case written into a view that is aligned to its elements only: equal to the aligned result"""
    name = "vector"
    planes = source_planes(name, dt, 2, seed=4)
    src = torch.from_numpy(planes).to(DEV)
    H, W = GRIDS[name][0]
    base = torch.zeros(2 * H * W + 1, dtype=src.dtype, device=DEV)
    out = base[1:].view(2, H, W)
    assert out.data_ptr() % 16 != 0 and out.data_ptr() % src.element_size() == 0
    assert call_abi(hip, name, src, out) == 0
    check_nearest(out.cpu().numpy(), planes, name, [0, 0], f"misaligned {dt}")
    aligned = torch.empty((2, H, W), dtype=src.dtype, device=DEV)
    assert aligned.data_ptr() % 16 == 0 and call_abi(hip, name, src, aligned) == 0
    assert U.mismatching_bytes(aligned.cpu().numpy(), out.cpu().numpy()) == 0


@pytest.mark.parametrize("dt", NP_DTYPES)
def test_identity_and_whole_pixel_shift(hip, dt):
    planes = source_planes("utm_over_geo", dt, 2, seed=2)
    Hs, Ws = planes.shape[1:]
    gt = GRIDS["utm_over_geo"][4]
    src = torch.from_numpy(planes).to(DEV)
    for crs in (4326, None, 1234):
        same = warp.reproject(src, gt, crs, gt, crs, (Hs, Ws), nodata=nodata_for(dt, 2))
        assert U.mismatching_bytes(same.cpu().numpy(), planes) == 0, crs        # the input bytes, NaN payloads and -0.0 included
    # a rotated grid onto itself
    rot = GRIDS["rotated17"][4]
    same = warp.reproject(src, rot, 32611, rot, 32611, (Hs, Ws))
    assert U.mismatching_bytes(same.cpu().numpy(), planes) == 0
    # shifted by (5, 7) whole pixels: a slice, and nodata where the destination leaves the source
    shifted = (gt[0] + 7 * gt[1], gt[1], 0.0, gt[3] + 5 * gt[5], 0.0, gt[5])
    nod = nodata_for(dt, 2)
    got = warp.reproject(src, gt, 4326, shifted, 4326, (Hs, Ws), nodata=nod).cpu().numpy()
    assert U.mismatching_bytes(got[:, :Hs - 5, :Ws - 7], planes[:, 5:, 7:]) == 0
    for p in range(2):
        fill = np.full((Hs, Ws), nod[p], dtype=planes.dtype)
        assert U.mismatching_bytes(got[p, Hs - 5:], fill[Hs - 5:]) == 0 and U.mismatching_bytes(got[p, :, Ws - 7:], fill[:, Ws - 7:]) == 0


# ------------------------------------------------------------------------------------------------ bilinear
def bilinear_plane(name, seed, kind):
    Hs, Ws = GRIDS[name][3]
    rng = np.random.default_rng(seed)
    if kind == "constant":
        a = np.full((Hs, Ws), 1234.5678, dtype=np.float32)
    else:
        a = (rng.standard_normal((Hs, Ws)) * 300 + 200).astype(np.float32)
    if kind != "dense":
        a[rng.random((Hs, Ws)) < 0.08] = -9999.0           # no-data holes
        a[rng.random((Hs, Ws)) < 0.04] = np.nan
        a[10:14, 20:31] = -9999.0
    return a


@pytest.mark.parametrize("name", ["utm_over_geo", "vector", "half_outside", "rotated17", "all_outside"])
@pytest.mark.parametrize("kind", ["holes", "dense", "constant"])
def test_bilinear(hip, name, kind):
    """against the float64 restatement rounded once to float32: |got - want| <= 2 * 2^-24 * max|x| (one float32 rounding, doubled for
    a last-place flip of the float64 quotient); the valid footprint is that of nearest on the same plane.  ``half_outside`` has the
    edge row and column, where the weights are renormalised over the samples inside."""
    plane = bilinear_plane(name, 11, kind)
    src = torch.from_numpy(plane).to(DEV)
    got = reproject(name, src, resampling="bilinear", nodata=-9999.0).cpu().numpy()
    near = reproject(name, src, resampling="nearest", nodata=-9999.0).cpu().numpy()
    want64, valid = U.bilinear_ref(plane, coords_ref(name), -9999.0)
    keep = compared(name)
    got_valid = got.view(np.uint32) != np.array(-9999.0, dtype=np.float32).view(np.uint32)
    near_valid = (near.view(np.uint32) != np.array(-9999.0, dtype=np.float32).view(np.uint32)) & ~np.isnan(near)
    assert not np.isnan(got).any()
    assert np.array_equal(got_valid[keep], valid[keep]) and np.array_equal(got_valid[keep], near_valid[keep]), "footprint"
    finite = plane[np.isfinite(plane) & (plane != -9999.0)]
    gate = 2 * 2.0 ** -24 * float(np.abs(finite).max())
    m = keep & valid
    err = float(np.abs(got[m].astype(np.float64) - want64[m].astype(np.float32).astype(np.float64)).max()) if m.any() else 0.0
    print(f"{name} {kind}: {valid.mean():.1%} valid, max |got - float32(restatement)| = {err:.3g} (gate {gate:.3g})")
    assert err <= gate
    if name == "all_outside":
        assert not valid.any()
    else:
        assert valid.any()
    if name == "half_outside":
        uv = coords_ref(name)
        edge = valid & ((uv[0] < 0.5) | (uv[1] < 0.5))                    # a neighbour beyond the first column / row: renormalised
        assert edge.sum() >= 10
    if kind == "constant":
        assert (got[got_valid] == np.float32(1234.5678)).all()            # exactly, wherever valid: keep or no keep


def test_bilinear_refuses_integers(hip):
    with pytest.raises(ValueError, match="bilinear"):
        reproject("utm_over_geo", torch.zeros(GRIDS["utm_over_geo"][3], dtype=torch.int16, device=DEV), resampling="bilinear")


# ------------------------------------------------------------------------------------------------ ABI, determinism
def test_abi_errors(hip):
    name = "utm_over_geo"
    Hs, Ws = GRIDS[name][3]
    H, W = GRIDS[name][0]
    s = torch.zeros((2, Hs, Ws), dtype=torch.float32, device=DEV)
    out = torch.empty((_lib.WARP_MAX_PLANES, H, W), dtype=torch.float32, device=DEV)
    coords = torch.empty((2, H, W), dtype=torch.float64, device=DEV)
    assert call_abi(hip, name, s, out) == 0
    assert call_abi(hip, name, s, out, P=_lib.WARP_MAX_PLANES) == 0
    assert call_abi(hip, name, s, None, P=0, uv=coords) == 0
    bad = ({"P": -1}, {"P": _lib.WARP_MAX_PLANES + 1}, {"P": 0},                              # P = 0 without coords: nothing to write
           {"elem": 3}, {"elem": 0}, {"elem": 16}, {"mode": 2}, {"mode": -1}, {"mode": 1, "elem": 8},
           {"dst_crs": 3857}, {"src_crs": 32661}, {"src_crs": 32700}, {"dst_crs": 0}, {"src_crs": 0}, {"dst_crs": -5, "src_crs": -5},
           {"out_h": 0}, {"out_w": -3}, {"src_h": 0}, {"src_w": -1}, {"out_h": 65536, "out_w": 32768},
           {"out": None}, {"out": out.data_ptr() + 2}, {"coords": coords.data_ptr() + 4}, {"oob_count": coords.data_ptr() + 4},
           {"flags": 2}, {"flags": 1})                                                        # unbounded coordinates only with P = 0
    for kw in bad:
        rc = call_abi(hip, name, s, out, **kw)
        assert rc == -1, kw
        with pytest.raises(ValueError, match="sc_warp"):
            _lib.check(rc)
    assert hip.sc_warp(None, _lib.stream()) == -1
    assert hip.sc_warp(_lib.sc_warp_args(), _lib.stream()) == -1         # everything zero
    a = _lib.sc_warp_args()

    def fresh():
        ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
        inv = warp.invert_geotransform(sgt)
        for i in range(6):
            a.dst_gt[i], a.src_inv[i] = dgt[i], inv[i]
        a.dst_crs, a.src_crs, a.P, a.elem_bytes, a.resampling, a.flags = dcrs, scrs, 1, 4, 0, 0
        (a.out_h, a.out_w), (a.src_h, a.src_w) = ds, ss
        a.src[0], a.row_stride[0], a.col_stride[0] = s.data_ptr(), Ws, 1
        a.out, a.coords, a.oob_count = out.data_ptr(), None, None
    fresh()
    assert hip.sc_warp(a, _lib.stream()) == 0
    a.src[0] = None
    assert hip.sc_warp(a, _lib.stream()) == -1                            # null source plane
    fresh(); a.src[0] = s.data_ptr() + 2
    assert hip.sc_warp(a, _lib.stream()) == -1                            # misaligned source
    fresh(); a.row_stride[0] = -Ws
    assert hip.sc_warp(a, _lib.stream()) == -1                            # negative strides
    fresh(); a.col_stride[0] = -1
    assert hip.sc_warp(a, _lib.stream()) == -1
    fresh(); a.dst_gt[1] = float("nan")
    assert hip.sc_warp(a, _lib.stream()) == -1                            # a geotransform that is not finite
    fresh(); a.src_inv[1] = a.src_inv[2] = 0.0
    assert hip.sc_warp(a, _lib.stream()) == -1                            # ... or singular
    fresh()
    assert hip.sc_warp(a, _lib.stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_two_calls_give_identical_bytes(hip, mode):
    planes = np.stack([bilinear_plane("half_outside", s, "holes") for s in (1, 2, 3)])
    src = torch.from_numpy(planes).to(DEV)
    a = reproject("half_outside", src, resampling=mode, nodata=-9999.0)
    b = reproject("half_outside", src, resampling=mode, nodata=-9999.0)
    assert U.mismatching_bytes(a.cpu().numpy(), b.cpu().numpy()) == 0
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS["half_outside"]
    c1, c2 = (warp.source_coords(ds, dgt, dcrs, sgt, scrs, src_shape=ss).cpu().numpy() for _ in range(2))
    assert U.mismatching_bytes(c1, c2) == 0


def test_reproject_like(hip, tmp_path):
    from starcop_amd import io_formats as io
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS["utm_over_geo"]
    path = str(tmp_path / "like.tif")
    io.write_tiff(path, np.zeros(ds, dtype=np.uint8), extra_tags=warp.geo_tags(dgt, dcrs))
    planes = source_planes("utm_over_geo", "int16", 2)
    got = warp.reproject_like(torch.from_numpy(planes).to(DEV), sgt, scrs, path, nodata=-1)
    check_nearest(got.cpu().numpy(), planes, "utm_over_geo", [-1, -1], "reproject_like a path")
    again = warp.reproject_like(torch.from_numpy(planes).to(DEV), sgt, scrs, io.tiff_info(path), nodata=-1)
    assert torch.equal(got, again)
    io.write_tiff(path, np.zeros(ds, dtype=np.uint8))
    with pytest.raises(ValueError, match="georeferencing"):
        warp.reproject_like(planes, sgt, scrs, path)
