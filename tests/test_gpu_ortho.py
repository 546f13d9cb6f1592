"""GLT orthorectification on the GPU (sc_glt_ortho through the C ABI, ortho.georeference, mag1c.mag1c_emit and the georeferenced /
out_folder arguments of the EMIT pipeline) against the numpy gather of tests/ortho_util.py: pure data movement, so every check is
equality of the raw bytes -- 100 % of the pixels, no tolerance."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ortho_util as U  # noqa: E402
from hip_ops import DEV  # noqa: E402
from starcop_amd import _lib, mag1c, model_module as mm, ortho, pipeline  # noqa: E402

NC = os.path.join(os.path.dirname(__file__), "golden", "io", "emit_l1b_like_sb0.nc")
DTYPES = ("float32", "float64", "uint8", "int16", "int32")


def fill_for(dt, i=0):
    if np.dtype(dt).kind == "f":
        return (-9999.0, float("nan"), -0.0)[i % 3]
    return {"uint8": (255, 0, 7), "int16": (-9999, 0, 32767), "int32": (-9999, 2 ** 31 - 1, 0)}[dt][i % 3]


def run(planes_np, gx, gy, fills, **kw):
    """stacked numpy planes -> device -> georeference -> numpy"""
    out = ortho.georeference(torch.from_numpy(np.ascontiguousarray(planes_np)).to(DEV), gx, gy, fill_value_default=fills, **kw)
    return out.cpu().numpy()


def check_equal(got, want, what):
    bad = U.mismatching_bytes(got, want)
    print(f"{what}: {got.dtype} {got.shape}, mismatching bytes {bad} of {got.nbytes}")
    assert bad == 0, what


def call_abi(hip, src, gx, gy, out, P=None, elem=None, oob=None, rows=None, cols=None, absolute=0):
    """one raw sc_glt_ortho call on a stacked (P, rows, cols) device tensor; returns the status code"""
    a = _lib.sc_ortho_args()
    a.glt_x, a.glt_y = gx.data_ptr(), gy.data_ptr()
    a.out_h, a.out_w = gx.shape
    a.rows, a.cols = (rows, cols) if rows is not None else src.shape[1:]
    a.P = src.shape[0] if P is None else P
    a.elem_bytes = src.element_size() if elem is None else elem
    a.absolute = absolute
    for p in range(min(max(a.P, 0), 64)):
        q = min(p, src.shape[0] - 1)
        a.src[p] = src[q].data_ptr()
        a.row_stride[p], a.col_stride[p] = src.stride(1), src.stride(2)
        a.fill_bits[p] = 0
    a.out = out.data_ptr()
    a.oob_count = oob.data_ptr() if oob is not None else None
    rc = hip.sc_glt_ortho(a, _lib.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dt", DTYPES)
def test_seeded_cases_are_bit_equal(hip, dt):
    rng = np.random.default_rng(17 + DTYPES.index(dt))
    f = fill_for(dt)
    # 1 x 1 grid
    src = U.random_source(rng, (1, 1), dt)
    one = np.ones((1, 1), np.int32)
    check_equal(run(src[None], one, one, f)[0], U.oracle(src, one, one, f), "1 x 1")
    check_equal(run(src[None], one * 0, one, f)[0], U.oracle(src, one * 0, one, f), "1 x 1, no data")
    # 37 x 53 output from a 19 x 23 source (odd width: the rows of the output do not start on 16-byte boundaries)
    src = U.random_source(rng, (19, 23), dt)
    gx, gy = U.random_glt(rng, (37, 53), 19, 23)
    check_equal(run(src[None], gx, gy, f)[0], U.oracle(src, gx, gy, f), "37 x 53 from 19 x 23")
    # 48 x 64 output (16-byte stores for every width), 2-D input and numpy in / numpy out
    gx, gy = U.random_glt(rng, (48, 64), 19, 23)
    got2d = ortho.georeference(torch.from_numpy(src).to(DEV), gx, gy, fill_value_default=f)
    assert got2d.shape == (48, 64)
    check_equal(got2d.cpu().numpy(), U.oracle(src, gx, gy, f), "48 x 64 from 19 x 23")
    host = ortho.georeference(src, gx, gy, fill_value_default=f)
    assert isinstance(host, np.ndarray)
    check_equal(host, U.oracle(src, gx, gy, f), "numpy in, numpy out")
    # all-zero GLT
    z = np.zeros((37, 53), np.int32)
    check_equal(run(src[None], z, z, f)[0], U.oracle(src, z, z, f), "all-zero GLT")
    # zero in only one of the two words
    gx, gy = U.random_glt(rng, (37, 52), 19, 23, p_nodata=0.0)
    gx[rng.random(gx.shape) < 0.3] = 0
    gy[rng.random(gy.shape) < 0.3] = 0
    assert ((gx == 0) != (gy == 0)).any()
    check_equal(run(src[None], gx, gy, f)[0], U.oracle(src, gx, gy, f), "zero in one word")
    # identity
    gx, gy = U.identity_glt(19, 23)
    got = run(src[None], gx, gy, f)[0]
    check_equal(got, U.oracle(src, gx, gy, f), "identity (oracle)")
    check_equal(got, src, "identity (source)")
    # absolute=True with signed entries
    gx, gy = U.random_glt(rng, (40, 56), 19, 23)
    sgx = gx * rng.choice([-1, 1], size=gx.shape).astype(np.int32)
    sgy = gy * rng.choice([-1, 1], size=gy.shape).astype(np.int32)
    check_equal(run(src[None], sgx, sgy, f, absolute=True)[0], U.oracle(src, sgx, sgy, f, absolute=True), "absolute, signed")
    check_equal(run(src[None], sgx, sgy, f, absolute=True)[0], U.oracle(src, gx, gy, f), "absolute == unsigned table")


def test_realistic_swath_is_bit_equal(hip):
    """1280 x 1242 swath -> 2000 x 2300 grid: rotated strip, no-data border, repeated source pixels; P = 5 float32 planes with
    one fill value each (NaN and -9999 among them)"""
    rng = np.random.default_rng(1280)
    gx, gy = U.swath_glt()
    assert gx.shape == (2000, 2300) and gx.max() == 1242 and gy.max() == 1280
    valid = gx != 0
    assert 0.3 < valid.mean() < 0.7 and valid.sum() > 1280 * 1242             # a border, and repeated source pixels
    src = U.random_source(rng, (5, 1280, 1242), "float32")
    fills = [-9999.0, float("nan"), -0.0, 1.5, -9999.0]
    got = run(src, gx, gy, fills)
    check_equal(got, U.oracle_planes(src, gx, gy, fills), "realistic swath, P = 5 float32")
    src8 = U.random_source(rng, (1280, 1242), "uint8")
    check_equal(run(src8[None], gx, gy, 255)[0], U.oracle(src8, gx, gy, 255), "realistic swath, uint8")
    src64 = U.random_source(rng, (1280, 1242), "float64")
    check_equal(run(src64[None], gx, gy, float("nan"))[0], U.oracle(src64, gx, gy, float("nan")), "realistic swath, float64")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("P", [1, 3, 5, 64])
def test_plane_counts_and_fill_values(hip, dt, P):
    rng = np.random.default_rng(100 * P + DTYPES.index(dt))
    src = U.random_source(rng, (P, 21, 34), dt)
    fills = [fill_for(dt, i) for i in range(P)]
    for shape in ((33, 48), (29, 45)):
        gx, gy = U.random_glt(rng, shape, 21, 34)
        want = U.oracle_planes(src, gx, gy, fills)
        check_equal(run(src, gx, gy, fills), want, f"stacked P = {P} {shape}")
        as_list = [torch.from_numpy(src[p].copy()).to(DEV) for p in range(P)]
        check_equal(ortho.georeference(as_list, gx, gy, fill_value_default=fills).cpu().numpy(), want, f"list P = {P} {shape}")


def test_more_planes_than_one_launch_takes(hip):
    rng = np.random.default_rng(70)
    src = U.random_source(rng, (70, 9, 11), "int16")
    gx, gy = U.random_glt(rng, (16, 24), 9, 11)
    fills = list(range(-35, 35))
    check_equal(run(src, gx, gy, fills), U.oracle_planes(src, gx, gy, fills), "P = 70 (two launches)")


@pytest.mark.parametrize("dt", DTYPES)
def test_layouts_are_read_in_place(hip, dt):
    rng = np.random.default_rng(40 + DTYPES.index(dt))
    f = fill_for(dt)
    gx, gy = U.random_glt(rng, (50, 64), 31, 27)
    # (rows, cols, 3) pixel-interleaved cube read through a permuted view
    cube = U.random_source(rng, (31, 27, 3), dt)
    t = torch.from_numpy(cube).to(DEV)
    view = t.permute(2, 0, 1)
    assert not view.is_contiguous() and view.data_ptr() == t.data_ptr()
    check_equal(ortho.georeference(view, gx, gy, fill_value_default=f).cpu().numpy(),
                U.oracle_planes(cube.transpose(2, 0, 1), gx, gy, [f] * 3), "pixel-interleaved (rows, cols, 3)")
    # three bands cut out of a wider interleaved cube, as a list of strided planes
    wide = U.random_source(rng, (31, 27, 9), dt)
    tw = torch.from_numpy(wide).to(DEV)
    check_equal(ortho.georeference([tw[..., b] for b in (7, 2, 4)], gx, gy, fill_value_default=f).cpu().numpy(),
                U.oracle_planes([wide[..., b] for b in (7, 2, 4)], gx, gy, [f] * 3), "bands of an interleaved cube")
    # non-contiguous column slice of a stacked tensor
    stack = U.random_source(rng, (3, 31, 40), dt)
    ts = torch.from_numpy(stack).to(DEV)
    sl = ts[:, :, 5:32]
    assert not sl.is_contiguous()
    check_equal(ortho.georeference(sl, gx, gy, fill_value_default=f).cpu().numpy(),
                U.oracle_planes(stack[:, :, 5:32], gx, gy, [f] * 3), "column slice")
    # a transposed plane (column stride = row length)
    tp = U.random_source(rng, (27, 31), dt)
    check_equal(ortho.georeference(torch.from_numpy(tp).to(DEV).t(), gx, gy, fill_value_default=f).cpu().numpy(),
                U.oracle(np.ascontiguousarray(tp.T), gx, gy, f), "transposed view")
    # planes smaller than the swath (the network output is cropped to multiples of 32): beyond a plane is no data
    full, crop = U.random_source(rng, (31, 27), dt), U.random_source(rng, (16, 24), dt)
    got = ortho.georeference([torch.from_numpy(full).to(DEV), torch.from_numpy(crop).to(DEV)], gx, gy, fill_value_default=f,
                             shape=(31, 27))
    check_equal(got.cpu().numpy(), U.oracle_planes([full, crop], gx, gy, [f, f], shape=(31, 27)), "cropped plane")
    # device GLT tensors are used as they are
    check_equal(ortho.georeference(torch.from_numpy(full).to(DEV), torch.from_numpy(gx).to(DEV), torch.from_numpy(gy).to(DEV),
                                   fill_value_default=f).cpu().numpy(), U.oracle(full, gx, gy, f), "device GLT")


def test_out_of_range_entries_are_filled_and_counted(hip):
    """entries beyond the swath never reach a load: the wrapper reports their number; with check=False the result is the oracle of
    the table with those entries marked no-data"""
    rng = np.random.default_rng(9)
    src = U.random_source(rng, (3, 19, 23), "float32")
    for shape in ((37, 53), (40, 64)):
        gx, gy = U.random_glt(rng, shape, 19, 23)
        bad = np.zeros(shape, bool)
        bad[3, 5] = bad[0, 0] = bad[shape[0] - 1, shape[1] - 1] = bad[11, 7] = bad[12, 9] = bad[20, 20] = True
        gx[3, 5], gy[3, 5] = 24, 1                      # gx = cols + 1
        gx[0, 0], gy[0, 0] = 1, 20                      # gy = rows + 1
        gx[-1, -1], gy[-1, -1] = 2 ** 31 - 1, 2 ** 31 - 1
        gx[11, 7], gy[11, 7] = -3, 4                    # negative without absolute
        gx[12, 9], gy[12, 9] = 5, -(2 ** 31)
        gx[20, 20], gy[20, 20] = 1000, 19
        with pytest.raises(ValueError, match=r"\b6 GLT entries"):
            run(src, gx, gy, -9999.0)
        cx, cy = gx.copy(), gy.copy()
        cx[bad] = 0
        cy[bad] = 0
        fills = [-9999.0, float("nan"), 2.0]
        check_equal(run(src, gx, gy, fills, check=False), U.oracle_planes(src, cx, cy, fills), f"out of range, check=False {shape}")
        # with absolute the entry (-3, 4) is valid; five remain
        with pytest.raises(ValueError, match=r"\b5 GLT entries"):
            run(src, gx, gy, -9999.0, absolute=True)     # -(2^31) has no absolute value in int32: still out of range
    # the raw counter through the C ABI
    g = torch.from_numpy(gx).to(DEV), torch.from_numpy(gy).to(DEV)
    s = torch.from_numpy(src).to(DEV)
    out = torch.empty((3,) + shape, dtype=torch.float32, device=DEV)
    oob = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert call_abi(hip, s, g[0], g[1], out, oob=oob) == 0 and int(oob.item()) == 6
    assert call_abi(hip, s, g[0], g[1], out, oob=None) == 0


def test_error_codes(hip):
    s = torch.zeros((2, 8, 8), dtype=torch.float32, device=DEV)
    gx = torch.ones((4, 4), dtype=torch.int32, device=DEV)
    out = torch.empty((64, 4, 4), dtype=torch.float32, device=DEV)
    assert call_abi(hip, s, gx, gx, out) == 0
    for kw in ({"P": 0}, {"P": 65}, {"P": -1}, {"elem": 3}, {"elem": 0}, {"elem": 16}, {"rows": 0, "cols": 8}, {"rows": 8, "cols": -2}):
        rc = call_abi(hip, s, gx, gx, out, **kw)
        assert rc == -1, kw
        with pytest.raises(ValueError, match="sc_glt_ortho"):
            _lib.check(rc)
    a = _lib.sc_ortho_args()
    assert hip.sc_glt_ortho(None, _lib.stream()) == -1
    assert hip.sc_glt_ortho(a, _lib.stream()) == -1                     # every pointer null
    a.glt_x = a.glt_y = gx.data_ptr()
    a.out = out.data_ptr()
    a.out_h = a.out_w = 4
    a.rows = a.cols = 8
    a.P, a.elem_bytes = 1, 4
    assert hip.sc_glt_ortho(a, _lib.stream()) == -1                     # null source plane
    a.src[0] = s.data_ptr()
    a.row_stride[0], a.col_stride[0] = 8, 1
    a.out_h = 0
    assert hip.sc_glt_ortho(a, _lib.stream()) == -1                     # bad output dims
    a.out_h = 4
    a.row_stride[0] = -8
    assert hip.sc_glt_ortho(a, _lib.stream()) == -1                     # negative stride
    a.row_stride[0] = 8
    a.plane_rows[0] = 9
    assert hip.sc_glt_ortho(a, _lib.stream()) == -1                     # plane larger than the swath
    a.plane_rows[0] = 0
    a.src[0] = s.data_ptr() + 2
    assert hip.sc_glt_ortho(a, _lib.stream()) == -1                     # misaligned source
    a.src[0] = s.data_ptr()
    assert hip.sc_glt_ortho(a, _lib.stream()) == 0
    torch.cuda.synchronize()


def test_mag1c_emit(hip):
    d = __import__("starcop_amd.hdf5_reader", fromlist=["x"]).read_emit_l1b(NC)
    wl, fw, raw, fill = d["wavelengths"], d["fwhm"], d["radiance"], d["fill_value"]
    keep = (wl >= 2122) & (wl <= 2488)
    templ = mag1c.generate_template_from_bands(wl[keep], fw[keep])
    for step in (None, 4):
        want_mf, want_alb = mag1c.mag1c_columns(torch.from_numpy(raw[..., keep]).to(DEV), templ[:, 1], fill, column_step=step)
        mf, alb = mag1c.mag1c_emit(raw, wl, fw, fill, georreferenced=False, column_step=step)
        assert mf.dtype == torch.float32 and mf.shape == raw.shape[:2]
        assert torch.equal(mf, want_mf) and torch.equal(alb, want_alb)
        gmf, galb = mag1c.mag1c_emit(torch.from_numpy(raw).to(DEV), wl, fw, fill, glt_x=d["glt_x"], glt_y=d["glt_y"], column_step=step)
        assert gmf.dtype == torch.float32 and gmf.shape == d["glt_x"].shape
        check_equal(gmf.cpu().numpy(), U.oracle(want_mf.cpu().numpy(), d["glt_x"], d["glt_y"], np.float32(fill)), "mag1c_emit mf")
        check_equal(galb.cpu().numpy(), U.oracle(want_alb.cpu().numpy(), d["glt_x"], d["glt_y"], np.float32(fill)), "mag1c_emit albedo")


GT = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)


def test_emit_granule_predict_georeferenced(hip, tmp_path):
    from starcop_amd import io_formats as io
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1)).to(DEV).eval()
    plain = pipeline.emit_granule_predict(model, NC, column_step=4, ratio_bands=(2350, 2310))
    geo = pipeline.emit_granule_predict(model, NC, column_step=4, ratio_bands=(2350, 2310), georeferenced=True)
    gx, gy, fill = plain["glt_x"], plain["glt_y"], plain["fill_value"]
    swath = tuple(plain["mf"].shape)
    assert swath == (40, 32) and gx.shape == (60, 70) and "files" not in geo
    for k in ("mf", "albedo", "prediction", "pred_binary", "ratio"):
        assert torch.equal(geo[k + "_raw"], plain[k]), k                  # today's outputs, under <key>_raw
        f = 0 if k == "pred_binary" else np.float32(fill)
        want = U.oracle_planes([plain[k].cpu().numpy()], gx, gy, [f], shape=swath)[0]
        assert geo[k].shape == (60, 70) and geo[k].dtype == plain[k].dtype
        check_equal(geo[k].cpu().numpy(), want, f"georeferenced {k}")
    assert torch.equal(geo["input"], plain["input"])
    rgb_want = U.oracle_planes(list(plain["input"][1:4].cpu().numpy()), gx, gy, [np.float32(fill)] * 3, shape=swath)
    check_equal(geo["rgb"].cpu().numpy(), rgb_want, "georeferenced rgb")
    # the same through emit_scene_predict
    d = __import__("starcop_amd.hdf5_reader", fromlist=["x"]).read_emit_l1b(NC)
    keep = (d["wavelengths"] >= 2122) & (d["wavelengths"] <= 2488)
    templ = mag1c.generate_template_from_bands(d["wavelengths"][keep], d["fwhm"][keep])
    scene = pipeline.emit_scene_predict(model, d["radiance"], d["wavelengths"], templ, fill_value=fill, column_step=4,
                                        ratio_bands=(2350, 2310), georeferenced=True, glt_x=gx, glt_y=gy)
    for k in ("mf", "albedo", "prediction", "pred_binary", "ratio", "rgb", "mf_raw", "pred_binary_raw"):
        assert torch.equal(scene[k], geo[k]), k

    # GeoTIFFs
    folder = str(tmp_path / "products")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        wrote = pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, out_folder=folder, geotransform=GT)
    assert not [w for w in rec if "geotransform" in str(w.message)]        # a geotransform is passed: nothing to warn about
    names = ["mag1c.tif", "albedo.tif", "pred.tif", "predbinary.tif", "rgb.tif"]
    assert sorted(os.path.basename(p) for p in wrote["files"]) == sorted(names)
    for name, key in zip(names, ("mf", "albedo", "prediction", "pred_binary", "rgb")):
        path = os.path.join(folder, name)
        assert os.path.exists(path), name
        a = io.read_tiff(path)
        want = geo[key].cpu().numpy()
        want = want if want.ndim == 3 else want[None]
        if key == "pred_binary":
            assert a.dtype == np.uint8 and np.array_equal(a, want.astype(np.uint8))
        else:
            assert a.dtype == np.float32
            check_equal(a, want, name)
        info = io.tiff_info(path)
        assert info.block == (128, 128) and info.bands == (3 if key == "rgb" else 1)
    info = io.tiff_info(os.path.join(folder, "mag1c.tif"))
    assert float(info.tags[42113][1][0]) == fill == -9999.0
    assert info.tags[33550][1] == (GT[1], -GT[5], 0.0) and info.tags[33922][1] == (0.0, 0.0, 0.0, GT[0], GT[3], 0.0)
    assert info.tags[34735][1][-1] == 4326
    xml = info.tags[42112][1][0]
    assert "CH4 Absorption (ppm x m)" in xml and '<Item name="mag1c">acrwl1mf</Item>' in xml
    assert "Albedo" in io.tiff_info(os.path.join(folder, "albedo.tif")).tags[42112][1][0]
    assert 42113 not in io.tiff_info(os.path.join(folder, "predbinary.tif")).tags
    # a second call skips what exists
    stamp = {n: os.stat(os.path.join(folder, n)).st_mtime_ns for n in names}
    os.remove(os.path.join(folder, "pred.tif"))
    again = pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, out_folder=folder, geotransform=GT)
    assert [os.path.basename(p) for p in again["files"]] == ["pred.tif"]
    assert all(os.stat(os.path.join(folder, n)).st_mtime_ns == stamp[n] for n in names if n != "pred.tif")
    assert pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, out_folder=folder, geotransform=GT)["files"] == []
    every = pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, out_folder=folder, geotransform=GT, overwrite=True)
    assert len(every["files"]) == 5
    # the fixture carries no geotransform attribute: without the argument the files are plain TIFFs and one warning says so
    bare = str(tmp_path / "bare")
    with pytest.warns(UserWarning, match="geotransform") as rec:
        pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, out_folder=bare)
    assert len([w for w in rec if "geotransform" in str(w.message)]) == 1
    info = io.tiff_info(os.path.join(bare, "mag1c.tif"))
    assert 33550 not in info.tags and 34735 not in info.tags and 42113 in info.tags
    check_equal(io.read_tiff(os.path.join(bare, "mag1c.tif"))[0], geo["mf"].cpu().numpy(), "mag1c.tif without georeferencing")
