"""The plane front-end of the raster operators (starcop_amd/planes.py): input forms and refusals, per-plane values, the strict and
the lenient fill pattern, and the filling of the argument structures.  Everything here is host code: no device, no library."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from starcop_amd import _lib, planes as PL


# ------------------------------------------------------------------------------------------------ as_planes
def test_as_planes_takes_the_four_forms():
    t2, t3 = torch.arange(12.0).reshape(3, 4), torch.arange(24.0).reshape(2, 3, 4)
    pl, single, host = PL.as_planes(t2, "f")
    assert (len(pl), single, host) == (1, True, False) and pl[0] is t2
    pl, single, host = PL.as_planes(t3, "f")
    assert (len(pl), single, host) == (2, False, False) and all(p.data_ptr() == t3[i].data_ptr() for i, p in enumerate(pl))
    pl, single, host = PL.as_planes([t2, t2 + 1], "f")
    assert (len(pl), single, host) == (2, False, False) and pl[0] is t2
    pl, single, host = PL.as_planes((t2,), "f")
    assert (len(pl), single, host) == (1, False, False)
    a3 = np.arange(24, dtype=np.int16).reshape(2, 3, 4)
    pl, single, host = PL.as_planes(a3, "f")
    assert (len(pl), single, host) == (2, False, True) and pl[1].dtype == torch.int16 and not pl[1].is_cuda
    assert pl[1].data_ptr() == a3[1].ctypes.data                        # the planes of a numpy array are views of it
    pl, single, host = PL.as_planes(a3[0], "f")
    assert (len(pl), single, host) == (1, True, True)


def test_as_planes_normalises_numpy_strides_and_uploads_nothing():
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    pl, _, host = PL.as_planes(a[:, ::-1, ::-1], "f")                   # negative strides: a contiguous copy, still on the host
    assert host and all(s >= 0 for p in pl for s in p.stride()) and not any(p.is_cuda for p in pl)
    assert np.array_equal(torch.stack(pl).numpy(), a[:, ::-1, ::-1])
    pl, _, _ = PL.as_planes(a[:, ::2, 1:], "f")                         # positive strides stay views
    assert pl[0].data_ptr() == a[0, 0, 1:].ctypes.data and pl[0].stride() == (8, 1)


def test_as_planes_reads_a_pixel_interleaved_cube_in_place():
    cube = torch.arange(3 * 4 * 5, dtype=torch.float32).reshape(3, 4, 5)            # (H, W, P)
    views = list(cube.permute(2, 0, 1).unbind(0))
    for data in (views, cube.permute(2, 0, 1)):
        pl, single, host = PL.as_planes(data, "f")
        assert len(pl) == 5 and not single and not host
        for k, p in enumerate(pl):
            assert p.data_ptr() == cube.data_ptr() + 4 * k and p.stride() == (20, 5) and tuple(p.shape) == (3, 4)


def test_as_planes_refusals():
    t = torch.zeros(3, 4)
    want = "^f: expected a tensor \\(H, W\\) or \\(P, H, W\\), a numpy array or a list of 2-D tensors, got "
    for bad, got in ((torch.zeros(2, 2, 3, 4), "\\(2, 2, 3, 4\\)"), (torch.zeros(3), "\\(3,\\)"), (torch.zeros(0, 3, 4), "\\(0, 3, 4\\)"),
                     (np.zeros((2, 2, 3, 4)), "\\(2, 2, 3, 4\\)"), ("scene.tif", "str"), (None, "NoneType")):
        with pytest.raises(ValueError, match=want + got + "$"):
            PL.as_planes(bad, "f")
    with pytest.raises(TypeError, match="^g: expected X, got dict$"):           # the caller's wording and exception type
        PL.as_planes({}, "g", "X", TypeError)
    with pytest.raises(ValueError, match="^g: expected X, got \\(3,\\)$"):       # a wrong shape is a ValueError for every caller
        PL.as_planes(torch.zeros(3), "g", "X", TypeError)
    for bad in ([], [t, torch.zeros(2, 3, 4)], [torch.zeros(3)]):
        with pytest.raises(ValueError, match="^f: a list must hold at least one 2-D tensor$"):
            PL.as_planes(bad, "f")
    with pytest.raises(ValueError, match="^f: all planes of a call share one dtype, device and shape$"):
        PL.as_planes([t, t.double()], "f")
    with pytest.raises(ValueError, match="^f: all planes of a call share one dtype, device and shape$"):
        PL.as_planes([t, torch.zeros(3, 5)], "f")
    with pytest.raises(ValueError, match="^f: all planes of a call share one dtype and device$"):
        PL.as_planes([t, t.double()], "f", same_shape=False)
    with pytest.raises(ValueError, match="^f: all planes of a call share one dtype and device$"):
        PL.as_planes([t, torch.zeros(3, 4, device="meta")], "f", same_shape=False)
    pl, _, _ = PL.as_planes([t, torch.zeros(2, 5)], "f", same_shape=False)       # shapes are the caller's business then
    assert [tuple(p.shape) for p in pl] == [(3, 4), (2, 5)]


def test_numpy_dtype():
    for dt in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float16, torch.float32, torch.float64):
        assert PL.numpy_dtype(dt, "f") == np.dtype(str(dt).replace("torch.", ""))
    for dt in (torch.bool, torch.complex64, torch.bfloat16):
        with pytest.raises(ValueError, match=f"^who: dtype {dt} is not supported \\(1-, 2-, 4- or 8-byte integers and floats\\)$"):
            PL.numpy_dtype(dt, "who")


# ------------------------------------------------------------------------------------------------ per-plane values
def test_per_plane():
    assert PL.per_plane(7, 3, "f", "fill values") == [7, 7, 7]
    assert PL.per_plane(None, 2, "f", "nodata values", default=0) == [0, 0]
    assert PL.per_plane(None, 2, "f", "fill values") == [None, None]
    assert PL.per_plane([1, 2, 3], 3, "f", "fill values") == [1, 2, 3]
    assert PL.per_plane((1.5, 2.5), 2, "f", "fill values") == [1.5, 2.5]
    assert PL.per_plane(np.array([4, 5]), 2, "f", "fill values") == [4, 5]
    assert PL.per_plane(np.float32(2.0), 2, "f", "fill values") == [2.0, 2.0]              # a numpy scalar is a scalar
    for n in (0, 2, 4):
        with pytest.raises(ValueError, match=f"^f: {n} nodata values for 3 planes$"):
            PL.per_plane(list(range(n)), 3, "f", "nodata values")
    with pytest.raises(ValueError, match="^g: 1 fill values for 2 planes$"):
        PL.per_plane(np.zeros(1), 2, "g", "fill values")


# a fill that is WRITTEN must be what np.full holds, or a ValueError; a fill that is only COMPARED is the same bits, or None when no
# element can equal it.  strict: bits (int) or "raises"; lenient: bits or None
NAN32, INF32 = 0x7FC00000, 0x7F800000
FILL_TABLE = [(0.5, "int16", "raises", None), (300, "uint8", "raises", None), (-1, "uint8", "raises", None),
              (float("nan"), "float32", NAN32, None),                  # written: numpy's NaN; compared: NaN equals nothing
              (float("nan"), "int32", "raises", None),
              (1e40, "float32", INF32, None),                          # written: what the conversion gives; compared: no float32 is 1e40
              (-9999.0, "float32", 0xC61C3C00, 0xC61C3C00), (-9999.0, "float64", 0xC0C3878000000000, 0xC0C3878000000000),
              (-9999.0, "int16", 0xD8F1, 0xD8F1), (-9999.0, "int32", 0xFFFFD8F1, 0xFFFFD8F1)]


@pytest.mark.parametrize("value, dtype, strict, lenient", FILL_TABLE)
def test_fill_bits_against_match_bits(value, dtype, strict, lenient):
    nd = np.dtype(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # numpy says that 1e40 overflows float32
        got_lenient = PL.match_bits(value, nd)
        if strict == "raises":
            with pytest.raises(ValueError, match=f"^who: fill value {value!r} cannot be represented in {dtype}$"):
                PL.fill_bits(value, nd, "who")
            assert got_lenient is None
            return
        got_strict = PL.fill_bits(value, nd, "who")
        held = np.full((1,), value, dtype=nd)
    assert got_strict == strict == int(held.view(f"u{nd.itemsize}")[0])
    assert got_lenient == lenient
    assert got_lenient is None or got_lenient == got_strict             # both agree bit for bit wherever both answer


# ------------------------------------------------------------------------------------------------ argument structures
class _Bare(ctypes.Structure):                 # as sc_warp_args holds its planes
    _fields_ = [("src", ctypes.c_void_p * 4), ("row_stride", ctypes.c_int64 * 4), ("col_stride", ctypes.c_int64 * 4)]


class _Sized(ctypes.Structure):                # as sc_ortho_args (plane_rows / plane_cols) and sc_wcut_args (rows / cols) do
    _fields_ = _Bare._fields_ + [("plane_rows", ctypes.c_int32 * 4), ("plane_cols", ctypes.c_int32 * 4)]


def test_chunks():
    assert PL.chunks(5, 4) == [(0, 4), (4, 1)] and PL.chunks(4, 4) == [(0, 4)] and PL.chunks(8, 4) == [(0, 4), (4, 4)]
    assert PL.chunks(1, 4) == [(0, 1)]
    assert PL.chunks(0, 4) == [(0, 0)]         # the warp's coordinate-only launch


@pytest.mark.parametrize("cls", [_Bare, _Sized])
def test_set_planes_across_a_chunk_boundary(cls):
    limit = 4
    cube = torch.zeros((6, 7, limit + 1), dtype=torch.int16)                       # P = limit + 1, pixel-interleaved
    views = [cube[: 6 - k, k:, k] for k in range(limit + 1)]                        # every plane its own pointer and shape
    seen = []
    for p0, n in PL.chunks(len(views), limit):
        a = cls()
        sized = {"rows": a.plane_rows, "cols": a.plane_cols} if cls is _Sized else {}
        assert PL.set_planes(a, views, p0, **sized) == n
        for k in range(limit):
            t = views[p0 + k] if k < n else None
            assert a.src[k] == (t.data_ptr() if k < n else None)
            assert (a.row_stride[k], a.col_stride[k]) == (t.stride() if k < n else (0, 0))
            if cls is _Sized:
                assert (a.plane_rows[k], a.plane_cols[k]) == (tuple(t.shape) if k < n else (0, 0))
        seen += [a.src[k] for k in range(n)]
    assert seen == [v.data_ptr() for v in views] and len(set(seen)) == limit + 1


def test_set_planes_fills_the_library_structures():
    t = torch.zeros((3, 5, 2))[:, :, 1]
    a = _lib.sc_ortho_args()
    assert PL.set_planes(a, [t, t], rows=a.plane_rows, cols=a.plane_cols) == 2
    assert (a.src[1], a.row_stride[1], a.col_stride[1], a.plane_rows[1], a.plane_cols[1]) == (t.data_ptr(), 10, 2, 3, 5)
    w = _lib.sc_wcut_args()
    assert PL.set_planes(w, [t], rows=w.rows, cols=w.cols) == 1 and (w.rows[0], w.cols[0], w.src[1]) == (3, 5, None)
    for cls in (_lib.sc_warp_args, _lib.sc_warp_area_args, _lib.sc_mosaic_source, _lib.sc_scene_planes_args):
        q = cls()
        assert PL.set_planes(q, [t]) == 1 and (q.src[0], q.row_stride[0], q.col_stride[0]) == (t.data_ptr(), 10, 2)
    many = [t] * (_lib.WARP_MAX_PLANES + 1)
    assert PL.set_planes(_lib.sc_warp_args(), many) == _lib.WARP_MAX_PLANES and PL.set_planes(_lib.sc_warp_args(), many, 32) == 1


@pytest.mark.parametrize("cls", [_lib.sc_wcut_args, _lib.sc_scene_planes_args])
def test_set_plane_ops(cls):
    a = cls()
    PL.set_plane_ops(a, 0, None, None, None)
    PL.set_plane_ops(a, 1, 0xC61C3C00, None, None)
    PL.set_plane_ops(a, 2, None, 0.1, None)
    PL.set_plane_ops(a, 3, 0, 1 / 3, (0.0, 2.0))
    assert [a.ops[k] for k in range(4)] == [0, _lib.WCUT_FILL, _lib.WCUT_SCALE, _lib.WCUT_FILL | _lib.WCUT_SCALE | _lib.WCUT_CLIP]
    assert (a.fill_bits[1], a.fill_bits[3]) == (0xC61C3C00, 0)
    assert a.scale[2] == float(np.float32(0.1)) and a.scale[3] == float(np.float32(1 / 3))
    assert (a.clip_lo[3], a.clip_hi[3]) == (0.0, 2.0)


def test_a_float_field_rounds_a_double_as_numpy_does():
    """set_plane_ops hands Python floats to float32 fields: the store must round them as ``np.float32(x)`` does, which is what the window
    cut asked for explicitly before.  Doubles of every kind: ties between two float32, the subnormal range, overflow, infinities, NaN."""
    rng = np.random.default_rng(7)
    with np.errstate(all="ignore"):
        u = rng.integers(0, 2 ** 64, size=20000, dtype=np.uint64).view(np.float64)            # every exponent, both signs, some NaN
        f = rng.integers(0, 2 ** 32, size=2000, dtype=np.uint64).astype(np.uint32).view(np.float32).astype(np.float64)
        ties = np.concatenate([f + np.spacing(f.astype(np.float32)).astype(np.float64) / 2, np.nextafter(f, np.inf), np.nextafter(f, -np.inf)])
        edge = np.array([0.0, -0.0, 1e40, -1e40, 3.4028235677973366e38, 3.4028234663852886e38, 1e-50, 7.0064923216240854e-46, 1.4e-45,
                         np.inf, -np.inf, np.nan, 0.1, 1 / 3, 2.0, 10000.0])
        xs = np.concatenate([u, f, ties, edge])
        want = xs.astype(np.float32)
    a = _lib.sc_wcut_args()
    got = np.empty(len(xs), np.float32)
    for i, x in enumerate(xs.tolist()):
        a.clip_lo[0] = x
        got[i] = a.clip_lo[0]
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.isnan(got[np.isnan(want)]).all()
