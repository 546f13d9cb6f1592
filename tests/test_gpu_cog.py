"""Cloud-Optimized GeoTIFFs on the GPU: sc_overview_reduce, sc_tiff_pack_tiles, sc_tiff_tile_flags, cog.write_cog and the ``cog=``
option of the scene pipelines against their numpy restatements (tests/cog_util.py), bit for bit."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cog_util as U  # noqa: E402
from hip_ops import DEV  # noqa: E402
from starcop_amd import cog, io_formats  # noqa: E402

SHAPES = [(131, 197), (129, 65), (5, 300), (64, 64)]
KINDS = [("float32", "average"), ("float32", "nearest"), ("uint8", "average"), ("uint8", "nearest"), ("uint8", "mode")]


def _layouts(a):
    """the same (nb, h, w) image as a dense tensor, as a permuted view of an (h, w, nb) interleaved buffer and as a transposed view
    of an (nb, w, h) one"""
    dense = torch.from_numpy(np.array(a)).to(DEV)
    inter = torch.from_numpy(np.array(np.moveaxis(a, 0, 2), order="C")).to(DEV).permute(2, 0, 1)
    trans = torch.from_numpy(np.array(np.swapaxes(a, 1, 2), order="C")).to(DEV).transpose(1, 2)
    assert inter.stride(2) == a.shape[0] and (a.shape[1] == 1 or trans.stride(1) == 1) and inter.shape == dense.shape == trans.shape
    return {"dense": dense, "interleaved": inter, "transposed": trans}


@functools.lru_cache(maxsize=None)
def _image(dtype, nb, shape, with_nodata):
    if dtype == "float32":
        a = U.float_image(nb, *shape, seed=31 + nb, nodata=0.0 if with_nodata else None)
    else:
        a = U.byte_image(nb, *shape, seed=41 + nb)
    a.setflags(write=False)
    return a


def _np(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def test_seeded_float_image_holds_what_the_tests_need():
    a = _image("float32", 1, (131, 197), True)
    b = U.bits(a)[0, :130, :196]
    valid = ((b & 0x7FFFFFFF) <= 0x7F800000) & (b != 0)
    n = valid[0::2, 0::2].astype(int) + valid[0::2, 1::2] + valid[1::2, 0::2] + valid[1::2, 1::2]
    assert set(np.unique(n)) == {0, 1, 2, 3, 4}
    assert np.isnan(a).any() and (U.bits(a) == 0x80000000).any() and (U.bits(a) == 0).any()
    mag = np.abs(a[np.isfinite(a) & (a != 0)])
    assert mag.min() < 2e-3 and mag.max() > 5e5
    neg0 = (U.bits(a)[0] == 0x80000000)
    assert (neg0[:, 1:] & (U.bits(a)[0][:, :-1] == 0)).any() or (neg0[:, :-1] & (U.bits(a)[0][:, 1:] == 0)).any()       # -0.0 next to the nodata 0.0
    u = _image("uint8", 1, (131, 197), True)[0, :130, :196]
    quad = np.stack([u[0::2, 0::2], u[0::2, 1::2], u[1::2, 0::2], u[1::2, 1::2]])
    srt = np.sort(quad, axis=0)
    assert ((srt[0] == srt[1]) & (srt[2] == srt[3]) & (srt[1] != srt[2])).any()                  # two against two: a mode tie


@pytest.mark.parametrize("with_nodata", [True, False])
@pytest.mark.parametrize("nb", [1, 3, 4])
@pytest.mark.parametrize("dtype, resampling", KINDS)
def test_overview_reduce_one_level(hip, dtype, resampling, nb, with_nodata):
    """one level, bit for bit, on every shape and every source layout"""
    nodata = 0 if with_nodata else None
    for shape in SHAPES:
        a = _image(dtype, nb, shape, with_nodata)
        want = U.reduce_level(a, resampling, nodata)
        for name, src in _layouts(a).items():
            got, = _np(cog.build_overviews(src, 1, resampling, nodata))
            assert U.same_bits(got, want), (shape, name, int((U.bits(got) != U.bits(want)).sum()))
    # -0.0 is a value, not the nodata 0.0
    if dtype == "float32" and resampling == "average" and with_nodata:
        x = np.array([[[-0.0, 0.0], [0.0, 0.0]]], dtype=np.float32)
        got, = _np(cog.build_overviews(torch.from_numpy(x).to(DEV), 1, "average", 0.0))
        assert U.bits(got).tolist() == [[[0x80000000]]]


@pytest.mark.parametrize("dtype, resampling, nb, nodata", [("float32", "average", 3, 0.0), ("float32", "average", 1, None),
                                                           ("uint8", "mode", 1, 0), ("uint8", "average", 4, None), ("float32", "nearest", 1, 0.0)])
def test_overview_fused_equals_chained(hip, dtype, resampling, nb, nodata):
    """(300, 517): the three levels of one launch == three launches of one level == the restatement; a five-level pyramid (two
    launches: 3 + 2 levels, down to a height of 10) == five steps of the restatement"""
    a = U.float_image(nb, 300, 517, 7, nodata=nodata) if dtype == "float32" else U.byte_image(nb, 300, 517, 8)
    src = torch.from_numpy(a).to(DEV)
    fused = cog.build_overviews(src, 3, resampling, nodata)
    chained, x = [], src
    for _ in range(3):
        x, = cog.build_overviews(x, 1, resampling, nodata)
        chained.append(x)
    want = U.pyramid(a, 5, resampling, nodata)
    assert [tuple(t.shape) for t in fused] == [(nb, 150, 259), (nb, 75, 130), (nb, 38, 65)]
    for k, (f, c) in enumerate(zip(_np(fused), _np(chained))):
        assert U.same_bits(f, c), k
        assert U.same_bits(f, want[k]), k
    five = _np(cog.build_overviews(src, cog.overview_levels(300, 517, min_size=17), resampling, nodata))
    assert len(five) == 5 and five[-1].shape == (nb, 10, 17)
    for k in range(5):
        assert U.same_bits(five[k], want[k]), k
    again = _np(cog.build_overviews(src, 5, resampling, nodata))
    assert all(U.same_bits(p, q) for p, q in zip(five, again))


def test_overview_refusals(hip):
    x = torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        cog.build_overviews(x, 1, "mode")
    with pytest.raises(ValueError):
        cog.build_overviews(x, [(4, 4), (3, 2)], "average")
    with pytest.raises(ValueError):
        cog.build_overviews(torch.zeros((5, 8, 8), device=DEV), 1, "average")
    assert cog.build_overviews(x, 0, "average") == []


# ------------------------------------------------------------------------------------------------ tiles
GUARD = 0xA5


def _pack(src, bs, predictor, slots_host, n_slots):
    """the call through a buffer of guard bytes with 32 of them on either side"""
    tile_bytes = bs * bs * src.shape[0] * src.element_size()
    n = n_slots * tile_bytes
    buf = torch.full((n + 64,), GUARD, dtype=torch.uint8, device=DEV)
    out = buf[32:32 + n].view(n_slots, tile_bytes)
    slots = torch.from_numpy(slots_host).to(DEV)
    got = cog.pack_tiles(src, bs, predictor, slots, slots_host, n_slots, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:32] == GUARD).all()) and bool((buf[32 + n:] == GUARD).all())
    return out.cpu().numpy()


def _write_tiff_tiles(tmp_path, a, bs):
    """the tile bytes io_formats.write_tiff builds, read back out of an uncompressed file"""
    p = str(tmp_path / "plain.tif")
    io_formats.write_tiff(p, a, blocksize=bs, compress=None)
    info = io_formats.tiff_info(p)
    raw = open(p, "rb").read()
    return [raw[o:o + c] for o, c in zip(info.offsets, info.counts)]


@pytest.mark.parametrize("nb", [1, 3, 4])
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_pack_tiles(hip, tmp_path, dtype, nb):
    bs = 16
    for shape in [(37, 50), (16, 16), (1, 17)]:
        a = U.float_image(nb, *shape, seed=51, nodata=-9999.0) if dtype == "float32" else U.byte_image(nb, *shape, seed=52, values=256)
        tiles = (-(-shape[0] // bs)) * (-(-shape[1] // bs))
        tile_bytes = bs * bs * nb * a.itemsize
        plain = U.pack_tiles(a, bs, 1)
        assert plain == _write_tiff_tiles(tmp_path, a, bs)
        # slots in reverse tile order, every third tile left out, one spare slot that no tile owns
        slots = np.full(tiles, -1, dtype=np.int32)
        kept = [t for t in range(tiles) if t % 3 != 1]
        for i, t in enumerate(reversed(kept)):
            slots[t] = i
        n_slots = len(kept) + 1
        info = io_formats.TiffInfo()
        info.dtype, info.compression, info.byteorder = np.dtype(a.dtype).newbyteorder("<"), 8, "<"
        padded = np.zeros((nb, -(-shape[0] // bs) * bs, -(-shape[1] // bs) * bs), a.dtype)
        padded[:, :shape[0], :shape[1]] = a
        for predictor in (1, 3 if dtype == "float32" else 2):
            want = U.pack_tiles(a, bs, predictor)
            for name, src in _layouts(a).items():
                got = _pack(src, bs, predictor, slots, n_slots)
                for t in range(tiles):
                    if slots[t] >= 0:
                        assert got[slots[t]].tobytes() == want[t], (shape, predictor, name, t)
                assert (got[n_slots - 1] == GUARD).all()                       # no tile owns it: untouched
            info.predictor = predictor
            nbx = -(-shape[1] // bs)
            for t in kept:                                                      # the decoder pinned on libtiff files undoes it
                px = io_formats._decode_block(zlib.compress(got[slots[t]].tobytes(), 6), info, bs, bs, nb)
                by, bx = divmod(t, nbx)
                assert U.same_bits(np.ascontiguousarray(np.moveaxis(px, 2, 0)), np.ascontiguousarray(padded[:, by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs]))
        # nothing to store: nothing is written
        none = _pack(torch.from_numpy(a).to(DEV), bs, 1, np.full(tiles, -1, dtype=np.int32), 1)
        assert (none == GUARD).all() and none.shape == (1, tile_bytes)


def test_pack_tiles_larger_blocks(hip):
    """128-pixel tiles of 4 float32 bands: a work-group stages 16 of the 128 tile rows at a time; 64-pixel uint8 tiles in one go"""
    for a, bs, predictor in [(U.float_image(4, 150, 130, 53, nodata=-9999.0), 128, 3), (U.byte_image(1, 70, 200, 54, values=256), 64, 2)]:
        want = U.pack_tiles(a, bs, predictor)
        slots = np.arange(len(want), dtype=np.int32)
        got = _pack(torch.from_numpy(a).to(DEV), bs, predictor, slots, len(want))
        assert all(got[t].tobytes() == want[t] for t in range(len(want)))


def test_pack_tiles_refusals(hip):
    x = torch.zeros((1, 20, 20), dtype=torch.float32, device=DEV)
    ok = np.array([0, 1, 2, 3], dtype=np.int32)
    out = torch.zeros((4, 1024), dtype=torch.uint8, device=DEV)
    for slots_host, n in [(np.array([0, 1, 1, 2], np.int32), 3), (np.array([0, 1, 2, 4], np.int32), 4), (np.array([0, -2, 1, 2], np.int32), 3)]:
        with pytest.raises(ValueError):
            cog.pack_tiles(x, 16, 1, torch.from_numpy(slots_host).to(DEV), slots_host, n, out=out)
    with pytest.raises(ValueError):                                   # the device table is not the checked one
        cog.pack_tiles(x, 16, 1, torch.from_numpy(ok[::-1].copy()).to(DEV), ok, 4, out=out)
    with pytest.raises(ValueError):                                   # the output is too small
        cog.pack_tiles(x, 16, 1, torch.from_numpy(ok).to(DEV), ok, 4, out=out[:3])
    with pytest.raises(ValueError):
        cog.pack_tiles(x, 16, 2, torch.from_numpy(ok).to(DEV), ok, 4, out=out)
    torch.cuda.synchronize()
    assert not out.any()


def test_tile_flags(hip):
    bs = 16
    nd = np.float32(-9999.0)
    a = np.full((2, 40, 37), nd, dtype=np.float32)                   # 3 x 3 tiles, the last row and column of tiles are edge tiles
    a[1, 15, 15] = 1.0                                               # tile 0: one other sample in its last pixel, second band
    a[0, 20, 36] = np.nan                                            # tile 5 (an edge tile): one other sample in its last in-image column
    b = a.copy()
    b[1, 15, 15] = nd
    for img, want in [(a, [0, 1, 1, 1, 1, 0, 1, 1, 1]), (b, [1, 1, 1, 1, 1, 0, 1, 1, 1])]:
        assert U.tile_flags(img, bs, -9999.0).tolist() == want
        for name, src in _layouts(img).items():
            assert cog.tile_flags(src, bs, -9999.0).cpu().tolist() == want, name
    # the padding of an edge tile is zero and does not count; without a nodata the fill is 0, and -0.0 is not 0.0
    assert cog.tile_flags(torch.from_numpy(a).to(DEV), bs).cpu().tolist() == [0] * 9
    z = np.zeros((1, 20, 33), dtype=np.float32)
    z[0, 3, 3] = -0.0
    z[0, 19, 32] = 5.0
    assert cog.tile_flags(torch.from_numpy(z).to(DEV), bs).cpu().tolist() == U.tile_flags(z, bs).tolist() == [0, 1, 1, 1, 1, 0]
    assert cog.tile_flags(torch.from_numpy(z).to(DEV), bs, 0.0).cpu().tolist() == [0, 1, 1, 1, 1, 0]
    u = np.zeros((3, 17, 16), dtype=np.uint8)
    u[2, 16, 15] = 7
    assert cog.tile_flags(torch.from_numpy(u).to(DEV), bs).cpu().tolist() == U.tile_flags(u, bs).tolist() == [1, 0]
    assert cog.tile_flags(torch.from_numpy(u).to(DEV), bs, 7).cpu().tolist() == U.tile_flags(u, bs, 7).tolist() == [0, 0]
    r = U.byte_image(3, 50, 70, 55, values=2)
    r[:, :32, 16:48] = 1
    assert cog.tile_flags(torch.from_numpy(r).to(DEV), bs, 1).cpu().tolist() == U.tile_flags(r, bs, 1).tolist()
    tiles, slots, flags = cog.pack_level(torch.from_numpy(r).to(DEV), bs, None, 1, True)
    assert flags.tolist() == U.tile_flags(r, bs, 1).tolist() and flags.sum() == 4
    assert slots.tolist() == np.where(flags == 0, np.cumsum(flags == 0) - 1, -1).tolist() and tiles.shape == (int((flags == 0).sum()), 16 * 16 * 3)


# ------------------------------------------------------------------------------------------------ write_cog
def _plane():
    a = np.random.default_rng(71).normal(300.0, 200.0, size=(300, 517)).astype(np.float32)
    y, x = np.mgrid[0:300, 0:517]
    a[(np.abs(x - (150 + 0.6 * y)) > 120)] = -9999.0             # a slanted strip of data, nodata around it
    return a


def _mask():
    y, x = np.mgrid[0:300, 0:517]
    return (((x - 200) ** 2 + (y - 140) ** 2 < 60 ** 2) | ((x // 7 + y // 5) % 11 == 0) & (x > 350)).astype(np.uint8)


def _rgb():
    a = np.random.default_rng(72).uniform(0.5, 12.0, size=(3, 300, 517)).astype(np.float32)
    a[:, _plane() == -9999.0] = -9999.0
    return a


CASES = {"plane": (_plane, -9999.0, "average"), "mask": (_mask, None, "mode"), "rgb": (_rgb, -9999.0, "average")}
GEO = {33550: (12, (5.0, 5.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0)), 34735: (3, (1, 1, 0, 1, 3072, 0, 1, 32611))}


def _tiles_of(path, ifd=0):
    """decompressed bytes of every stored tile of an IFD, None for an absent one"""
    info = io_formats.tiff_info(path, ifd=ifd)
    raw = open(path, "rb").read()
    return [None if c == 0 else zlib.decompress(raw[o:o + c]) for o, c in zip(info.offsets, info.counts)]


@pytest.mark.parametrize("predictor", [None, "auto"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_write_cog(hip, tmp_path, case, predictor):
    make, nodata, resampling = CASES[case]
    a = make()
    a3 = a if a.ndim == 3 else a[None]
    dev = torch.from_numpy(a).to(DEV)
    kw = dict(blocksize=16, overview_min_size=64, predictor=predictor, nodata=nodata, extra_tags=GEO)
    p = str(tmp_path / "a.tif")
    res = cog.write_cog(p, dev, **kw)
    assert io_formats.cog_layout_problems(p) == []
    want = [a3] + U.pyramid(a3, 4, resampling, nodata)
    assert [w.shape[1:] for w in want] == [(300, 517), (150, 259), (75, 130), (38, 65), (19, 33)]
    assert io_formats.tiff_ifd_count(p) == 5 and res["levels"] == 5
    flagged = 0
    for k, w in enumerate(want):
        info = io_formats.tiff_info(p, ifd=k)
        assert info.predictor == ({"float32": 3, "uint8": 2}[str(a.dtype)] if predictor == "auto" else 1)
        assert U.same_bits(io_formats.read_tiff(p, info=info), w), k             # level 0: the source itself
        flags = U.tile_flags(w, 16, nodata)
        assert [c == 0 for c in info.counts] == [bool(f) for f in flags], k          # absent = flagged, exactly
        flagged += int(flags.sum())
    for t, v in GEO.items():
        assert io_formats.tiff_info(p).tags[t][1] == v[1]
    assert (42113 in io_formats.tiff_info(p).tags) == (nodata is not None)
    assert res["tiles"] == sum(len(U.tile_flags(w, 16)) for w in want) and res["tiles_stored"] == res["tiles"] - flagged < res["tiles"]
    assert res["bytes_to_host"] == res["tiles_stored"] * 16 * 16 * a3.shape[0] * a.itemsize and res["bytes_written"] == os.path.getsize(p)
    # the same bytes again, from a numpy array, from another layout, and whatever the pool size
    ref = open(p, "rb").read()
    q = str(tmp_path / "b.tif")
    for image, extra in [(dev, {}), (a, {}), (dev, {"workers": 1}), (dev, {"workers": 4}), (_layouts(a3)["interleaved"], {})]:
        cog.write_cog(q, image, **kw, **extra)
        assert open(q, "rb").read() == ref
    # sparse=False stores every tile
    full = cog.write_cog(q, dev, sparse=False, **kw)
    assert full["tiles_stored"] == full["tiles"] == res["tiles"] and io_formats.cog_layout_problems(q) == []
    assert all(c > 0 for k in range(5) for c in io_formats.tiff_info(q, ifd=k).counts)
    assert U.same_bits(io_formats.read_tiff(q), a3)


@pytest.mark.parametrize("case", sorted(CASES))
def test_write_cog_single_level_has_the_tiles_of_write_tiff(hip, tmp_path, case):
    make, nodata, _ = CASES[case]
    a = make()
    p, q = str(tmp_path / "cog.tif"), str(tmp_path / "plain.tif")
    tags = {**GEO, **({42113: (2, ("-9999",))} if nodata is not None else {})}
    res = cog.write_cog(p, torch.from_numpy(a).to(DEV), blocksize=16, overviews=(), sparse=False, predictor=None, nodata=nodata, extra_tags=tags)
    io_formats.write_tiff(q, a, blocksize=16, extra_tags=tags)
    assert res["levels"] == 1 and io_formats.tiff_ifd_count(p) == 1 and io_formats.cog_layout_problems(p) == []
    assert _tiles_of(p) == _tiles_of(q) and None not in _tiles_of(p)
    ti, tq = io_formats.tiff_info(p), io_formats.tiff_info(q)
    assert {t: v for t, v in ti.tags.items() if t not in (324, 325)} == {t: v for t, v in tq.tags.items() if t not in (324, 325)}
    # uncompressed, and the default block size
    res = cog.write_cog(p, torch.from_numpy(a).to(DEV), compress=None, nodata=nodata, overview_min_size=256)
    info = io_formats.tiff_info(p)
    assert info.block == (128, 128) and info.compression == 1 and res["levels"] == 3 and io_formats.cog_layout_problems(p) == []
    a3 = a if a.ndim == 3 else a[None]
    assert U.same_bits(io_formats.read_tiff(p, info=info), a3)


# ------------------------------------------------------------------------------------------------ pipelines
def _geo(info):
    return {t: v for t, v in info.tags.items() if t in io_formats.GEO_TAGS}


def _same_product(cog_path, plain_path, min_ifds=2):
    assert io_formats.cog_layout_problems(cog_path) == []
    assert io_formats.tiff_ifd_count(cog_path) >= min_ifds and io_formats.tiff_ifd_count(plain_path) == 1
    ci, pi = io_formats.tiff_info(cog_path), io_formats.tiff_info(plain_path)
    assert U.same_bits(io_formats.read_tiff(cog_path, info=ci), io_formats.read_tiff(plain_path, info=pi))
    assert _geo(ci) == _geo(pi) != {}
    return ci


def _without_cog_module(call):
    """run ``call`` with starcop_amd.cog absent from sys.modules: the default path must not import it"""
    import starcop_amd
    saved = sys.modules.pop("starcop_amd.cog")
    attr = starcop_amd.__dict__.pop("cog", None)
    try:
        out = call()
        assert "starcop_amd.cog" not in sys.modules
    finally:
        sys.modules["starcop_amd.cog"] = saved
        if attr is not None:
            starcop_amd.cog = attr
    return out


def test_aviris_scene_predict_cog(hip, tmp_path):
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
    square = [[(500000.0 + 5.0 * 20, 4100000.0 - 5.0 * 10), (500000.0 + 5.0 * 40, 4100000.0 - 5.0 * 10), (500000.0 + 5.0 * 40, 4100000.0 - 5.0 * 30),
               (500000.0 + 5.0 * 20, 4100000.0 - 5.0 * 30), (500000.0 + 5.0 * 20, 4100000.0 - 5.0 * 10)]]
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32, label_polygons=[square])
    names = ["label.tif", "pred.tif", "predbinary.tif"]
    before = _without_cog_module(lambda: pipeline.aviris_scene_predict(model, folder, str(tmp_path / "a"), **kw))
    assert sorted(os.path.basename(p) for p in before["files"]) == names
    out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "c"), cog=dict(overview_min_size=64), **kw)
    assert sorted(os.path.basename(p) for p in out["files"]) == names
    for name in names:
        info = _same_product(str(tmp_path / "c" / name), str(tmp_path / "a" / name))
        assert info.block == (128, 128)
        over = io_formats.read_tiff(str(tmp_path / "c" / name), info=io_formats.tiff_info(str(tmp_path / "c" / name), ifd=1))
        key, nodata, how = {"pred.tif": ("prediction", S.FILL, "average"), "predbinary.tif": ("pred_binary", None, "mode"),
                            "label.tif": ("label_mask", None, "mode")}[name]
        assert U.same_bits(over, U.reduce_level(out[key].cpu().numpy()[None], how, nodata))
    assert out["label_mask"].any() and io_formats.tiff_info(str(tmp_path / "c" / "pred.tif")).tags[42113][1] == ("-9999",)
    # finer tiles: the empty ones are left out, and read back as nodata
    fine = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "f"), cog=dict(overview_min_size=64, blocksize=16), **kw)
    info = _same_product(str(tmp_path / "f" / "pred.tif"), str(tmp_path / "a" / "pred.tif"))
    assert 0 in info.counts and torch.equal(fine["prediction"], out["prediction"])
    # the default call after all of this: the bytes of the call made before cog.py was imported
    after = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "b"), **kw)
    for name in names:
        assert open(str(tmp_path / "b" / name), "rb").read() == open(str(tmp_path / "a" / name), "rb").read(), name
    assert torch.equal(after["prediction"], before["prediction"])


def test_cloud_mask_file_cog(hip, tmp_path):
    from starcop_amd import sentinel2
    from test_gpu_scene import _model
    model = _model()
    dn = np.random.default_rng(24).integers(0, 20000, size=(13, 70, 100)).astype(np.uint16)
    geo = {33550: (12, (10.0, 10.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 600000.0, 4500000.0, 0.0)), 34735: (3, (1, 1, 0, 1, 3072, 0, 1, 32633))}
    src_tif = str(tmp_path / "s2.tif")
    io_formats.write_tiff(src_tif, dn, extra_tags=geo)
    kw = dict(tile=32, halo=32, scale=1e-4)
    before = _without_cog_module(lambda: sentinel2.cloud_mask_file(src_tif, str(tmp_path / "a.tif"), model, **kw))
    mask = sentinel2.cloud_mask_file(src_tif, str(tmp_path / "c.tif"), model, cog=dict(overview_min_size=64), **kw)
    assert isinstance(mask, np.ndarray) and np.array_equal(mask, before) and len(np.unique(mask)) > 1
    info = _same_product(str(tmp_path / "c.tif"), str(tmp_path / "a.tif"))
    assert info.tags[42112] == io_formats.tiff_info(str(tmp_path / "a.tif")).tags[42112] and 42113 not in info.tags
    over = io_formats.read_tiff(str(tmp_path / "c.tif"), info=io_formats.tiff_info(str(tmp_path / "c.tif"), ifd=1))
    assert np.array_equal(over, U.reduce_level(mask[None], "mode"))
    sentinel2.cloud_mask_file(src_tif, str(tmp_path / "b.tif"), model, **kw)
    assert open(str(tmp_path / "b.tif"), "rb").read() == open(str(tmp_path / "a.tif"), "rb").read()


def test_emit_granule_predict_cog(hip, tmp_path):
    """every raster of the EMIT run (float32 planes, the 3-band rgb, the uint8 mask) as a COG: the pixels, the nodata and the
    georeferencing of the default files; the default files keep their bytes"""
    from starcop_amd import model_module as mm, pipeline
    nc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "io", "emit_l1b_like_sb0.nc")
    gt = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1)).to(DEV).eval()
    kw = dict(column_step=4, georeferenced=True, geotransform=gt)
    names = ["albedo.tif", "mag1c.tif", "pred.tif", "predbinary.tif", "rgb.tif"]
    before = _without_cog_module(lambda: pipeline.emit_granule_predict(model, nc, out_folder=str(tmp_path / "a"), **kw))
    assert sorted(os.path.basename(p) for p in before["files"]) == names
    H, W = before["pred_binary"].shape
    levels = 1 + len(cog.overview_levels(H, W, 32))
    assert levels >= 2
    out = pipeline.emit_granule_predict(model, nc, out_folder=str(tmp_path / "c"), cog=dict(overview_min_size=32, blocksize=16), **kw)
    assert sorted(os.path.basename(p) for p in out["files"]) == names
    for name in names:
        c, a = str(tmp_path / "c" / name), str(tmp_path / "a" / name)
        info = _same_product(c, a, min_ifds=levels)
        assert io_formats.tiff_ifd_count(c) == levels and info.tags.get(42113) == io_formats.tiff_info(a).tags.get(42113)
        assert info.tags[42112] == io_formats.tiff_info(a).tags[42112]
        full = io_formats.read_tiff(c, info=info)
        nodata = None if name == "predbinary.tif" else out["fill_value"]
        over = io_formats.read_tiff(c, info=io_formats.tiff_info(c, ifd=1))
        assert U.same_bits(over, U.reduce_level(full, "mode" if name == "predbinary.tif" else "average", nodata)), name
    pipeline.emit_granule_predict(model, nc, out_folder=str(tmp_path / "b"), **kw)
    for name in names:
        assert open(str(tmp_path / "b" / name), "rb").read() == open(str(tmp_path / "a" / name), "rb").read(), name
