"""The host side of the Cloud-Optimized GeoTIFF writer, no GPU: io_formats.write_tiff_levels / tiff_info(ifd=) / tiff_ifd_count /
cog_layout_problems fed with tiles packed by the numpy restatement (tests/cog_util.py), libtiff (through Pillow) as a second
decoder, cog.overview_levels and the refusals of cog.write_cog that need no device."""
import os
import struct

import numpy as np
import pytest
import torch

import cog_util as U
from starcop_amd import cog, io_formats

BS = 16
GEO = {33550: (12, (5.0, 5.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0)), 34735: (3, (1, 1, 0, 1, 3072, 0, 1, 32611))}
ABSENT = (3, 1, 0)            # the absent tile of each level


def _pyramid_f32():
    """70 x 129 float32 with a nodata border, and its two overviews"""
    rng = np.random.default_rng(5)
    a = rng.normal(100.0, 30.0, size=(1, 70, 129)).astype(np.float32)
    a[:, :, :20] = -9999.0
    return [a] + U.pyramid(a, 2, "average", -9999.0)


def _write(path, imgs, predictor, nodata="-9999", absent=ABSENT, extra=GEO):
    levels = [(im.shape[1:], U.payloads(im, BS, predictor, absent=(absent[k],) if absent else ())) for k, im in enumerate(imgs)]
    tags = dict(extra)
    if nodata is not None:
        tags[42113] = (2, (nodata,))
    tags.update(io_formats.gdal_metadata_tag({}, ["band"]))
    return io_formats.write_tiff_levels(path, levels, imgs[0].dtype, bands=imgs[0].shape[0], blocksize=BS, predictor=predictor, extra_tags=tags)


def _with_absent(im, k, fill):
    """``im`` with tile ABSENT[k] replaced by the fill value: what a reader returns for the file"""
    out = im.copy()
    nbx = -(-im.shape[2] // BS)
    by, bx = divmod(ABSENT[k], nbx)
    out[:, by * BS:(by + 1) * BS, bx * BS:(bx + 1) * BS] = fill
    return out


@pytest.mark.parametrize("predictor", [1, 3])
def test_write_tiff_levels_three_level_pyramid(tmp_path, predictor):
    imgs = _pyramid_f32()
    assert [im.shape for im in imgs] == [(1, 70, 129), (1, 35, 65), (1, 18, 33)]
    p = str(tmp_path / "a.tif")
    size = _write(p, imgs, predictor)
    assert size == os.path.getsize(p)
    assert io_formats.cog_layout_problems(p) == []
    assert io_formats.tiff_ifd_count(p) == 3
    for k, im in enumerate(imgs):
        info = io_formats.tiff_info(p, ifd=k)
        assert (info.height, info.width) == im.shape[1:] and info.block == (BS, BS) and info.predictor == predictor and info.compression == 8
        assert info.tags[42113][1] == ("-9999",)
        assert (254 in info.tags) == (k > 0) and all((t in info.tags) == (k == 0) for t in (33550, 33922, 34735, 42112))
        assert info.offsets[ABSENT[k]] == 0 and info.counts[ABSENT[k]] == 0
        back = io_formats.read_tiff(p, info=info)
        assert U.same_bits(back, _with_absent(im, k, np.float32(-9999.0)))
        part = io_formats.read_tiff(p, window=(3, 5, 11, 20), info=info)
        assert U.same_bits(part, np.ascontiguousarray(_with_absent(im, k, np.float32(-9999.0))[:, 3:14, 5:25]))
    assert io_formats.tiff_info(p).height == 70                      # the default is the main image
    with pytest.raises(IndexError):
        io_formats.tiff_info(p, ifd=3)
    with pytest.raises(IndexError):
        io_formats.tiff_info(p, ifd=-1)


def test_write_tiff_levels_three_bands_and_single_tile(tmp_path):
    """3-band uint8 with predictor 2 down to a level of ONE tile (its offset sits in the IFD entry itself)"""
    a = U.byte_image(3, 40, 30, 9, values=200)
    imgs = [a] + U.pyramid(a, 2, "mode")
    assert imgs[-1].shape == (3, 10, 8)
    p = str(tmp_path / "b.tif")
    _write(p, imgs, 2, nodata=None, absent=None)
    assert io_formats.cog_layout_problems(p) == []
    for k, im in enumerate(imgs):
        assert np.array_equal(io_formats.read_tiff(p, info=io_formats.tiff_info(p, ifd=k)), im)
    assert io_formats.tiff_ifd_count(p) == 3 and io_formats.tiff_ifd_count(os.path.join(os.path.dirname(__file__), "golden", "io",
                                                                                           "tiled_f32_deflate_pred3.tif")) >= 1


def test_write_tiff_levels_refusals(tmp_path):
    a = np.zeros((1, 20, 20), np.float32)
    p = str(tmp_path / "c.tif")
    tiles = U.payloads(a, BS)
    with pytest.raises(ValueError):
        io_formats.write_tiff_levels(p, [((20, 20), tiles[:3])], np.float32, blocksize=BS)             # a tile is missing
    with pytest.raises(ValueError):
        io_formats.write_tiff_levels(p, [((20, 20), tiles), ((9, 10), [tiles[0]])], np.float32, blocksize=BS)      # not ceil(20 / 2)
    with pytest.raises(ValueError):
        io_formats.write_tiff_levels(p, [((20, 20), tiles)], np.float32, blocksize=BS, predictor=2)
    with pytest.raises(ValueError):
        io_formats.write_tiff_levels(p, [((20, 20), tiles)], np.float32, blocksize=24)

    class Huge(bytes):                                            # a payload that claims 3 GiB without holding it
        def __len__(self):
            return 3 << 30
    with pytest.raises(NotImplementedError):
        io_formats.write_tiff_levels(p, [((20, 20), [Huge(b"x")] * 4)], np.float32, blocksize=BS)


@pytest.mark.parametrize("dtype, predictor", [("float32", 3), ("float32", 1), ("uint8", 2), ("uint8", 1)])
def test_libtiff_decodes_every_frame(tmp_path, dtype, predictor):
    """Pillow's libtiff reads the tiles and the predictor of every IFD to the same array"""
    from PIL import Image, features
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff")
    golden = os.path.join(os.path.dirname(__file__), "golden", "io", "tiled_f32_deflate_pred3.tif")
    with Image.open(golden) as im:                                # the decoder itself, on a libtiff-written predictor-3 file
        assert np.array_equal(np.asarray(im), io_formats.read_tiff(golden)[0])
    if dtype == "float32":
        imgs = _pyramid_f32()
    else:
        a = U.byte_image(1, 70, 129, 3, values=200)
        imgs = [a] + U.pyramid(a, 2, "mode", 255)
    p = str(tmp_path / "d.tif")
    # every tile stored: this libtiff refuses a tile of byte count 0 ("Invalid tile byte count"); the sparse form is GDAL's, and
    # GDAL answers such a tile itself without asking libtiff.  read_tiff's handling of it is pinned in the tests above.
    _write(p, imgs, predictor, nodata="-9999" if dtype == "float32" else "255", absent=None)
    assert io_formats.cog_layout_problems(p) == []
    with Image.open(p) as im:
        assert im.n_frames == 3
        for k, want in enumerate(imgs):
            im.seek(k)
            got = np.asarray(im)
            assert got.dtype == want.dtype and U.same_bits(got, want[0])
            assert U.same_bits(io_formats.read_tiff(p, info=io_formats.tiff_info(p, ifd=k)), want)


# ------------------------------------------------------------------------------------------------ seeded defects
def _good(tmp_path):
    p = str(tmp_path / "good.tif")
    _write(p, _pyramid_f32(), 3)
    assert io_formats.cog_layout_problems(p) == []
    return p, io_formats._raw_ifds(p)[1]


def _patched(tmp_path, src, edits, tail=b""):
    data = bytearray(open(src, "rb").read())
    data += tail
    for pos, raw in edits:
        data[pos:pos + len(raw)] = raw
    p = str(tmp_path / "bad.tif")
    open(p, "wb").write(bytes(data))
    return p


def test_layout_overview_tile_behind_the_full_resolution(tmp_path):
    p, ifds = _good(tmp_path)
    e = ifds[1]["entries"]
    i = 2                                                          # a stored tile of overview 1
    off, cnt = e[324]["values"][i], e[325]["values"][i]
    size = os.path.getsize(p)
    size += size & 1
    tile = open(p, "rb").read()[off:off + cnt]
    bad = _patched(tmp_path, p, [(e[324]["value_offset"] + 4 * i, struct.pack("<I", size))], tail=(b"\0" if os.path.getsize(p) & 1 else b"") + tile)
    info = io_formats.tiff_info(bad, ifd=1)
    assert U.same_bits(io_formats.read_tiff(bad, info=info), io_formats.read_tiff(p, info=io_formats.tiff_info(p, ifd=1)))      # still a readable TIFF
    problems = io_formats.cog_layout_problems(bad)
    assert problems and any("tile data" in s for s in problems)


def test_layout_missing_new_subfile_type(tmp_path):
    p, ifds = _good(tmp_path)
    pos = ifds[2]["entries"][254]["pos"]
    bad = _patched(tmp_path, p, [(pos, struct.pack("<H", 255))])              # tag 254 -> 255 (SubfileType): the entries stay sorted
    problems = io_formats.cog_layout_problems(bad)
    assert len(problems) == 1 and "IFD 2" in problems[0] and "NewSubfileType" in problems[0]


def test_layout_wrong_overview_size(tmp_path):
    p, ifds = _good(tmp_path)
    pos = ifds[1]["entries"][256]["pos"]
    bad = _patched(tmp_path, p, [(pos + 8, struct.pack("<I", 66))])           # 65 -> 66 columns: the same tile grid
    problems = io_formats.cog_layout_problems(bad)
    assert any("IFD 1 is 35 x 66" in s for s in problems)


def test_layout_ifd_array_behind_the_first_tile(tmp_path):
    p, ifds = _good(tmp_path)
    e = ifds[1]["entries"][325]
    size = os.path.getsize(p)
    pad = b"\0" if size & 1 else b""
    table = open(p, "rb").read()[e["value_offset"]:e["value_offset"] + e["nbytes"]]
    bad = _patched(tmp_path, p, [(e["pos"] + 8, struct.pack("<I", size + len(pad)))], tail=pad + table)
    assert U.same_bits(io_formats.read_tiff(bad, info=io_formats.tiff_info(bad, ifd=1)), io_formats.read_tiff(p, info=io_formats.tiff_info(p, ifd=1)))
    problems = io_formats.cog_layout_problems(bad)
    assert len(problems) == 1 and "tag 325" in problems[0] and "behind the first tile" in problems[0]


def test_layout_of_a_plain_write_tiff_file(tmp_path):
    """a single-resolution tiled file is a (degenerate) conforming layout; a stripped file is not"""
    p = str(tmp_path / "plain.tif")
    io_formats.write_tiff(p, np.arange(40 * 50, dtype=np.float32).reshape(40, 50), blocksize=16)
    assert io_formats.cog_layout_problems(p) == [] and io_formats.tiff_ifd_count(p) == 1
    assert io_formats.cog_layout_problems(__file__) != []


# ------------------------------------------------------------------------------------------------ cog.py without a device
def test_overview_levels():
    assert cog.overview_levels(9000, 4000) == [(4500, 2000), (2250, 1000), (1125, 500), (563, 250), (282, 125)]
    assert cog.overview_levels(512, 512) == []
    assert cog.overview_levels(5, 300, min_size=64) == [(3, 150), (2, 75), (1, 38)]
    assert cog.overview_levels(513, 2) == [(257, 1)]


@pytest.mark.parametrize("image, kw", [
    (np.zeros((20, 20), np.float64), {}),
    (np.zeros((20, 20), np.uint16), {}),
    (torch.zeros((20, 20), dtype=torch.int32), {}),
    (np.zeros((5, 20, 20), np.float32), {}),
    (torch.zeros((5, 20, 20), dtype=torch.uint8), {}),
    (np.zeros((20, 20), np.float32), {"resampling": "mode"}),
    (np.zeros((20, 20), np.float32), {"blocksize": 24}),
    (torch.zeros((20, 20), dtype=torch.uint8), {"blocksize": 100}),
    (np.zeros((20, 20), np.float32), {"resampling": "cubic"}),
    (np.zeros((20, 20), np.float32), {"predictor": 2}),
    (np.zeros((20, 20), np.uint8), {"predictor": 3}),
    (np.zeros((20, 20), np.float32), {"nodata": -9999.0, "extra_tags": {42113: (2, ("0",))}}),
    (np.zeros((20, 20), np.uint8), {"nodata": 300}),
])
def test_write_cog_refusals_need_no_device(tmp_path, image, kw):
    """every refusal is a ValueError raised before anything touches a device -- also where there is one"""
    p = str(tmp_path / "never.tif")
    with pytest.raises(ValueError):
        cog.write_cog(p, image, **kw)
    assert not os.path.exists(p)


def test_write_cog_has_no_cpu_fallback(tmp_path):
    from starcop_amd._lib import StarcopHipError
    with pytest.raises(StarcopHipError):
        cog.write_cog(str(tmp_path / "cpu.tif"), torch.zeros((20, 20), dtype=torch.float32))          # a CPU tensor
    if not torch.cuda.is_available():
        with pytest.raises(StarcopHipError):
            cog.write_cog(str(tmp_path / "cpu.tif"), np.zeros((20, 20), np.float32))
    assert cog.default_workers() <= 16
