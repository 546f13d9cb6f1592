"""On-disk formats of the STARCOP hot path, read without rasterio / GDAL / spectral (none of them is in the build image).

What the reference reads and writes on this path:
  * one single-band float32 (labels: uint8) cloud-optimised GeoTIFF per product per 512 x 512 sample folder --
    ``rasterio.open(f"{folder}/{product}.tif").read(window=window)`` in starcop/data/dataset.py:59-102, written by
    ``save_cog(v, path, profile={"BLOCKSIZE": 128})`` in starcop/data/sampling_dataset.py:332-355 -- and the mag1c / albedo
    outputs of starcop/process_aviris.py:209-232;
  * the AVIRIS-NG radiance cube and its GLT as ENVI files opened as BIP memmaps (``spectral.io.envi.open(hdr)
    .open_memmap(interleave='bip')``, process_aviris.py:183-187).

``read_tiff`` decodes classic (32-bit offset) TIFFs, tiled or stripped, 8/16/32/64-bit unsigned / signed / float samples,
chunky or planar multi-band, compression none / deflate / LZW with predictor 1, 2 or 3, either byte order, and reads only the
blocks a window touches (the first IFD = full resolution of a COG).  ``write_tiff`` writes tiled (BLOCKSIZE 128), deflate or
uncompressed files that carry the GeoTIFF tags handed to it, so a round trip keeps the georeferencing.  ``write_tiff_levels`` lays
finished tiles out as a Cloud-Optimized GeoTIFF (IFDs first, overviews, sparse tiles; ``starcop_amd.cog`` packs the tiles on the
device), ``tiff_info(path, ifd=k)`` / ``tiff_ifd_count`` reach its overviews and ``cog_layout_problems`` checks the layout rules.
``open_envi`` parses an
ENVI header and returns the cube as a (lines, samples, bands) memmap view plus wavelengths / fwhm.  ``load_tileset`` reads the
sample folders of a split into pinned host buffers and uploads them asynchronously into a ``ResidentTileSet``.
LZW and the predictors are undone by host C++ in libstarcop_hip.so (sc_tiff_lzw_decode / sc_tiff_unpredict): a Python loop
over LZW codes would take seconds per tile.
"""
import os
import re
import struct
import zlib
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2), 9: ("i", 4),
          10: ("ii", 8), 11: ("f", 4), 12: ("d", 8), 16: ("Q", 8)}
GEO_TAGS = (33550, 33922, 34264, 34735, 34736, 34737, 42112, 42113)       # pixel scale, tiepoints, transform, geo keys, GDAL metadata / nodata


class TiffInfo:
    def __init__(self):
        self.width = self.height = 0
        self.bands = 1
        self.dtype = np.dtype("uint8")
        self.block = (0, 0)            # (rows, cols) of a tile, or (rows_per_strip, width)
        self.tiled = False
        self.offsets = self.counts = ()
        self.compression, self.predictor, self.planar = 1, 1, 1
        self.byteorder = "<"
        self.tags: Dict[int, tuple] = {}           # raw values of every tag: {tag: (type, values)}

    def geo_tags(self):
        return {t: v for t, v in self.tags.items() if t in GEO_TAGS}


def _tiff_header(f, path):
    """-> (byte order, offset of the first IFD) of an open classic TIFF"""
    head = f.read(8)
    bo = {b"II": "<", b"MM": ">"}.get(head[:2])
    if bo is None:
        raise ValueError(f"{path}: not a TIFF file")
    magic, ifd = struct.unpack(bo + "HI", head[2:8])
    if magic == 43:
        raise NotImplementedError(f"{path}: BigTIFF is not supported (STARCOP samples are classic TIFFs of ~1 MB)")
    if magic != 42:
        raise ValueError(f"{path}: bad TIFF magic {magic}")
    return bo, ifd


def _ifd_offsets(f, path):
    """-> (byte order, [offset of every IFD of the chain])"""
    bo, off = _tiff_header(f, path)
    offs = []
    while off and len(offs) < 65536:
        if off in offs:
            raise ValueError(f"{path}: the IFD chain loops")
        offs.append(off)
        f.seek(off)
        n, = struct.unpack(bo + "H", f.read(2))
        f.seek(off + 2 + 12 * n)
        off, = struct.unpack(bo + "I", f.read(4))
    return bo, offs


def tiff_ifd_count(path) -> int:
    """number of IFDs (images: the full resolution and its overviews) of a TIFF file"""
    with open(path, "rb") as f:
        return len(_ifd_offsets(f, path)[1])


def tiff_info(path, ifd: int = 0) -> TiffInfo:
    """``ifd``: which image of the file (0 = the full resolution of a COG, k = its k-th overview); IndexError past the last"""
    with open(path, "rb") as f:
        if ifd == 0:
            bo, off = _tiff_header(f, path)
        else:
            bo, offs = _ifd_offsets(f, path)
            if not 0 <= ifd < len(offs):
                raise IndexError(f"{path}: IFD {ifd} of a file with {len(offs)}")
            off = offs[ifd]
        f.seek(off)
        n, = struct.unpack(bo + "H", f.read(2))
        raw = f.read(12 * n)
        info = TiffInfo()
        info.byteorder = bo
        for i in range(n):
            tag, typ, cnt, val = struct.unpack(bo + "HHI4s", raw[12 * i:12 * i + 12])
            if typ not in _TYPES:
                continue
            code, size = _TYPES[typ]
            nbytes = size * cnt
            if nbytes <= 4:
                data = val[:nbytes]
            else:
                off, = struct.unpack(bo + "I", val)
                pos = f.tell(); f.seek(off); data = f.read(nbytes); f.seek(pos)
            if typ == 2:
                vals = (data.rstrip(b"\0").decode("latin-1"),)
            else:
                vals = struct.unpack(bo + code[0] * (cnt * len(code)), data)
            info.tags[tag] = (typ, vals)
    t = info.tags

    def one(tag, default=None):
        return t[tag][1][0] if tag in t else default
    info.width, info.height = one(256), one(257)
    info.bands = one(277, 1)
    bits = t.get(258, (3, (1,)))[1]
    fmt = t.get(339, (3, (1,)))[1][0]
    if len(set(bits)) != 1:
        raise NotImplementedError(f"{path}: bands of different bit depth")
    kind = {1: "u", 2: "i", 3: "f"}.get(fmt)
    if kind is None or bits[0] not in (8, 16, 32, 64):
        raise NotImplementedError(f"{path}: sample format {fmt} with {bits[0]} bits")
    info.dtype = np.dtype(f"{bo}{kind}{bits[0] // 8}")
    info.compression, info.predictor, info.planar = one(259, 1), one(317, 1), one(284, 1)
    if 322 in t:
        info.tiled = True
        info.block = (one(323), one(322))
        info.offsets, info.counts = t[324][1], t[325][1]
    else:
        info.block = (min(one(278, info.height), info.height), info.width)
        info.offsets, info.counts = t[273][1], t[279][1]
    return info


def _decode_block(buf: bytes, info: TiffInfo, rows: int, cols: int, spp: int) -> np.ndarray:
    """one tile / strip -> (rows, cols, spp) array in native byte order"""
    n = rows * cols * spp * info.dtype.itemsize
    c = info.compression
    if c == 1:
        raw = buf
    elif c in (8, 32946):
        raw = zlib.decompress(buf)
    elif c == 5:
        from . import _lib
        raw = _lib.tiff_lzw_decode(buf, n)
    else:
        raise NotImplementedError(f"TIFF compression {c} (supported: none, deflate, LZW)")
    if len(raw) < n:
        raise ValueError(f"TIFF block decodes to {len(raw)} bytes, expected {n}")
    a = np.frombuffer(raw, dtype=np.uint8, count=n)
    if info.predictor == 3:          # floating-point predictor: bytes of a row are de-interleaved by significance and differenced
        from . import _lib
        a = _lib.tiff_unpredict(a, 3, rows, cols, spp, info.dtype.itemsize, info.byteorder == ">")
        return a.view(info.dtype.newbyteorder("=")).reshape(rows, cols, spp)
    a = a.view(info.dtype).reshape(rows, cols, spp).astype(info.dtype.newbyteorder("="))
    if info.predictor == 2:          # horizontal differencing, per sample, modular integer arithmetic
        if a.dtype.kind == "f":
            raise NotImplementedError("TIFF predictor 2 on floating-point samples")
        np.cumsum(a, axis=1, dtype=a.dtype, out=a)
    elif info.predictor != 1:
        raise NotImplementedError(f"TIFF predictor {info.predictor}")
    return a


def read_tiff(path, window: Optional[Tuple[int, int, int, int]] = None, info: Optional[TiffInfo] = None) -> np.ndarray:
    """-> (bands, h, w) array; ``window`` = (row_off, col_off, height, width) inside the image (what
    ``rasterio.windows.Window(col_off, row_off, width, height)`` selects in dataset.py:59-76); only the blocks the window touches
    are read and decoded."""
    info = info or tiff_info(path)
    r0, c0, h, w = (0, 0, info.height, info.width) if window is None else (int(v) for v in window)
    if r0 < 0 or c0 < 0 or h <= 0 or w <= 0 or r0 + h > info.height or c0 + w > info.width:
        raise ValueError(f"{path}: window {window} outside the {info.height} x {info.width} image")
    bh, bw = info.block
    nby, nbx = -(-info.height // bh), -(-info.width // bw)
    planes = info.bands if info.planar == 2 else 1
    spp = 1 if info.planar == 2 else info.bands
    out = np.empty((info.bands, h, w), dtype=info.dtype.newbyteorder("="))
    with open(path, "rb") as f:
        for pl in range(planes):
            for by in range(r0 // bh, (r0 + h - 1) // bh + 1):
                for bx in range(c0 // bw, (c0 + w - 1) // bw + 1):
                    k = pl * nby * nbx + by * nbx + bx
                    rows = bh if info.tiled else min(bh, info.height - by * bh)      # tiles are always full size, strips are not
                    if info.counts[k] == 0:
                        # GDAL sparse file (SPARSE_OK=TRUE): a block that was never written has offset = byte count = 0 and
                        # reads as the nodata value (GDAL_NODATA, tag 42113) or zeros
                        nod = info.tags.get(42113)
                        try:
                            fillv = float(nod[1][0].strip().strip("\0")) if nod else 0.0
                        except (ValueError, AttributeError, IndexError):
                            fillv = 0.0
                        blk = np.full((rows, bw, spp), fillv, dtype=out.dtype)
                    else:
                        f.seek(info.offsets[k])
                        blk = _decode_block(f.read(info.counts[k]), info, rows, bw, spp)
                    y0, x0 = by * bh, bx * bw
                    ys, ye = max(r0, y0), min(r0 + h, y0 + rows)
                    xs, xe = max(c0, x0), min(c0 + w, x0 + bw)
                    part = blk[ys - y0:ye - y0, xs - x0:xe - x0, :]
                    if info.planar == 2:
                        out[pl, ys - r0:ye - r0, xs - c0:xe - c0] = part[..., 0]
                    else:
                        out[:, ys - r0:ye - r0, xs - c0:xe - c0] = np.moveaxis(part, 2, 0)
    return out


def write_tiff(path, array, blocksize: int = 128, compress: Optional[str] = "deflate", extra_tags: Optional[Dict[int, tuple]] = None):
    """(bands, h, w) or (h, w) array -> tiled little-endian TIFF with BLOCKSIZE x BLOCKSIZE tiles (128: the reference's
    ``profile={"BLOCKSIZE": 128}``), deflate or no compression, chunky samples.  ``extra_tags`` = {tag: (type, values)} as in
    ``TiffInfo.tags`` -- pass ``info.geo_tags()`` of a source file to keep the GeoTIFF georeferencing."""
    a = np.asarray(array)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("write_tiff: expected a (bands, h, w) or (h, w) array")
    kind = {"u": 1, "i": 2, "f": 3}.get(a.dtype.kind)
    if kind is None or a.dtype.itemsize not in (1, 2, 4, 8):
        raise ValueError(f"write_tiff: unsupported dtype {a.dtype}")
    if blocksize % 16:
        raise ValueError("write_tiff: TIFF tile sizes must be multiples of 16")
    comp = {None: 1, "none": 1, "deflate": 8}.get(compress)
    if comp is None:
        raise ValueError(f"write_tiff: compress must be None or 'deflate' (got {compress!r})")
    nb, H, W = a.shape
    a = np.ascontiguousarray(np.moveaxis(a, 0, 2)).astype(a.dtype.newbyteorder("<"))
    nby, nbx = -(-H // blocksize), -(-W // blocksize)
    blocks = []
    for by in range(nby):
        for bx in range(nbx):
            t = np.zeros((blocksize, blocksize, nb), dtype=a.dtype)
            part = a[by * blocksize:(by + 1) * blocksize, bx * blocksize:(bx + 1) * blocksize]
            t[:part.shape[0], :part.shape[1]] = part
            raw = t.tobytes()
            blocks.append(zlib.compress(raw, 6) if comp == 8 else raw)
    entries = {256: (4, (W,)), 257: (4, (H,)), 258: (3, (8 * a.dtype.itemsize,) * nb), 259: (3, (comp,)), 262: (3, (1,)),
               277: (3, (nb,)), 284: (3, (1,)), 322: (4, (blocksize,)), 323: (4, (blocksize,)), 339: (3, (kind,) * nb)}
    if nb > 1:
        entries[338] = (3, (0,) * (nb - 1))          # extra samples: unspecified
    for tag, tv in (extra_tags or {}).items():
        if tag not in entries and tag not in (324, 325, 273, 279, 278):
            entries[int(tag)] = tv
    ntags = len(entries) + 2
    pos = 8 + 2 + 12 * ntags + 4                     # header + IFD, then out-of-line values, then the tiles
    blobs = []

    def pack(typ, vals):
        if typ == 2:
            return vals[0].encode("latin-1") + b"\0"
        code, _ = _TYPES[typ]
        return struct.pack("<" + code[0] * len(vals), *vals)
    ool = {}
    for tag, (typ, vals) in entries.items():
        data = pack(typ, vals)
        if len(data) > 4:
            ool[tag] = (pos, data); pos += len(data) + (len(data) & 1)
    inline = len(blocks) == 1                        # a single LONG fits the IFD entry itself
    off_pos = pos; pos += 0 if inline else 4 * len(blocks)
    cnt_pos = pos; pos += 0 if inline else 4 * len(blocks)
    offsets = []
    for b in blocks:
        offsets.append(pos); pos += len(b) + (len(b) & 1)
    entries[324] = (4, tuple(offsets)); entries[325] = (4, tuple(len(b) for b in blocks))
    ool[324] = (off_pos, pack(*entries[324])); ool[325] = (cnt_pos, pack(*entries[325]))
    if inline:
        ool.pop(324); ool.pop(325)
    with open(path, "wb") as f:
        f.write(struct.pack("<2sHI", b"II", 42, 8))
        f.write(struct.pack("<H", ntags))
        for tag in sorted(entries):
            typ, vals = entries[tag]
            data = pack(typ, vals)
            cnt = len(data) if typ == 2 else len(vals) // len(_TYPES[typ][0])
            if tag in ool:
                f.write(struct.pack("<HHII", tag, typ, cnt, ool[tag][0]))
            else:
                f.write(struct.pack("<HHI4s", tag, typ, cnt, data.ljust(4, b"\0")))
        f.write(struct.pack("<I", 0))
        for tag in sorted(ool, key=lambda k: ool[k][0]):
            p, data = ool[tag]
            assert f.tell() == p, (tag, f.tell(), p)
            f.write(data + (b"\0" if len(data) & 1 else b""))
        for b in blocks:
            f.write(b + (b"\0" if len(b) & 1 else b""))


_MAIN_ONLY_TAGS = (33550, 33922, 34264, 34735, 34736, 34737, 42112)       # georeferencing and GDAL metadata: IFD 0 of a COG only


def _pack_tag(typ, vals):
    if typ == 2:
        return vals[0].encode("latin-1") + b"\0"
    return struct.pack("<" + _TYPES[typ][0][0] * len(vals), *vals)


def write_tiff_levels(path, levels, dtype, bands: int = 1, blocksize: int = 128, compress: Optional[str] = "deflate", predictor: int = 1,
                      extra_tags: Optional[Dict[int, tuple]] = None) -> int:
    """Finished tiles -> a classic little-endian TIFF in Cloud-Optimized GeoTIFF order.  Pure host code: the tiles arrive encoded.

    ``levels`` = [((h, w), payloads), ...], the full resolution first, then every overview, each ceil(previous / 2); ``payloads``
    lists the tiles of a level row-major: ``bytes`` as they go into the file (a [blocksize][blocksize][bands] chunky little-endian
    tile after ``predictor`` and ``compress``), or None for a tile that is absent.  ``extra_tags`` are the tags of the main image.

    Layout: the header, IFD 0 at offset 8 and its out-of-line values, then one IFD per overview (NewSubfileType = 1; the same tile
    size, sample format, compression and predictor; GDAL_NODATA repeated; the georeferencing and the GDAL metadata stay on the main
    image) each followed by its values, and only then tile bytes: the smallest overview first, the full resolution last, row-major
    inside a level.  An absent tile has offset = byte count = 0 (GDAL's sparse form, which ``read_tiff`` reads as nodata).  No
    GDAL structural-metadata block is written: it would declare block leaders that are not there.  A file that would pass 4 GiB
    raises NotImplementedError (BigTIFF).  Returns the file size."""
    dt = np.dtype(dtype)
    kind = {"u": 1, "i": 2, "f": 3}.get(dt.kind)
    if kind is None or dt.itemsize not in (1, 2, 4, 8):
        raise ValueError(f"write_tiff_levels: unsupported dtype {dt}")
    if blocksize <= 0 or blocksize % 16:
        raise ValueError("write_tiff_levels: TIFF tile sizes must be multiples of 16")
    comp = {None: 1, "none": 1, "deflate": 8}.get(compress)
    if comp is None:
        raise ValueError(f"write_tiff_levels: compress must be None or 'deflate' (got {compress!r})")
    if predictor not in (1, 2, 3) or (predictor == 2 and kind == 3) or (predictor == 3 and kind != 3):
        raise ValueError(f"write_tiff_levels: predictor {predictor} on {dt} samples")
    levels = [((int(h), int(w)), list(tiles)) for (h, w), tiles in levels]
    if not levels:
        raise ValueError("write_tiff_levels: no image")
    nb = int(bands)
    for k, ((h, w), tiles) in enumerate(levels):
        if h < 1 or w < 1 or len(tiles) != (-(-h // blocksize)) * (-(-w // blocksize)):
            raise ValueError(f"write_tiff_levels: level {k} is {h} x {w} with {len(tiles)} tiles of {blocksize}")
        if k and (h, w) != (-(-levels[k - 1][0][0] // 2), -(-levels[k - 1][0][1] // 2)):
            raise ValueError(f"write_tiff_levels: level {k} is {h} x {w}, not half of {levels[k - 1][0]}")
    extra = {int(t): v for t, v in (extra_tags or {}).items()}
    ifds = []
    for k, ((h, w), tiles) in enumerate(levels):
        e = {256: (4, (w,)), 257: (4, (h,)), 258: (3, (8 * dt.itemsize,) * nb), 259: (3, (comp,)), 262: (3, (1,)), 277: (3, (nb,)),
             284: (3, (1,)), 322: (4, (blocksize,)), 323: (4, (blocksize,)), 339: (3, (kind,) * nb),
             324: (4, (0,) * len(tiles)), 325: (4, tuple(0 if t is None else len(t) for t in tiles))}
        if k:
            e[254] = (4, (1,))                          # NewSubfileType: a reduced-resolution image
        if predictor != 1:
            e[317] = (3, (predictor,))
        if nb > 1:
            e[338] = (3, (0,) * (nb - 1))
        for tag, tv in extra.items():
            if tag not in e and tag not in (254, 317, 273, 279, 278) and (k == 0 or tag == 42113):
                e[tag] = tv
        ifds.append(e)
    # pass 1: where every IFD and every out-of-line value goes
    pos = 8
    plan = []
    for e in ifds:
        start = pos
        pos += 2 + 12 * len(e) + 4
        ool = {}
        for tag in sorted(e):
            n = len(_pack_tag(*e[tag]))
            if n > 4:
                ool[tag] = pos
                pos += n + (n & 1)
        plan.append((start, ool))
    # pass 2: the tiles, the smallest overview first
    for k in range(len(levels) - 1, -1, -1):
        offs = []
        for t in levels[k][1]:
            offs.append(0 if t is None else pos)
            if t is not None:
                if len(t) == 0:
                    raise ValueError("write_tiff_levels: an empty tile payload (None marks an absent tile)")
                pos += len(t) + (len(t) & 1)
        ifds[k][324] = (4, tuple(offs))
    if pos > 0xFFFFFFFF:
        raise NotImplementedError(f"{path}: {pos} bytes do not fit a classic TIFF (BigTIFF is not supported)")
    with open(path, "wb") as f:
        f.write(struct.pack("<2sHI", b"II", 42, 8))
        for k, e in enumerate(ifds):
            start, ool = plan[k]
            assert f.tell() == start, (k, f.tell(), start)
            f.write(struct.pack("<H", len(e)))
            for tag in sorted(e):
                typ, vals = e[tag]
                data = _pack_tag(typ, vals)
                cnt = len(data) if typ == 2 else len(vals) // len(_TYPES[typ][0])
                if tag in ool:
                    f.write(struct.pack("<HHII", tag, typ, cnt, ool[tag]))
                else:
                    f.write(struct.pack("<HHI4s", tag, typ, cnt, data.ljust(4, b"\0")))
            f.write(struct.pack("<I", plan[k + 1][0] if k + 1 < len(ifds) else 0))
            for tag in sorted(ool):
                data = _pack_tag(*e[tag])
                assert f.tell() == ool[tag], (tag, f.tell(), ool[tag])
                f.write(data + (b"\0" if len(data) & 1 else b""))
        for k in range(len(levels) - 1, -1, -1):
            for t in levels[k][1]:
                if t is not None:
                    f.write(t)
                    if len(t) & 1:
                        f.write(b"\0")
        assert f.tell() == pos, (f.tell(), pos)
    return pos


def _raw_ifds(path):
    """every IFD of a little- or big-endian classic TIFF as it lies in the file -> (byte order, [{"offset", "end", "next",
    "entries": {tag: {"type", "count", "pos": file position of the 12-byte entry, "value_offset": position of an out-of-line value
    or None, "nbytes", "values"}}}])"""
    out = []
    with open(path, "rb") as f:
        bo, offs = _ifd_offsets(f, path)
        for off in offs:
            f.seek(off)
            n, = struct.unpack(bo + "H", f.read(2))
            raw = f.read(12 * n)
            nxt, = struct.unpack(bo + "I", f.read(4))
            entries = {}
            for i in range(n):
                tag, typ, cnt, val = struct.unpack(bo + "HHI4s", raw[12 * i:12 * i + 12])
                if typ not in _TYPES:
                    continue
                code, size = _TYPES[typ]
                nbytes = size * cnt
                voff = None
                if nbytes <= 4:
                    data = val[:nbytes]
                else:
                    voff, = struct.unpack(bo + "I", val)
                    f.seek(voff)
                    data = f.read(nbytes)
                vals = (data.rstrip(b"\0").decode("latin-1"),) if typ == 2 else struct.unpack(bo + code[0] * (cnt * len(code)), data)
                entries[tag] = {"type": typ, "count": cnt, "pos": off + 2 + 12 * i, "value_offset": voff, "nbytes": nbytes, "values": vals}
            out.append({"offset": off, "end": off + 2 + 12 * n + 4, "next": nxt, "entries": entries})
    return bo, out


def cog_layout_problems(path):
    """The layout rules of a Cloud-Optimized GeoTIFF as ``write_tiff_levels`` writes it -> a list of sentences, empty for a
    conforming file: classic little-endian TIFF, IFD 0 at offset 8, every IFD behind the one before it, every image tiled, every
    overview marked with NewSubfileType bit 0, ceil(previous / 2) in size and alike in tile size, samples, compression, predictor
    and GDAL_NODATA, georeferencing and GDAL metadata on the main image only, every IFD and every out-of-line value in front of the
    first tile byte, tile data ascending from the smallest overview to the full resolution and row-major inside a level, absent
    tiles with offset = byte count = 0."""
    problems = []
    try:
        bo, ifds = _raw_ifds(path)
    except (ValueError, NotImplementedError, struct.error) as e:
        return [f"not a readable classic TIFF: {e}"]
    if bo != "<":
        problems.append("the file is big-endian")
    if not ifds:
        return problems + ["the file has no IFD"]
    if ifds[0]["offset"] != 8:
        problems.append(f"IFD 0 is at offset {ifds[0]['offset']}, not 8")

    def val(e, tag, default=None):
        return e[tag]["values"] if tag in e else default
    first_tile = None
    runs = []
    for k, d in enumerate(ifds):
        e = d["entries"]
        if k and d["offset"] <= ifds[k - 1]["offset"]:
            problems.append(f"IFD {k} at offset {d['offset']} does not follow IFD {k - 1} at {ifds[k - 1]['offset']}")
        if 322 not in e or 323 not in e or 324 not in e or 325 not in e:
            problems.append(f"IFD {k} is not tiled")
            continue
        offs, cnts = e[324]["values"], e[325]["values"]
        h, w, bh, bw = val(e, 257)[0], val(e, 256)[0], val(e, 323)[0], val(e, 322)[0]
        if len(offs) != len(cnts) or len(offs) != (-(-h // bh)) * (-(-w // bw)) * (val(e, 277, (1,))[0] if val(e, 284, (1,))[0] == 2 else 1):
            problems.append(f"IFD {k}: {len(offs)} tile offsets and {len(cnts)} byte counts for a {h} x {w} image of {bh} x {bw} tiles")
        if any((o == 0) != (c == 0) for o, c in zip(offs, cnts)):
            problems.append(f"IFD {k}: an absent tile must have offset = byte count = 0")
        runs.append((k, [o for o in offs if o]))
        for o in offs:
            if o and (first_tile is None or o < first_tile):
                first_tile = o
        sub = val(e, 254, (0,))[0]
        if k == 0:
            if sub & 1:
                problems.append("IFD 0 is marked as a reduced-resolution image (NewSubfileType)")
            continue
        m = ifds[0]["entries"]
        p = ifds[k - 1]["entries"]
        if not sub & 1:
            problems.append(f"IFD {k}: NewSubfileType is missing or lacks the reduced-resolution bit")
        if 256 in p and 257 in p and (h, w) != (-(-val(p, 257)[0] // 2), -(-val(p, 256)[0] // 2)):
            problems.append(f"IFD {k} is {h} x {w}, not half of the {val(p, 257)[0]} x {val(p, 256)[0]} of IFD {k - 1}")
        for tag, name in ((322, "tile width"), (323, "tile length"), (258, "bits per sample"), (339, "sample format"), (277, "samples per pixel"),
                          (259, "compression"), (317, "predictor"), (284, "planar configuration"), (42113, "GDAL_NODATA")):
            if val(e, tag) != val(m, tag):
                problems.append(f"IFD {k}: {name} {val(e, tag)} differs from the main image's {val(m, tag)}")
        for tag in _MAIN_ONLY_TAGS:
            if tag in e:
                problems.append(f"IFD {k} carries tag {tag}, which belongs to the main image only")
    if first_tile is not None:
        for k, d in enumerate(ifds):
            if d["end"] > first_tile:
                problems.append(f"IFD {k} ends at {d['end']}, behind the first tile byte at {first_tile}")
            for tag, t in d["entries"].items():
                if t["value_offset"] is not None and t["value_offset"] + t["nbytes"] > first_tile:
                    problems.append(f"IFD {k}: the values of tag {tag} at {t['value_offset']} lie behind the first tile byte at {first_tile}")
    last = 0
    for k, offs in reversed(runs):
        for i, o in enumerate(offs):
            if o <= last:
                problems.append(f"IFD {k}: tile data at {o} is not behind {last}: tiles go row-major, the smallest overview first and "
                                f"the full resolution last")
                break
            last = o
    return problems


# ------------------------------------------------------------------------------------------------ PNG
def write_png(path, scanlines, width: int, height: int, text: Optional[str] = None):
    """8-bit truecolour PNG from finished scanlines: ``height`` rows of ``1 + 3 * width`` bytes, each a filter byte 0 followed by
    RGB triplets (what ``sc_render_panels`` leaves in its canvas), so the buffer goes to zlib without a repack.  ``text`` is
    stored in one tEXt chunk with the keyword ``Comment``; ``plot.Panels.save`` puts the panel names and ranges there as JSON."""
    data = memoryview(np.ascontiguousarray(np.asarray(scanlines, dtype=np.uint8))).cast("B")
    width, height = int(width), int(height)
    if width < 1 or height < 1 or len(data) != height * (1 + 3 * width):
        raise ValueError(f"write_png: {len(data)} bytes are not {height} scanlines of 1 + 3 * {width} bytes")
    if any(data[0::1 + 3 * width]):
        raise ValueError("write_png: every scanline must start with the filter byte 0")

    def chunk(kind: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))]
    if text is not None:
        out.append(chunk(b"tEXt", b"Comment\0" + text.encode("latin-1")))
    out += [chunk(b"IDAT", zlib.compress(data)), chunk(b"IEND", b"")]
    with open(path, "wb") as f:
        f.write(b"".join(out))


# ------------------------------------------------------------------------------------------------ ENVI
_ENVI_DTYPES = {1: "u1", 2: "i2", 3: "i4", 4: "f4", 5: "f8", 12: "u2", 13: "u4", 14: "i8", 15: "u8"}


def read_envi_header(path_hdr) -> Dict[str, object]:
    """ENVI .hdr -> dict (lower-case keys; brace lists become lists of strings)"""
    txt = open(path_hdr, "r", errors="replace").read()
    if not txt.lstrip().upper().startswith("ENVI"):
        raise ValueError(f"{path_hdr}: not an ENVI header")
    out = {}
    for m in re.finditer(r"^\s*([^=\n]+?)\s*=\s*(\{[^}]*\}|[^\n]*)", txt, re.M):
        k, v = m.group(1).strip().lower(), m.group(2).strip()
        if v.startswith("{"):
            v = [s.strip() for s in v[1:-1].replace("\n", " ").split(",") if s.strip()]
        out[k] = v
    return out


def open_envi(path, writable: bool = False):
    """``path`` = the data file or its ``.hdr``.  -> (cube, meta): ``cube`` is a numpy memmap VIEW of shape (lines, samples,
    bands) whatever the file's interleave (the reference's ``open_memmap(interleave='bip')``, process_aviris.py:183-187; for BIP
    files the view is contiguous), ``meta`` = {"wavelengths", "fwhm" (float64 arrays or None), "header"}."""
    hdr = path if path.endswith(".hdr") else (path + ".hdr" if os.path.exists(path + ".hdr") else os.path.splitext(path)[0] + ".hdr")
    h = read_envi_header(hdr)
    dat = path if not path.endswith(".hdr") else next((c for c in (path[:-4], path[:-4] + ".img", path[:-4] + ".dat", path[:-4] + ".lut")
                                                       if os.path.exists(c)), None)
    if dat is None:
        raise FileNotFoundError(f"no data file next to {hdr}")
    ns, nl, nb = int(h["samples"]), int(h["lines"]), int(h["bands"])
    dt = _ENVI_DTYPES.get(int(h["data type"]))
    if dt is None:
        raise NotImplementedError(f"{hdr}: ENVI data type {h['data type']}")
    dt = np.dtype((">" if int(h.get("byte order", 0)) else "<") + dt)
    il = str(h.get("interleave", "bsq")).lower()
    shape = {"bip": (nl, ns, nb), "bil": (nl, nb, ns), "bsq": (nb, nl, ns)}[il]
    mm = np.memmap(dat, dtype=dt, mode="r+" if writable else "r", offset=int(h.get("header offset", 0)), shape=shape)
    cube = {"bip": mm, "bil": mm.transpose(0, 2, 1), "bsq": mm.transpose(1, 2, 0)}[il]

    def floats(key):
        return np.array([float(v) for v in h[key]], dtype=np.float64) if key in h else None
    return cube, {"wavelengths": floats("wavelength"), "fwhm": floats("fwhm"), "header": h}


def envi_geo_tags(header: Dict[str, object]) -> Dict[int, tuple]:
    """GeoTIFF georeferencing tags from an ENVI header's ``map info`` (what rasterio's ``src.transform`` / ``src.crs`` carry from
    the radiance file into the mag1c product, process_aviris.py:179-181,222-226).  ``map info = {UTM, x_ref, y_ref, easting,
    northing, x_size, y_size, zone, North|South, datum, units=..., rotation=deg}`` becomes the affine transform GDAL's ENVI
    driver builds (rotation in degrees, counter-clockwise, applied to the pixel axes) stored as ModelTransformationTag (34264) --
    or ModelPixelScale (33550) + ModelTiepoint (33922) when there is no rotation -- and a GeoKeyDirectory (34735) with
    ProjectedCSTypeGeoKey = EPSG 326zz / 327zz for WGS-84 UTM or GeographicTypeGeoKey 4326 for ``Geographic Lat/Lon``.
    Returns {} when the header has no usable map info."""
    mi = header.get("map info")
    if not isinstance(mi, list) or len(mi) < 7:
        return {}
    proj = mi[0].strip().lower()
    try:
        xr, yr, e0, n0, px, py = (float(v) for v in mi[1:7])
    except ValueError:
        return {}
    rot = 0.0
    for v in mi[7:]:
        if v.lower().replace(" ", "").startswith("rotation="):
            rot = float(v.split("=")[1])
    import math
    r = -math.radians(rot)
    gt = (e0 - (xr - 1.0) * px, math.cos(r) * px, -math.sin(r) * px, n0 + (yr - 1.0) * py, -math.sin(r) * py, -math.cos(r) * py)
    tags: Dict[int, tuple] = {}
    if rot == 0.0:
        tags[33550] = (12, (px, py, 0.0))
        tags[33922] = (12, (0.0, 0.0, 0.0, gt[0], gt[3], 0.0))
    else:
        tags[34264] = (12, (gt[1], gt[2], 0.0, gt[0], gt[4], gt[5], 0.0, gt[3], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0))
    if proj == "utm" and len(mi) >= 9:
        zone = int(float(mi[7]))
        epsg = (32700 if mi[8].strip().lower().startswith("s") else 32600) + zone
        # header (version 1, revision 1.0, 3 keys), GTModelType = projected, GTRasterType = PixelIsArea, ProjectedCSType
        tags[34735] = (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, epsg))
    elif proj.startswith("geographic"):
        tags[34735] = (3, (1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326))
    return tags


def envi_geotransform(header: Dict[str, object]):
    """The full 6-term GDAL geotransform of an ENVI ``map info``, ``rotation=`` included, with the sign convention of
    :func:`envi_geo_tags` (degrees, counter-clockwise, applied to the pixel axes: the numbers its ModelTransformationTag holds), the
    EPSG code of the header (326zz / 327zz for UTM, 4326 for ``Geographic Lat/Lon``, else None) and the rotation in degrees ->
    ``(gt, epsg, rotation)``; ``(None, None, 0.0)`` when the header has no usable map info."""
    tags = envi_geo_tags(header)
    if not tags:
        return None, None, 0.0
    gt, epsg = geo_from_tags(tags)
    rot = 0.0
    for v in header["map info"][7:]:
        if v.lower().replace(" ", "").startswith("rotation="):
            rot = float(v.split("=")[1])
    return gt, epsg, rot


def geo_from_tags(info):
    """``(geotransform, epsg)`` of a GeoTIFF from its tags (a ``TiffInfo`` or a {tag: (type, values)} dict): the 6-term GDAL
    geotransform from ModelPixelScale (33550) + ModelTiepoint (33922) -- the tiepoint may sit at any pixel -- or from the
    ModelTransformation (34264), and the EPSG code from the GeoKeyDirectory (34735) as :func:`envi_geo_tags`,
    ``ortho.emit_geo_tags`` and ``warp.geo_tags`` write it: ProjectedCSTypeGeoKey (3072), else GeographicTypeGeoKey (2048).
    Either is None when the tags do not carry it."""
    tags = info.tags if isinstance(info, TiffInfo) else dict(info)
    gt = None
    if 33550 in tags and 33922 in tags:
        sx, sy = (float(v) for v in tags[33550][1][:2])
        i, j, _, x, y, _ = (float(v) for v in tags[33922][1][:6])
        gt = (x - i * sx, sx, 0.0, y + j * sy, 0.0, -sy)
    elif 34264 in tags:
        m = [float(v) for v in tags[34264][1]]
        gt = (m[3], m[0], m[1], m[7], m[4], m[5])
    epsg = None
    if 34735 in tags:
        keys = [int(v) for v in tags[34735][1]]
        found = {keys[k]: keys[k + 3] for k in range(4, min(len(keys), 4 + 4 * keys[3]) - 3, 4) if keys[k + 1] == 0}
        epsg = found.get(3072, found.get(2048))
    return gt, epsg


def window_geo_tags(info, row_off: int, col_off: int) -> Dict[int, tuple]:
    """Georeferencing tags of a window of a raster: the source's, moved to the window's upper-left corner (what the transform
    of ``RasterioReader.read_from_window(window, boundless=True)`` is, sampling_dataset.py:266).  ``info``: a ``TiffInfo`` or a
    {tag: (type, values)} dict.  A ModelTiepoint (33922) with its ModelPixelScale (33550) is re-anchored at pixel (0, 0) of the
    window; a ModelTransformation (34264) gets its translation column shifted by the rotated offset.  Offsets may be negative
    (a window that starts outside the raster).  The geo keys (34735-34737) are carried over; nodata and metadata tags are not.
    A source without georeferencing gives {}."""
    tags = info.tags if isinstance(info, TiffInfo) else dict(info)
    row_off, col_off = int(row_off), int(col_off)
    out: Dict[int, tuple] = {}
    if 33922 in tags and 33550 in tags:
        sx, sy = (float(v) for v in tags[33550][1][:2])
        i, j, k, x, y, z = (float(v) for v in tags[33922][1][:6])
        out[33550] = tags[33550]
        out[33922] = (12, (0.0, 0.0, 0.0, x + (col_off - i) * sx, y - (row_off - j) * sy, z))
    elif 34264 in tags:
        m = [float(v) for v in tags[34264][1]]
        m[3] = m[3] + m[0] * col_off + m[1] * row_off
        m[7] = m[7] + m[4] * col_off + m[5] * row_off
        out[34264] = (12, tuple(m))
    else:
        return {}
    for t in (34735, 34736, 34737):
        if t in tags:
            out[t] = tags[t]
    return out


def scaled_geo_tags(tags, sy: float, sx: float) -> Dict[int, tuple]:
    """Georeferencing tags of a raster resampled onto pixels ``sy`` x ``sx`` times as large (``sy = H / oh``, ``sx = W / ow``, the
    TRUE ratios, so the full extent maps onto the full extent and the upper-left corner stays where it is).  ``tags``: a ``TiffInfo``
    or a {tag: (type, values)} dict.  A ModelPixelScale (33550) is multiplied; a ModelTransformation (34264) gets its column vector
    (per output column) multiplied by ``sx`` and its row vector by ``sy``.  The tiepoint / translation and the geo keys are left
    alone (a tiepoint that is not at pixel (0, 0) has its pixel coordinates divided instead); every other tag is carried over."""
    tags = tags.tags if isinstance(tags, TiffInfo) else tags
    out = dict(tags)
    sy, sx = float(sy), float(sx)
    if 33550 in out:
        t, v = out[33550]
        out[33550] = (t, (float(v[0]) * sx, float(v[1]) * sy) + tuple(v[2:]))
        if 33922 in out and (float(out[33922][1][0]) != 0.0 or float(out[33922][1][1]) != 0.0):
            t, v = out[33922]                                 # a tiepoint off the corner keeps its place on the ground
            out[33922] = (t, (float(v[0]) / sx, float(v[1]) / sy) + tuple(v[2:]))
    if 34264 in out:
        t, v = out[34264]
        m = [float(e) for e in v]
        m[0], m[4], m[8] = m[0] * sx, m[4] * sx, m[8] * sx
        m[1], m[5], m[9] = m[1] * sy, m[5] * sy, m[9] * sy
        out[34264] = (t, tuple(m))
    return out


def gdal_metadata_tag(tags: Dict[str, object], descriptions: Sequence[str] = ()) -> Dict[int, tuple]:
    """GDAL_METADATA (42112): the XML in which GDAL / rasterio keep dataset tags and band descriptions -- what
    ``save_cog(..., descriptions=[...], tags={...})`` leaves in the reference's products (process_aviris.py:222-232)."""
    def esc(v):
        return str(v).replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;")
    items = []
    for k, v in tags.items():
        if isinstance(v, (list, tuple, np.ndarray)):
            v = "[" + " ".join(repr(float(x)) for x in np.asarray(v).ravel()) + "]"
        items.append(f'  <Item name="{esc(k)}">{esc(v)}</Item>')
    for i, d in enumerate(descriptions):
        items.append(f'  <Item name="DESCRIPTION" sample="{i}" role="description">{esc(d)}</Item>')
    return {42112: (2, ("<GDALMetadata>\n" + "\n".join(items) + "\n</GDALMetadata>",))}


# ------------------------------------------------------------------------------------------------ sample folders
def load_sample(folder: str, products: Sequence[str], window=None) -> np.ndarray:
    """(len(products), h, w) float32: ``torch.cat([rasterio.open(f"{folder}/{p}.tif").read(window=window) ...]).float()``
    of starcop/data/dataset.py:66-76"""
    return np.concatenate([read_tiff(os.path.join(folder, f"{p}.tif"), window).astype(np.float32) for p in products], axis=0)


def load_tileset(folders: Sequence[str], input_products: Sequence[str], output_products: Sequence[str] = ("labelbinary",),
                 weight_loss: Optional[str] = "weight_mag1c", ids: Optional[Sequence[str]] = None, device="cuda", workers: int = 8,
                 extra_products: Sequence[str] = ()):
    """Reads the sample folders of a split (the ``folder`` column of the reference's train.csv / test.csv, datamodule.py:98-106)
    into PINNED host buffers with a pool of decoder threads (zlib releases the GIL) and uploads each tensor with one
    asynchronous copy -> ``datamodule.ResidentTileSet`` (tiles resident in HBM for the whole training run).  ``extra_products``
    (e.g. what only the plot loaders show) are kept one (M,1,H,W) plane each in ``ResidentTileSet.extras``."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from .datamodule import ResidentTileSet
    folders = list(folders)
    first = load_sample(folders[0], input_products)
    H, W = first.shape[-2:]
    M = len(folders)
    pin = torch.cuda.is_available()
    groups = [("inputs", list(input_products)), ("outputs", list(output_products))] + ([("weight_loss", [weight_loss])] if weight_loss else [])
    groups += [("extra:" + p, [p]) for p in extra_products]
    host = {name: torch.empty((M, len(p), H, W), dtype=torch.float32, pin_memory=pin) for name, p in groups}

    def work(i):
        for name, prods in groups:
            host[name][i] = torch.from_numpy(load_sample(folders[i], prods))
    with ThreadPoolExecutor(max_workers=max(1, workers)) as ex:
        list(ex.map(work, range(M)))
    dev = {name: t.to(device, non_blocking=True) for name, t in host.items()}
    if pin:
        torch.cuda.current_stream().synchronize()        # the pinned staging buffers may be released after this
    return ResidentTileSet(dev["inputs"], dev["outputs"], dev.get("weight_loss"), ids=ids or [os.path.basename(f.rstrip("/")) for f in folders],
                           device=device, extras={p: dev["extra:" + p] for p in extra_products})
