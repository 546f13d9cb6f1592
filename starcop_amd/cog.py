"""Cloud-Optimized GeoTIFFs straight from device tensors: what ``georeader.save_cog`` does for every product the reference writes.

A product stays on the device until it is TIFF bytes.  The overview pyramid (``sc_overview_reduce``: up to three levels per launch
from one read of its source), the search for tiles that hold nothing but fill (``sc_tiff_tile_flags``) and the cut into padded,
pixel-interleaved tiles with their predictor (``sc_tiff_pack_tiles``) are HIP kernels; only the tiles that will be stored cross to
the host, one copy per level through a pinned buffer.  The host deflates them on a thread pool (zlib releases the GIL) and
``io_formats.write_tiff_levels`` lays the file out: IFDs first, the smallest overview's tiles next, the full resolution last, absent
tiles as offset = byte count = 0.  There is no CPU fallback: without a gfx950 device every call here raises.
"""
import ctypes as C
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from . import io_formats

RESAMPLING = {"average": _lib.COG_AVERAGE, "nearest": _lib.COG_NEAREST, "mode": _lib.COG_MODE}
_DTYPES = {torch.float32: np.dtype(np.float32), torch.uint8: np.dtype(np.uint8)}


def overview_levels(h, w, min_size=512):
    """[(h1, w1), ...]: halve (rounding up) until the longer side is at most ``min_size``"""
    h, w, min_size = int(h), int(w), int(min_size)
    if h < 1 or w < 1 or min_size < 1:
        raise ValueError(f"overview_levels: bad size {h} x {w} or min_size {min_size}")
    out = []
    while max(h, w) > min_size:
        h, w = -(-h // 2), -(-w // 2)
        out.append((h, w))
    return out


def _nodata_bits(nodata, dtype, who):
    """bit pattern of ``nodata`` in ``dtype`` (numpy); None -> None"""
    if nodata is None:
        return None
    if dtype == np.uint8:
        v = float(nodata)
        if v != int(v) or not 0 <= v <= 255:
            raise ValueError(f"{who}: nodata {nodata!r} is not a uint8 value")
        return int(v)
    return int(np.float32(nodata).view(np.uint32))


def _check(who, dtype, shape, blocksize=None, resampling=None, predictor=None):
    """the refusals that need no device -> (numpy dtype, resampling code or None, TIFF predictor or None)"""
    np_dt = _DTYPES.get(dtype) if isinstance(dtype, torch.dtype) else (np.dtype(dtype) if np.dtype(dtype) in _DTYPES.values() else None)
    if np_dt is None:
        raise ValueError(f"{who}: float32 or uint8 expected, got {dtype}")
    if len(shape) not in (2, 3):
        raise ValueError(f"{who}: expected an (H, W) or (bands, H, W) image, got shape {tuple(shape)}")
    if len(shape) == 3 and not 1 <= shape[0] <= _lib.COG_MAX_BANDS:
        raise ValueError(f"{who}: {shape[0]} bands (1 to {_lib.COG_MAX_BANDS})")
    if min(shape) < 1:
        raise ValueError(f"{who}: empty image {tuple(shape)}")
    if blocksize is not None and (int(blocksize) < 16 or int(blocksize) % 16):
        raise ValueError(f"{who}: TIFF tile sizes must be multiples of 16 (got {blocksize})")
    mode = None
    if resampling is not None:
        if resampling not in RESAMPLING:
            raise ValueError(f"{who}: resampling must be one of {sorted(RESAMPLING)} (got {resampling!r})")
        if resampling == "mode" and np_dt != np.uint8:
            raise ValueError(f"{who}: mode resampling is for uint8 images, not {np_dt}")
        mode = RESAMPLING[resampling]
    pred = None
    if predictor is not None:
        pred = {"auto": 3 if np_dt == np.float32 else 2}.get(predictor, predictor)
        if pred not in (1, 2, 3) or (pred == 2 and np_dt != np.uint8) or (pred == 3 and np_dt != np.float32):
            raise ValueError(f"{who}: predictor {predictor!r} on {np_dt} (1; 2 on uint8; 3 on float32; 'auto')")
    return np_dt, mode, pred


def _device_image(image, who):
    """numpy array or tensor -> (nb, H, W) device tensor, read in place (a numpy array is uploaded once)"""
    if isinstance(image, torch.Tensor):
        _lib.require_device(image)
        t = image
    else:
        _lib.require_device()
        a = np.asarray(image)
        if any(s < 0 for s in a.strides):
            a = np.ascontiguousarray(a)
        t = torch.from_numpy(a).to("cuda", non_blocking=False)
    return t[None] if t.dim() == 2 else t


def _image_struct(t, nd_bits):
    s = _lib.sc_cog_image()
    s.data = t.data_ptr()
    s.elem_bytes = t.element_size()
    s.nb, s.h, s.w = (int(v) for v in t.shape)
    s.band_stride, s.row_stride, s.col_stride = (int(v) for v in t.stride())
    s.has_nodata = int(nd_bits is not None)
    s.nodata_bits = nd_bits or 0
    return s


def build_overviews(image, levels, resampling, nodata=None):
    """``sc_overview_reduce``: the pyramid of an (H, W) or (nb, H, W) float32 / uint8 image -> one dense (nb, h_k, w_k) device tensor
    per level.  ``levels``: how many, or the shapes ``overview_levels`` gave (each must be ceil(previous / 2)).  Three levels come
    out of one launch; deeper pyramids chain launches from the last level written."""
    shape = tuple(image.shape)
    np_dt, mode, _ = _check("build_overviews", image.dtype, shape, resampling=resampling)
    nd = _nodata_bits(nodata, np_dt, "build_overviews")
    h, w = shape[-2:]
    if isinstance(levels, int):
        n = levels
    else:
        want = []
        for _ in levels:
            h, w = -(-h // 2), -(-w // 2)
            want.append((h, w))
        if [tuple(int(v) for v in s) for s in levels] != want:
            raise ValueError(f"build_overviews: levels {list(levels)} are not the halvings {want} of {shape[-2:]}")
        n = len(want)
    if n < 0:
        raise ValueError("build_overviews: negative level count")
    src = _device_image(image, "build_overviews")
    lib = _lib.load()
    out = []
    while len(out) < n:
        k = min(3, n - len(out))
        a = _lib.sc_overview_args()
        a.src = _image_struct(src, nd)
        a.resampling, a.levels = mode, k
        hh, ww = int(src.shape[1]), int(src.shape[2])
        made = []
        for i in range(k):
            hh, ww = -(-hh // 2), -(-ww // 2)
            made.append(torch.empty((src.shape[0], hh, ww), dtype=src.dtype, device=src.device))
            a.dst[i] = made[-1].data_ptr()
        _lib.check(lib.sc_overview_reduce(C.byref(a), _lib.stream()))
        out += made
        src = made[-1]
    return out


def tile_flags(image, blocksize, nodata=None):
    """``sc_tiff_tile_flags``: uint8 device tensor, one entry per ``blocksize`` tile (row-major): 1 where every in-image sample has
    the bits of the fill value (``nodata``, else 0)"""
    np_dt, _, _ = _check("tile_flags", image.dtype, tuple(image.shape), blocksize=blocksize)
    nd = _nodata_bits(nodata, np_dt, "tile_flags")
    src = _device_image(image, "tile_flags")
    bs = int(blocksize)
    tiles = (-(-int(src.shape[1]) // bs)) * (-(-int(src.shape[2]) // bs))
    flags = torch.empty(tiles, dtype=torch.uint8, device=src.device)
    s = _image_struct(src, nd)
    _lib.check(_lib.load().sc_tiff_tile_flags(C.byref(s), bs, _lib.ptr(flags), _lib.stream()))
    return flags


def pack_tiles(image, blocksize, predictor, slots, slots_host, n_slots, out=None):
    """``sc_tiff_pack_tiles``: the tiles with a slot >= 0 as TIFF tile bytes -> uint8 device tensor (n_slots, tile bytes).
    ``slots`` (int32 device) and ``slots_host`` (the same as an int32 numpy array) name the slot of every tile, -1 for none."""
    np_dt, _, pred = _check("pack_tiles", image.dtype, tuple(image.shape), blocksize=blocksize, predictor=predictor)
    src = _device_image(image, "pack_tiles")
    bs = int(blocksize)
    tile_bytes = bs * bs * int(src.shape[0]) * src.element_size()
    if out is None:
        out = torch.empty((int(n_slots), tile_bytes), dtype=torch.uint8, device=src.device)
    slots_host = np.ascontiguousarray(slots_host, dtype=np.int32)
    a = _lib.sc_tiff_pack_args()
    a.src = _image_struct(src, None)
    a.bs, a.predictor, a.n_slots = bs, pred, int(n_slots)
    a.slots, a.slots_host = slots.data_ptr(), slots_host.ctypes.data
    a.out, a.out_bytes = out.data_ptr(), out.numel()
    if slots.dtype != torch.int32 or not slots.is_contiguous() or slots.numel() != slots_host.size:
        raise ValueError("pack_tiles: slots must be a contiguous int32 device tensor as long as slots_host")
    _lib.check(_lib.load().sc_tiff_pack_tiles(C.byref(a), _lib.stream()))
    return out


def pack_level(image, blocksize=128, predictor=None, nodata=None, sparse=True):
    """One level of a file, ready for the host: flags the tiles that hold nothing but fill, gives the others consecutive slots
    (all of them with ``sparse=False``), packs those on the device and copies them to the host in ONE transfer through a pinned
    buffer.  -> (tiles: uint8 numpy array (stored tiles, tile bytes) over the pinned buffer, slots: int32 numpy array per tile, -1
    for an absent one, flags: uint8 numpy array per tile).  Synchronises the stream."""
    np_dt, _, pred = _check("pack_level", image.dtype, tuple(image.shape), blocksize=blocksize, predictor=predictor or 1)
    src = _device_image(image, "pack_level")
    flags = tile_flags(src, blocksize, nodata)
    keep = (flags == 0) if sparse else torch.ones_like(flags, dtype=torch.bool)
    slots = torch.where(keep, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
    both = torch.stack([slots, flags.to(torch.int32)]).cpu().numpy()           # the one synchronising read of the tables
    slots_host, flags_host = np.ascontiguousarray(both[0]), both[1].astype(np.uint8)
    n = int((slots_host >= 0).sum())
    bs = int(blocksize)
    tile_bytes = bs * bs * int(src.shape[0]) * src.element_size()
    host = torch.empty((n, tile_bytes), dtype=torch.uint8, pin_memory=True)
    if n:
        dev = pack_tiles(src, bs, pred, slots, slots_host, n)
        host.copy_(dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return host.numpy(), slots_host, flags_host


def default_workers():
    """threads of the deflate pool: the CPUs this process may run on, 16 at most (never the machine's CPU count)"""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _tag_nodata(extra_tags):
    t = (extra_tags or {}).get(42113)
    if not t:
        return None
    try:
        return float(str(t[1][0]).strip().strip("\0"))
    except (ValueError, IndexError, TypeError):
        raise ValueError(f"write_cog: GDAL_NODATA tag {t!r} is not a number")


def write_cog(path, image, blocksize=128, compress="deflate", predictor=None, nodata=None, overviews="auto", overview_min_size=512,
              resampling=None, sparse=True, extra_tags=None, workers=None):
    """(H, W) or (nb, H, W) float32 / uint8 image -> Cloud-Optimized GeoTIFF.  A device tensor is read in place (any non-negative
    strides), a numpy array is uploaded once.

    ``overviews``: "auto" = ``overview_levels(H, W, overview_min_size)``, a level count, or () for none.  ``resampling``: "average",
    "nearest" or "mode" (uint8 only); None = average for float32, mode for uint8.  ``predictor``: None / 1 = none (tile bytes as
    ``write_tiff`` builds them), 2 (uint8), 3 (float32) or "auto" = 3 for float32, 2 for uint8.  ``nodata`` is the fill value of
    the overviews and of absent tiles and is written as GDAL_NODATA (tag 42113) unless ``extra_tags`` carries the tag, which must
    then agree; a tag without ``nodata`` is taken as the nodata.  ``sparse``: tiles that hold nothing but fill (nodata, else 0) are
    not stored.  ``compress``: "deflate" (zlib level 6 per tile, ``workers`` threads; None = the CPUs of this process, 16 at most)
    or None.  -> {"levels", "tiles", "tiles_stored", "bytes_to_host", "bytes_written"}."""
    shape = tuple(image.shape)
    np_dt, _, pred = _check("write_cog", image.dtype, shape, blocksize=blocksize, predictor=1 if predictor is None else predictor)
    if resampling is None:
        resampling = "average" if np_dt == np.float32 else "mode"
    _check("write_cog", image.dtype, shape, resampling=resampling)
    if compress not in (None, "none", "deflate"):
        raise ValueError(f"write_cog: compress must be None or 'deflate' (got {compress!r})")
    tagged = _tag_nodata(extra_tags)
    if nodata is None:
        nodata = tagged
    elif tagged is not None and _nodata_bits(tagged, np_dt, "write_cog") != _nodata_bits(nodata, np_dt, "write_cog") and \
            not (np.isnan(tagged) and np.isnan(float(nodata))):
        raise ValueError(f"write_cog: nodata {nodata!r} and the GDAL_NODATA tag {tagged!r} of extra_tags differ")
    _nodata_bits(nodata, np_dt, "write_cog")
    H, W = shape[-2:]
    if isinstance(overviews, str):
        if overviews != "auto":
            raise ValueError(f"write_cog: overviews must be 'auto', a count or () (got {overviews!r})")
        n_over = len(overview_levels(H, W, overview_min_size))
    elif isinstance(overviews, int):
        n_over = overviews
    else:
        n_over = len(tuple(overviews))
    if workers is None:
        workers = default_workers()
    if int(workers) < 1:
        raise ValueError(f"write_cog: workers={workers}")
    tags = dict(extra_tags or {})
    if nodata is not None and 42113 not in tags:
        tags[42113] = (2, (f"{float(nodata):.9g}" if np_dt == np.float32 else str(int(nodata)),))
    src = _device_image(image, "write_cog")
    images = [src] + build_overviews(src, n_over, resampling, nodata)
    packed = [pack_level(im, blocksize, pred, nodata, sparse) for im in images]
    deflate = compress == "deflate"
    jobs = [tiles[i] for tiles, _, _ in packed for i in range(tiles.shape[0])]
    if deflate:
        if int(workers) == 1 or len(jobs) < 2:
            done = [zlib.compress(t, 6) for t in jobs]
        else:
            with ThreadPoolExecutor(max_workers=int(workers)) as pool:
                done = list(pool.map(lambda t: zlib.compress(t, 6), jobs, chunksize=1))
    else:
        done = [t.tobytes() for t in jobs]
    levels, first = [], 0
    for im, (tiles, slots, _) in zip(images, packed):
        levels.append(((int(im.shape[1]), int(im.shape[2])), [None if s < 0 else done[first + s] for s in slots.tolist()]))
        first += tiles.shape[0]
    size = io_formats.write_tiff_levels(path, levels, np_dt, bands=int(src.shape[0]), blocksize=int(blocksize),
                                        compress="deflate" if deflate else None, predictor=pred, extra_tags=tags)
    return {"levels": len(images), "tiles": sum(int(s.size) for _, s, _ in packed), "tiles_stored": len(jobs),
            "bytes_to_host": sum(int(t.nbytes) for t, _, _ in packed), "bytes_written": size}
