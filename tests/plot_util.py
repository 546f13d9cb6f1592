"""numpy restatement of the per-pixel contract of the validation panels (DESIGN.md "Validation panels", include/starcop_hip.h) and
a small PNG decoder, shared by tests/test_plot_host.py and tests/test_gpu_plot.py.  Nothing here imports matplotlib or PIL."""
import json
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g15_panels.npz")
WHITE = np.array([255, 255, 255], np.uint8)
F32 = np.float32


def viridis8():
    return np.loadtxt(os.path.join(ROOT, "starcop_amd", "data", "viridis8.txt"), dtype=np.uint8).reshape(256, 3)


def _values(x, div=1.0):
    v = np.asarray(x).astype(F32)
    if F32(div) != F32(1):
        v = v / F32(div)
    return v


def finite_minmax(x, div=1.0):
    """(min, max) over the finite values as float32, (0, 1) if there is none: sc_panel_minmax"""
    v = _values(x, div)
    v = v[np.isfinite(v)]
    return (F32(0), F32(1)) if v.size == 0 else (v.min(), v.max())


def band_bytes(x, vmin, vmax, div=1.0, lut=None):
    """BAND: (H, W, 3) uint8"""
    lut = viridis8() if lut is None else lut
    v = _values(x, div)
    vmin, vmax = F32(vmin), F32(vmax)
    fin = np.isfinite(v)
    d = F32(np.float64(vmax) - np.float64(vmin))
    with np.errstate(all="ignore"):
        t = (np.where(fin, v, F32(0)) - vmin) / d if vmax != vmin else np.zeros_like(v)
        xa = (t * F32(256)).astype(F32)
        idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, np.trunc(np.clip(xa, -1, 256)))).astype(np.int64)
    out = lut[idx]
    out[~fin] = WHITE
    return out


def rgb_bytes(r, g, b):
    """RGB: (H, W, 3) uint8"""
    v = np.stack([np.asarray(c).astype(F32) for c in (r, g, b)], axis=-1)
    bad = np.isnan(v).any(axis=-1)
    c = np.where(v < 0, F32(0), np.where(v > 1, F32(1), v)).astype(F32)
    with np.errstate(all="ignore"):
        out = np.trunc(np.where(np.isnan(c), F32(0), c) * F32(255)).astype(np.uint8)
    out[bad] = WHITE
    return out


def cat_bytes(x, categories):
    """CATEGORICAL: categories = [(value, (r, g, b)), ...]; the last match wins, no match is black"""
    v = np.asarray(x).astype(F32)
    out = np.zeros(v.shape + (3,), np.uint8)
    for value, colour in categories:
        out[v == F32(value)] = np.asarray(colour, np.uint8)
    return out


def compose(panels, Hc, Wc):
    """PNG scanlines (Hc, 1 + 3 Wc) uint8 of panels = [(image (H, W, 3), scale, y, x), ...]: white background, filter byte 0"""
    img = np.full((Hc, Wc, 3), 255, np.uint8)
    for im, scale, y, x in panels:
        big = np.repeat(np.repeat(im, scale, axis=0), scale, axis=1)
        img[y:y + big.shape[0], x:x + big.shape[1]] = big
    return np.concatenate([np.zeros((Hc, 1), np.uint8), img.reshape(Hc, 3 * Wc)], axis=1)


def decode_png(path):
    """(width, height, image (H, W, 3) uint8, tEXt dict) of an 8-bit truecolour, non-interlaced PNG whose rows all use filter 0;
    checks the signature, every chunk's CRC, the IHDR fields and the filter bytes"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n", "PNG signature"
    pos, idat, text, ihdr, kinds = 8, [], {}, None, []
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, f"CRC of {kind}"
        kinds.append(kind)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"tEXt":
            key, _, val = body.partition(b"\0")
            text[key.decode("latin-1")] = val.decode("latin-1")
        pos += 12 + n
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and pos == len(raw)
    width, height, depth, colour, comp, filt, interlace = ihdr
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0), ihdr
    rows = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(height, 1 + 3 * width)
    assert not rows[:, 0].any(), "filter byte 0 on every row"
    return width, height, rows[:, 1:].reshape(height, width, 3), text


def png_comment(text):
    return json.loads(text["Comment"])
