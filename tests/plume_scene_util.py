"""numpy restatements of the whole-flight-line plume path (sc_scene_gather_planes / sc_scene_core_counts / ModelModule.predict_scene /
pipeline.aviris_scene_predict), the seeded flight-line-like scenes of its tests and their ENVI writer.  Builds on scene_util.py."""
import os

import numpy as np

from scene_util import gather_ref, paste_cores

FILL = -9999.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fill_bits(value):
    return int(np.array(value, dtype=np.float32).view(np.uint32))


def prepare_plane(x, fill=None, scale=None, clip=None):
    """what WindowDataset does to a product before it becomes a network input, the fill compared as a bit pattern:
    np.where(bits == fill, 0, x * float32(s)), then np.clip"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = x * np.float32(scale) if scale is not None else x.copy()
    if fill is not None:
        y = np.where(bits(x) == fill_bits(fill), np.float32(0), y)
    if clip is not None:
        y = np.clip(y, np.float32(clip[0]), np.float32(clip[1]))
    return y.astype(np.float32)


def prepare_planes(planes, fills, scales, clips):
    return np.stack([prepare_plane(p, f, s, c) for p, f, s, c in zip(planes, fills, scales, clips)])


def gather_planes_ref(planes, fills, scales, clips, pad_rows, pad_cols, offsets, window):
    """fill / scale / clip per plane, np.pad(reflect), slices -> (n, P, wh, ww)"""
    return gather_ref(prepare_planes(planes, fills, scales, clips), pad_rows, pad_cols, offsets, window)


def core_counts_ref(plane, fill, plan):
    """pixels of every core's destination rectangle whose bits differ from the fill's"""
    valid = bits(plane) != fill_bits(fill)
    out = []
    for (y0, y1, x0, x1), (dr, dc) in zip(plan.cores.tolist(), plan.dests.tolist()):
        out.append(int(valid[dr:dr + y1 - y0, dc:dc + x1 - x0].sum()) if y1 > y0 and x1 > x0 else 0)
    return np.asarray(out, dtype=np.int32)


def strip_mask(H, W, centre=120.0, slope=0.35, half_width=110.0, first_row=0):
    """the valid pixels of a flight-line-like scene: a slanted strip |x - (centre + slope * y)| < half_width that begins at row
    ``first_row`` of the rectangle"""
    y, x = np.mgrid[0:H, 0:W]
    return (np.abs(x - (centre + slope * y)) < half_width) & (y >= first_row)


def flight_line(H, W, seed, valid=None, factor=1.037):
    """seeded raw products of the default model (mag1c, three radiance bands) of an (H, W) orthorectified flight line: mag1c ~
    600 N(0, 1) + 200, radiance ~ U(0.5, 12), FILL outside the slanted valid strip; the bands are ONE (H, W, 3) buffer.
    -> (planes [mag1c, r, g, b], fills, scales, clips, valid)"""
    rng = np.random.default_rng(seed)
    valid = strip_mask(H, W) if valid is None else valid
    mf = (600.0 * rng.standard_normal((H, W)) + 200.0).astype(np.float32)
    rgb = rng.uniform(0.5, 12.0, size=(H, W, 3)).astype(np.float32)
    mf[~valid] = FILL
    rgb[~valid] = FILL
    planes = [mf, rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]]
    return planes, [FILL] * 4, [None, factor, factor, factor], [(0.0, 10000.0), None, None, None], valid


def predict_scene_ref(forward, planes, fills, scales, clips, plan, nodata=FILL):
    """the restatement of ModelModule.predict_scene: windows cut in numpy, ``forward`` ((1, C, wh, ww) float32 array -> ((wh, ww)
    float32 probability, (wh, ww) mask)) one window at a time, cores pasted, the first plane's fill pixels set to nodata / 0"""
    H, W = planes[0].shape
    wins = gather_planes_ref(planes, fills, scales, clips, plan.pad_rows, plan.pad_cols, plan.offsets.tolist(), plan.window)
    res = [forward(w[None]) for w in wins]
    prob = paste_cores(np.stack([r[0] for r in res]).astype(np.float32), plan, H, W)
    mask = paste_cores(np.stack([r[1] for r in res]).astype(np.uint8), plan, H, W)
    if fills[0] is not None:
        hole = bits(planes[0]) == fill_bits(fills[0])
        prob[hole] = np.float32(nodata)
        mask[hole] = 0
    return prob, mask


MAP_INFO = "{UTM, 1, 1, 500000.0, 4100000.0, 5.0, 5.0, 11, North, WGS-84, units=Meters}"


def write_flight_line(folder, cube, wavelengths, fill=FILL, map_info=MAP_INFO):
    """cube (lines, samples, bands) float32 -> {folder}/{name}_img + .hdr (ENVI, BIP) with band centres, map info and the data
    ignore value"""
    os.makedirs(folder, exist_ok=True)
    name = os.path.basename(str(folder).rstrip("/"))
    np.ascontiguousarray(cube, dtype=np.float32).tofile(os.path.join(folder, f"{name}_img"))
    with open(os.path.join(folder, f"{name}_img.hdr"), "w") as f:
        f.write(f"ENVI\nsamples = {cube.shape[1]}\nlines = {cube.shape[0]}\nbands = {cube.shape[2]}\nheader offset = 0\ndata type = 4\n"
                f"interleave = bip\nbyte order = 0\nwavelength units = Nanometers\n"
                f"wavelength = {{ {', '.join(f'{v:.4f}' for v in wavelengths)} }}\n"
                f"map info = {map_info}\ndata ignore value = {fill:g}\n")
    return str(folder)
