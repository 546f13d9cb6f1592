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


def write_mag1c_flight_line(parent, nl=96, ns=40, seed=5):
    """the flight line the matched filter is tested on, as ``{parent}/ang20190101t000000_rdn/<name>_img`` + ``<name>_glt`` (ENVI,
    BIP): 101 bands on a 5 nm grid from 2000 to 2500 nm (74 of them inside [2122, 2488] nm and outside the bad-band windows), a
    weak CH4 signal in a rectangle, 23 detector groups that vary along a row AND down, a no-data border of 5 lines and negative
    (interpolated) indices; a rotated ``map info`` and no data ignore value.  -> (folder, cube, glt, wl, fwhm, target)"""
    from starcop_amd import mag1c
    rng = np.random.default_rng(seed)
    wl = np.linspace(2000.0, 2500.0, 101)
    fwhm = np.full_like(wl, 5.6)
    target = mag1c.generate_template_from_bands(wl, fwhm)[:, 1]
    cube = (rng.uniform(1, 6, size=wl.size) * (1 + 0.05 * rng.standard_normal((nl, ns, wl.size)))).astype(np.float32)
    k = np.zeros((nl, ns)); k[30:50, 10:20] = 2e-5
    cube = (cube * (1 + k[..., None] * np.nan_to_num(target))).astype(np.float32)
    glt = np.zeros((nl, ns, 2), dtype=np.int32)
    glt[..., 0] = (np.arange(ns)[None, :] + (np.arange(nl)[:, None] // 8)) % 23 + 1      # orthorectified: detector sample varies along a row AND down
    glt[:5, :, 0] = 0                                                                    # no-data border
    glt[..., 0] *= np.where(rng.random((nl, ns)) < 0.5, 1, -1)                           # interpolated pixels carry a negative index
    glt[..., 1] = np.arange(nl)[:, None]
    name = "ang20190101t000000_rdn"
    folder = os.path.join(str(parent), name)
    os.makedirs(folder)
    for suffix, arr, dt, extra in (("img", cube, 4, f"wavelength = {{ {', '.join(f'{v:.4f}' for v in wl)} }}\nfwhm = {{ {', '.join(f'{v:.2f}' for v in fwhm)} }}\n"
                                    "map info = {UTM, 1, 1, 500000.0, 4100000.0, 5.0, 5.0, 11, North, WGS-84, units=Meters, rotation=-12.0}\n"),
                                   ("glt", glt, 3, "")):
        arr.tofile(os.path.join(folder, f"{name}_{suffix}"))
        with open(os.path.join(folder, f"{name}_{suffix}.hdr"), "w") as f:
            f.write(f"ENVI\nsamples = {ns}\nlines = {nl}\nbands = {arr.shape[2]}\nheader offset = 0\n"
                    f"data type = {dt}\ninterleave = bip\nbyte order = 0\n{extra}")
    return folder, cube, glt, wl, fwhm, target
