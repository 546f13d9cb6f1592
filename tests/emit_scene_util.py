"""Fake EMIT evaluation scenes on disk: ENVI ``*_radiance_RGB`` / ``*_radiance_magic`` files (numpy + a header) and a label GeoTIFF."""
import os

import numpy as np


def write_envi(path, cube):
    """(bands, lines, samples) float32 array -> BSQ ENVI file ``path`` with ``path.hdr``"""
    cube = np.ascontiguousarray(cube, dtype="<f4")
    cube.tofile(path)
    with open(path + ".hdr", "w") as fh:
        fh.write(f"ENVI\nsamples = {cube.shape[2]}\nlines = {cube.shape[1]}\nbands = {cube.shape[0]}\nheader offset = 0\n"
                 "file type = ENVI Standard\ndata type = 4\ninterleave = bsq\nbyte order = 0\n")


def write_scene(root, kind, name, rgb, magic, label=None, labels_name="label.tif"):
    from starcop_amd import io_formats as io
    d = os.path.join(str(root), kind, name)
    os.makedirs(d)
    write_envi(os.path.join(d, f"{name}_radiance_RGB"), rgb)
    write_envi(os.path.join(d, f"{name}_radiance_magic"), magic[None])
    if label is not None:
        io.write_tiff(os.path.join(d, labels_name), label)
    return d
