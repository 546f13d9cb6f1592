"""Plume label masks and connected components on the GPU.

Mirrors the reference's starcop/data/mask_creation.py:6-27 (proposed_mask: the ``labelbinary`` target of every sample folder)
and the caching of that target in starcop/data/sampling_dataset.py:453-460 (_cache_data_permian_2019).
All compute runs in libstarcop_hip.so (include/starcop_hip.h: sc_proposed_mask, sc_connected_components).
"""
import os

import numpy as np
import torch

from . import _lib, stacks
from ._lib import check, ptr, stream

THRESHOLD = 200.0          # mask_creation.py:11: mag1c_values[0] >= 200


def _workspace(N, H, W, dev):
    wb = _lib.load().sc_label_workspace_bytes(N, H, W)          # 0 for bad dims: the call itself then raises with the dims message
    return torch.empty(max(wb, 1), dtype=torch.uint8, device=dev), wb


def _proposed_mask_device(label_rgba, mag1c, threshold, se_bits):
    """label_rgba (B, C, H, W) / mag1c (B, Cm, H, W) device tensors -> (B, H, W) device bool"""
    lib = _lib.load()
    if label_rgba.dim() != 4 or mag1c.dim() != 4:
        raise ValueError("proposed_mask: expected (C, H, W) or (B, C, H, W) label_rgba and mag1c")
    if label_rgba.shape[0] != mag1c.shape[0] or label_rgba.shape[-2:] != mag1c.shape[-2:]:
        raise ValueError(f"proposed_mask: label_rgba {tuple(label_rgba.shape)} and mag1c {tuple(mag1c.shape)} differ in shape")
    _lib.require_device(label_rgba)
    _lib.require_device(mag1c)
    B, H, W = mag1c.shape[0], mag1c.shape[-2], mag1c.shape[-1]
    alpha, astride = stacks.plane_operand(label_rgba[:, -1], torch.uint8)      # existing label: the last band, != 0
    mag, mstride = stacks.plane_operand(mag1c[:, 0], torch.float32)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=mag.device)
    work, wb = _workspace(B, H, W, mag.device)
    check(lib.sc_proposed_mask(ptr(mag), mstride, ptr(alpha), astride, float(threshold), int(se_bits), ptr(out), ptr(work), wb,
                               B, H, W, stream()))
    return out.view(torch.bool)


def proposed_mask(label_rgba_values, mag1c_values, threshold=THRESHOLD, se_bits=_lib.SE_CROSS):
    """mask_creation.py:6-27: the mag1c >= threshold pixels of every connected component (8-connectivity) of
    dilation(opening(mag1c >= threshold, disk(1)), disk(1)) that touches a hand-labelled pixel (label_rgba's last band != 0).

    numpy (C, H, W) arrays -> (H, W) numpy bool, computed on the GPU; device tensors (C, H, W) or (B, C, H, W) -> device bool
    (H, W) or (B, H, W).  mag1c is band 0 of ``mag1c_values``."""
    if isinstance(label_rgba_values, np.ndarray) or isinstance(mag1c_values, np.ndarray):
        lab = torch.from_numpy(np.ascontiguousarray(label_rgba_values))
        mag = torch.from_numpy(np.ascontiguousarray(mag1c_values, dtype=np.float32))
        if lab.dim() != 3 or mag.dim() != 3:
            raise ValueError("proposed_mask: numpy inputs are (C, H, W) arrays")
        _lib.require_device()
        if lab.dtype != torch.uint8:
            lab = (lab[-1:] != 0).to(torch.uint8)
        return _proposed_mask_device(lab[None].cuda(), mag[None].cuda(), threshold, se_bits)[0].cpu().numpy()
    lab, mag = label_rgba_values, mag1c_values
    if lab.dim() == 3 and mag.dim() == 3:
        return _proposed_mask_device(lab[None], mag[None], threshold, se_bits)[0]
    return _proposed_mask_device(lab, mag, threshold, se_bits)


def connected_components(mask, connectivity=2):
    """skimage.measure.label / scipy.ndimage.label of ``mask != 0``: connectivity 1 (4-neighbours) or 2 (8-neighbours, the
    default of skimage for 2-D images).  (H, W) or (N, H, W) -> (labels int32 of the same shape, counts): background 0,
    components numbered from 1 in the raster order of their first pixel.  numpy in -> numpy labels and an int (H, W) or an
    (N,) int64 array of counts; device tensor in -> device labels and device int32 counts (an int for (H, W))."""
    lib = _lib.load()
    stacks.check_stack(mask, "connected_components", "mask")
    m3, single, host = stacks.device_mask(mask)
    m3 = m3.contiguous()                           # the kernel takes no strides
    N, H, W = m3.shape
    labels = torch.empty((N, H, W), dtype=torch.int32, device=m3.device)
    counts = torch.empty((N,), dtype=torch.int32, device=m3.device)
    work, wb = _workspace(N, H, W, m3.device)
    check(lib.sc_connected_components(ptr(m3), int(connectivity), ptr(labels), ptr(counts), ptr(work), wb, N, H, W, stream()))
    labels = stacks.finish(labels, single, host)
    if single:
        return labels, int(counts[0].item())
    return labels, (counts.cpu().numpy().astype(np.int64) if host else counts)


def write_label_masks(dataframe, batch_size=16, overwrite=False, threshold=THRESHOLD, device=None):
    """sampling_dataset.py:453-460 / 298-303: for every row's ``folder``, read ``mag1c.tif`` and ``label_rgba.tif``, compute
    proposed_mask and write ``labelbinary.tif`` there (uint8, tiled 128 x 128, mag1c's georeferencing without a nodata value,
    "labelbinary" as band description).  Existing files are left alone unless ``overwrite``.  Folders of one shape are computed
    in batches of ``batch_size`` per launch.  Every input is checked before anything is written: a missing product raises
    FileNotFoundError, mag1c and label_rgba of different sizes ValueError."""
    from . import io_formats as io
    device = torch.device(device if device is not None else "cuda")
    folders = [str(f) for f in dataframe["folder"]]
    todo = [d for d in folders if overwrite or not os.path.exists(os.path.join(d, "labelbinary.tif"))]
    infos = {}
    for d in todo:
        for prod in ("mag1c", "label_rgba"):
            path = os.path.join(d, f"{prod}.tif")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{d}: missing {prod}.tif, needed for labelbinary.tif")
        mi, li = io.tiff_info(os.path.join(d, "mag1c.tif")), io.tiff_info(os.path.join(d, "label_rgba.tif"))
        if (mi.height, mi.width) != (li.height, li.width):
            raise ValueError(f"{d}: mag1c.tif is {mi.height} x {mi.width} but label_rgba.tif is {li.height} x {li.width}")
        infos[d] = mi
    by_shape = {}
    for d in todo:
        by_shape.setdefault((infos[d].height, infos[d].width), []).append(d)
    for group in by_shape.values():
        for s in range(0, len(group), batch_size):
            chunk = group[s:s + batch_size]
            mag = np.stack([io.read_tiff(os.path.join(d, "mag1c.tif"))[:1].astype(np.float32) for d in chunk])
            alpha = np.stack([io.read_tiff(os.path.join(d, "label_rgba.tif"))[-1:] != 0 for d in chunk]).astype(np.uint8)
            out = _proposed_mask_device(torch.from_numpy(alpha).to(device), torch.from_numpy(mag).to(device), threshold,
                                        _lib.SE_CROSS).cpu().numpy().astype(np.uint8)
            for d, o in zip(chunk, out):
                tags = {t: v for t, v in infos[d].geo_tags().items() if t not in (42112, 42113)}     # fill_value_default None
                tags.update(io.gdal_metadata_tag({}, ["labelbinary"]))
                io.write_tiff(os.path.join(d, "labelbinary.tif"), o, blocksize=128, extra_tags=tags)
