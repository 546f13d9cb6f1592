"""On-the-fly input features of the hot path, on the GPU.

Mirrors /root/reference/starcop/data/feature_extration.py:
  weight_mag1c :32-35, no_outliers :37-40, ratio_2c_match_c_from_sums_outlier :42-56 (e.g. the registered product
  ``ratio_aviris_2350_2310_out`` :196), and the EMIT->AVIRIS value-range rescale of
  starcop/emit_tools/emit_dataset.py:62-106 (the same constants as notebook inference_on_raw_EMIT_nc_file cell 17).
Tensors live on the device; tiles are batched (B, H, W) so that one launch handles a batch of tiles.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr, stream


def _as_tiles(t):
    t = torch.as_tensor(t)
    _lib.require_device(t)
    t = t.contiguous().float()
    lead = t.shape[:-2]
    B = 1
    for d in lead:
        B *= int(d)
    return t, B, int(t.shape[-2] * t.shape[-1])


def trimmed_sums(x, p=5):
    """np.sum(no_outliers(tile, p)) for every (H, W) tile of ``x`` -> float64 tensor of the leading shape."""
    lib = _lib.load()
    x, B, n = _as_tiles(x)
    sums = torch.empty(B, dtype=torch.float64, device=x.device)
    wb = lib.sc_trimmed_sum_workspace_bytes(B)
    work = torch.empty(wb, dtype=torch.uint8, device=x.device)
    check(lib.sc_trimmed_sums(ptr(x), B, n, float(p), ptr(sums), ptr(work), wb, stream()))
    return sums.reshape(x.shape[:-2])


def ratio_2c_match_c_from_sums_outlier(background_channel, signal, p=5, zero_value_out=-.6):
    """Varon-style two-band ratio: R = (c*signal - background)/(background + 1e-6) with c matching the 5-95 % trimmed
    sums of the two bands; pixels where both bands are < 1e-6 get ``zero_value_out``.  Same argument order as the
    reference (it is called as ``f(band_absorbing, band_reference)``)."""
    lib = _lib.load()
    bg, B, n = _as_tiles(background_channel)
    sg, B2, n2 = _as_tiles(signal)
    if (B, n) != (B2, n2):
        raise ValueError("background and signal tiles must have the same shape")
    s_bg, s_sg = trimmed_sums(bg, p).reshape(-1), trimmed_sums(sg, p).reshape(-1)
    out = torch.empty_like(sg)
    check(lib.sc_band_ratio(ptr(bg), ptr(sg), ptr(out), B, n, ptr(s_bg), ptr(s_sg), 0.0, float(zero_value_out), stream()))
    return out


def _clip_scale(x, div, lo, hi, mult, nan_to_num=False):
    lib = _lib.load()
    x = torch.as_tensor(x)
    _lib.require_device(x)
    x = x.contiguous().float()
    out = torch.empty_like(x)
    check(lib.sc_clip_scale(ptr(x), ptr(out), x.numel(), float(div), float(lo), float(hi), float(mult), int(nan_to_num), stream()))
    return out


def weight_mag1c(mag1c):
    """Loss weight of a pixel: clip(mag1c / 400, 0.1, 1)."""
    return _clip_scale(mag1c, 400.0, 0.1, 1.0, 1.0)


# constants of emit_dataset.py:62-69
MAGIC_DIV_BY, RGB_DIV_BY, MAGIC_MULT_BY, RGB_MULT_BY = 240., 20., 1750., 60.


def emit_to_aviris_input(mf, rgb):
    """(H, W) mag1c + (3, H, W) RGB radiance of an EMIT scene -> (4, H', W') network input in the AVIRIS value range:
    crop to multiples of 32, clip(mf/240, 0, 2)*1750, clip(rgb/20, 0, 2)*60, nan_to_num."""
    mf, rgb = torch.as_tensor(mf), torch.as_tensor(rgb)
    h, w = (mf.shape[-2] // 32) * 32, (mf.shape[-1] // 32) * 32
    out = torch.empty((4, h, w), dtype=torch.float32, device=mf.device)
    out[0] = _clip_scale(mf[:h, :w], MAGIC_DIV_BY, 0.0, 2.0, MAGIC_MULT_BY, nan_to_num=True)
    out[1:] = _clip_scale(rgb[:, :h, :w], RGB_DIV_BY, 0.0, 2.0, RGB_MULT_BY, nan_to_num=True)
    return out


# ------------------------------------------------------------------------------------------------ Sanchez-Garcia MLR ratio
# feature_extration.py:58-125: per-tile least squares of a target band on k regressor bands, then a division of the target by
# the prediction (include/starcop_hip.h: sc_mlr_*)
MLR_DIVISIONS = {"c_matched_outliers": _lib.MLR_C_MATCHED, "simple_plus": _lib.MLR_SIMPLE_PLUS, "residual": _lib.MLR_RESIDUAL}


def _tile_layout(t):
    """(B, floats between tiles) of a float32 (..., H, W) tensor whose tiles are dense planes at one stride, else None."""
    if t.dtype != torch.float32 or t.dim() < 2:
        return None
    H, W = t.shape[-2:]
    if (W > 1 and t.stride(-1) != 1) or (H > 1 and t.stride(-2) != W):
        return None
    lead = [(int(d), int(s)) for d, s in zip(t.shape[:-2], t.stride()[:-2]) if d != 1]
    for (_, s0), (d1, s1) in zip(lead[:-1], lead[1:]):
        if s0 != d1 * s1:
            return None
    B = 1
    for d, _ in lead:
        B *= d
    return B, (lead[-1][1] if lead else 0)


def _mlr_operands(bands_bg, target):
    """regressors (a list of (..., H, W) tensors or one (..., k, H, W) tensor) and the (..., H, W) target -> sc_mlr_args.
    Planes that are views of one storage at a common tile stride (e.g. bands of a stacked (B, 8, H, W) tensor) are read in
    place; anything else is stacked into a dense (B, k, H, W) copy first."""
    if isinstance(bands_bg, (list, tuple)):
        planes = [torch.as_tensor(b) for b in bands_bg]
    else:
        x = torch.as_tensor(bands_bg)
        planes = [x[..., j, :, :] for j in range(x.shape[-3])]
    target = torch.as_tensor(target)
    k = len(planes)
    if not 1 <= k <= 9:
        raise ValueError(f"the MLR ratio takes 1..9 regressor bands, got {k}")
    for p in planes + [target]:
        _lib.require_device(p)
    shape = tuple(target.shape)
    if len(shape) < 2 or any(tuple(p.shape) != shape for p in planes):
        raise ValueError("regressor and target tiles must all have the target's (..., H, W) shape")
    H, W = shape[-2:]
    n = H * W
    lay = [_tile_layout(p) for p in planes]
    if None in lay or len(set(lay)) != 1 or len({p.untyped_storage().data_ptr() for p in planes}) != 1:
        x = torch.stack([p.float().reshape(-1, H, W) for p in planes], 1).contiguous()
        planes = [x[:, j] for j in range(k)]
        lay = [(x.shape[0], k * n)]
    B, ts = lay[0]
    tl = _tile_layout(target)
    if tl is None:
        target = target.float().contiguous()
        tl = (B, n)
    a = _lib.sc_mlr_args()
    base = planes[0].data_ptr()
    a.base = base
    for j, p in enumerate(planes):
        a.band_off[j] = (p.data_ptr() - base) // 4
    a.k, a.B, a.n = k, B, n
    a.tile_stride = ts if B > 1 else 0
    a.target = target.data_ptr()
    a.target_tile_stride = tl[1] if B > 1 else 0
    return a, (planes, target), shape


def _mlr(bands_bg, target, division=None, autoclip=False):
    if division is not None and division not in MLR_DIVISIONS:
        raise ValueError(f"unknown division {division!r}: one of {sorted(MLR_DIVISIONS)} "
                         "('simple' is unreachable in the reference: it ends in assert False)")
    lib = _lib.load()
    a, keep, shape = _mlr_operands(bands_bg, target)
    dev = keep[1].device
    wb = lib.sc_mlr_workspace_bytes(a.B, a.n, a.k)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    coef = torch.empty((a.B, a.k + 1), dtype=torch.float64, device=dev)
    check(lib.sc_mlr_fit(C.byref(a), ptr(coef), ptr(work), wb, stream()))
    if division is None:
        return coef, shape
    r = None
    if division == "c_matched_outliers":          # the trimmed sums are taken on the stored prediction
        r = torch.empty((a.B, a.n), dtype=torch.float32, device=dev)
        check(lib.sc_mlr_predict(C.byref(a), ptr(coef), ptr(r), stream()))
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    check(lib.sc_mlr_ratio(C.byref(a), ptr(coef), ptr(r), MLR_DIVISIONS[division], int(bool(autoclip)), ptr(out), ptr(work), wb,
                           stream()))
    return out


def mlr_fit(bands_bg, target):
    """Least squares with intercept of every (H, W) target tile on its k regressor bands, over all pixels
    (sklearn LinearRegression().fit as ratio_MLR_local does) -> (coef (..., k), intercept (...)), float64 device tensors.
    A zero-variance band gets coefficient 0 (the minimum-norm solution)."""
    coef, shape = _mlr(bands_bg, target)
    lead = shape[:-2]
    return coef[:, :-1].reshape(*lead, coef.shape[1] - 1), coef[:, -1].reshape(lead)


def ratio_MLR_local(bands_bg, band_target_signal, division="c_matched_outliers", autoclip=False):
    """feature_extration.py:58-109 for every (H, W) tile: ``bands_bg`` is a list of k (..., H, W) device tensors or one
    (..., k, H, W) tensor, ``band_target_signal`` (..., H, W); returns float32 of the target's shape."""
    return _mlr(bands_bg, band_target_signal, division, autoclip)


def ratio_MLR_local_5IN(IN1, IN2, IN3, IN4, IN5, target_B, division="c_matched_outliers", autoclip=False):
    return ratio_MLR_local([IN1, IN2, IN3, IN4, IN5], target_B, division=division, autoclip=autoclip)


def ratio_MLR_local_9IN(IN1, IN2, IN3, IN4, IN5, IN6, IN7, IN8, IN9, target_B, division="c_matched_outliers", autoclip=False):
    return ratio_MLR_local([IN1, IN2, IN3, IN4, IN5, IN6, IN7, IN8, IN9], target_B, division=division, autoclip=autoclip)


def ratio_MLR_local_5IN_simplediv(IN1, IN2, IN3, IN4, IN5, target_B, division="simple_plus", autoclip=False):
    return ratio_MLR_local([IN1, IN2, IN3, IN4, IN5], target_B, division=division, autoclip=autoclip)


def use_pretrained_model_b1to6_b8(*inputs, **kwargs):
    raise NotImplementedError("ratio_lrn_bands2band8only_60ep_512_l1 needs the reference's remote regression checkpoint "
                              "(ModelModuleRegression), which this project does not ship")


# ------------------------------------------------------------------------------------------------ the feature registry
WV3_BANDS = [f"TOA_WV3_SWIR{w + 1}" for w in range(8)]
_WV3_MLR_IN = ["TOA_WV3_SWIR1", "TOA_WV3_SWIR2", "TOA_WV3_SWIR4", "TOA_WV3_SWIR5", "TOA_WV3_SWIR6"]
_S2_9IN = ["TOA_S2B_B2", "TOA_S2B_B3", "TOA_S2B_B4", "TOA_S2B_B5", "TOA_S2B_B6", "TOA_S2B_B7", "TOA_S2B_B8", "TOA_S2B_B8A", "TOA_S2B_B11"]
_S2_5IN = ["TOA_S2B_B2", "TOA_S2B_B3", "TOA_S2B_B4", "TOA_S2B_B8", "TOA_S2B_B11"]


def _entry(function, inputs):
    return {"function": function, "inputs": list(inputs), "fill_value_default": None}


# feature_extration.py:193-246: product name -> function, input products (in call order), fill value
FEATURES = {
    "weight_mag1c": _entry(weight_mag1c, ["mag1c"]),
    "ratio_aviris_2350_2310_out": _entry(ratio_2c_match_c_from_sums_outlier, ["TOA_AVIRIS_2350nm", "TOA_AVIRIS_2310nm"]),
    "ratio_aviris_2350_2360_out": _entry(ratio_2c_match_c_from_sums_outlier, ["TOA_AVIRIS_2350nm", "TOA_AVIRIS_2360nm"]),
    "ratio_aviris_2360_2310_out": _entry(ratio_2c_match_c_from_sums_outlier, ["TOA_AVIRIS_2360nm", "TOA_AVIRIS_2310nm"]),
    "ratio_wv3_B7_B5_varon21_sum_c_out": _entry(ratio_2c_match_c_from_sums_outlier, ["TOA_WV3_SWIR7", "TOA_WV3_SWIR5"]),
    "ratio_wv3_B8_B5_varon21_sum_c_out": _entry(ratio_2c_match_c_from_sums_outlier, ["TOA_WV3_SWIR8", "TOA_WV3_SWIR5"]),
    "ratio_wv3_B7_B6_varon21_sum_c_out": _entry(ratio_2c_match_c_from_sums_outlier, ["TOA_WV3_SWIR7", "TOA_WV3_SWIR6"]),
    "ratio_wv3_B7_B7MLR_SanchezGarcia22_sum_c_out": _entry(ratio_MLR_local_5IN, _WV3_MLR_IN + ["TOA_WV3_SWIR7"]),
    "ratio_wv3_B8_B8MLR_SanchezGarcia22_sum_c_out": _entry(ratio_MLR_local_5IN, _WV3_MLR_IN + ["TOA_WV3_SWIR8"]),
    "ratio_wv3_B7_B7MLR_SanchezGarcia22_simplediv": _entry(ratio_MLR_local_5IN_simplediv, _WV3_MLR_IN + ["TOA_WV3_SWIR7"]),
    "ratio_wv3_B8_B8MLR_SanchezGarcia22_simplediv": _entry(ratio_MLR_local_5IN_simplediv, _WV3_MLR_IN + ["TOA_WV3_SWIR8"]),
    "ratio_lrn_bands2band8only_60ep_512_l1": _entry(use_pretrained_model_b1to6_b8, ["TOA_WV3_SWIR1", "TOA_WV3_SWIR2", "TOA_WV3_SWIR3",
                                                                                    "TOA_WV3_SWIR4", "TOA_WV3_SWIR5", "TOA_WV3_SWIR6",
                                                                                    "TOA_WV3_SWIR8"]),
    "ratio_wv3_B7_B7MLR_fromS2_9bands_sum_c_out": _entry(ratio_MLR_local_9IN, _S2_9IN + ["TOA_WV3_SWIR7"]),
    "ratio_wv3_B7_B7MLR_fromS2_5bands_sum_c_out": _entry(ratio_MLR_local_5IN, _S2_5IN + ["TOA_WV3_SWIR7"]),
    "ratio_wv3_B8_B8MLR_fromS2_9bands_sum_c_out": _entry(ratio_MLR_local_9IN, _S2_9IN + ["TOA_WV3_SWIR8"]),
    "ratio_wv3_B8_B8MLR_fromS2_5bands_sum_c_out": _entry(ratio_MLR_local_5IN, _S2_5IN + ["TOA_WV3_SWIR8"]),
}


def extract_features(features, dataframe, batch_size=16, device=None):
    """feature_extration.py:249-286: for every row's ``folder``, compute each product of ``features`` whose
    ``{folder}/{feature}.tif`` does not exist yet from its input products and write it there (tiled 128 x 128, the first
    input's georeferencing, the product name as band description).  Tiles of one shape are computed in batches of
    ``batch_size`` per launch.  Existing files are left alone, so a second call writes nothing."""
    import os
    import numpy as np
    from . import io_formats as io
    unknown = [f for f in features if f not in FEATURES]
    if unknown:
        raise KeyError(f"unknown features {unknown}: known are {sorted(FEATURES)}")
    device = torch.device(device if device is not None else "cuda")
    folders = [str(f) for f in dataframe["folder"]]
    for f in features:
        todo = [d for d in folders if not os.path.exists(os.path.join(d, f"{f}.tif"))]
        if not todo:
            continue
        fn, inputs = FEATURES[f]["function"], FEATURES[f]["inputs"]
        infos = {d: io.tiff_info(os.path.join(d, f"{inputs[0]}.tif")) for d in todo}
        by_shape = {}
        for d in todo:
            by_shape.setdefault((infos[d].height, infos[d].width), []).append(d)
        for group in by_shape.values():
            for s in range(0, len(group), batch_size):
                chunk = group[s:s + batch_size]
                x = torch.from_numpy(np.stack([io.load_sample(d, inputs) for d in chunk])).to(device)   # (b, inputs, H, W)
                out = fn(*[x[:, i] for i in range(len(inputs))]).float().cpu().numpy()
                for d, o in zip(chunk, out):
                    tags = {t: v for t, v in infos[d].geo_tags().items() if t != 42113}       # fill_value_default None: no nodata
                    tags.update(io.gdal_metadata_tag({}, [f]))
                    io.write_tiff(os.path.join(d, f"{f}.tif"), o, blocksize=128, extra_tags=tags)
