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


MAGIC_CLIP_TO, RGB_CLIP_TO = (0., 2.), (0., 2.)


def emit_to_aviris_input(mf, rgb=None, magic_div_by=MAGIC_DIV_BY, rgb_div_by=RGB_DIV_BY, magic_clip_to=MAGIC_CLIP_TO,
                         rgb_clip_to=RGB_CLIP_TO, magic_mult_by=MAGIC_MULT_BY, rgb_mult_by=RGB_MULT_BY):
    """(H, W) mag1c + (3, H, W) RGB radiance of an EMIT scene -> (4, H', W') network input in the AVIRIS value range:
    crop to multiples of 32, clip(mf/240, 0, 2)*1750, clip(rgb/20, 0, 2)*60, nan_to_num.  The six constants are the
    ``hyperparams`` of emit_dataset.py:52-69; ``rgb=None`` is its one-channel ``mag1c_only`` mode."""
    mf = torch.as_tensor(mf)
    h, w = (mf.shape[-2] // 32) * 32, (mf.shape[-1] // 32) * 32
    out = torch.empty((1 if rgb is None else 4, h, w), dtype=torch.float32, device=mf.device)
    out[0] = _clip_scale(mf[:h, :w], magic_div_by, magic_clip_to[0], magic_clip_to[1], magic_mult_by, nan_to_num=True)
    if rgb is not None:
        out[1:] = _clip_scale(torch.as_tensor(rgb)[:, :h, :w], rgb_div_by, rgb_clip_to[0], rgb_clip_to[1], rgb_mult_by, nan_to_num=True)
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


# ------------------------------------------------------------------------------------------------ learned band ratio
# feature_extration.py:127-175: a cnn_v2 regression model predicts WV3 band 8 from bands 1-6; the product is the matched ratio of
# the real band 8 against that prediction.  The reference pulls its checkpoint from a bucket on first use; here the model is
# handed over explicitly with set_learned_model() -- the project ships no weights.
_learned_model = None


def set_learned_model(module_or_checkpoint_path, settings=None):
    """The model behind ``ratio_lrn_bands2band8only_60ep_512_l1``: a module mapping (B, 6, H, W) to (B, 1, H, W) (a
    ``ModelModuleRegression`` or a bare ``SimpleCNN_v2(6, 1)``), or the path of a local ``ModelModuleRegression`` checkpoint to
    load with ``settings``.  ``None`` unsets it.  Returns the module."""
    global _learned_model
    m = module_or_checkpoint_path
    if isinstance(m, (str, bytes)) or hasattr(m, "__fspath__"):
        path = m.decode() if isinstance(m, bytes) else str(m)
        if path.startswith("gs://"):
            raise NotImplementedError(f"{path}: remote checkpoints are not fetched; copy the file and pass its local path")
        if settings is None:
            raise ValueError("set_learned_model(path) needs the settings the checkpoint was trained with")
        from .model_module_regression import ModelModuleRegression
        m = ModelModuleRegression.load_from_checkpoint(path, settings=settings)
        m = m.to("cuda")
    if m is not None:
        m.eval()
    _learned_model = m
    return m


def use_pretrained_model_b1to6_b8(*inputs, **kwargs):
    """feature_extration.py:152-175 for every (H, W) tile: stack bands 1-6, run the learned model, then
    ``ratio_2c_match_c_from_sums_outlier(target, output, zero_value_out=-0.5)`` with -0.5 where the target band is 0."""
    if _learned_model is None:
        raise NotImplementedError("ratio_lrn_bands2band8only_60ep_512_l1 needs the reference's regression checkpoint "
                                  "(wv3_cnn_v2_bands2band8only_60ep_512_l1), which this project does not ship: load one with "
                                  "features.set_learned_model(module_or_checkpoint_path, settings)")
    if kwargs or len(inputs) != 7:
        raise TypeError("use_pretrained_model_b1to6_b8(inB1, inB2, inB3, inB4, inB5, inB6, outB8)")
    bands = [torch.as_tensor(b) for b in inputs]
    for b in bands:
        _lib.require_device(b)
    target = bands[6].contiguous().float()
    shape = tuple(target.shape)
    if len(shape) < 2 or any(tuple(b.shape) != shape for b in bands):
        raise ValueError("the six input bands and the target band must all have one (..., H, W) shape")
    H, W = shape[-2:]
    x = torch.stack([b.float().reshape(-1, H, W) for b in bands[:6]], 1).contiguous()          # (B, 6, H, W)
    with torch.no_grad():
        output = _learned_model(x)
    if tuple(output.shape) != (x.shape[0], 1, H, W):
        raise ValueError(f"the learned model must map (B, 6, H, W) to (B, 1, H, W), got {tuple(output.shape)}")
    tgt = target.reshape(-1, H, W)
    R = ratio_2c_match_c_from_sums_outlier(tgt, output[:, 0], zero_value_out=-0.5)
    R[tgt == 0] = -0.5
    return R.reshape(shape)


# ------------------------------------------------------------------------------------------------ the feature registry
WV3_BANDS = [f"TOA_WV3_SWIR{w + 1}" for w in range(8)]
_WV3_MLR_IN = ["TOA_WV3_SWIR1", "TOA_WV3_SWIR2", "TOA_WV3_SWIR4", "TOA_WV3_SWIR5", "TOA_WV3_SWIR6"]
_S2_9IN = ["TOA_S2B_B2", "TOA_S2B_B3", "TOA_S2B_B4", "TOA_S2B_B5", "TOA_S2B_B6", "TOA_S2B_B7", "TOA_S2B_B8", "TOA_S2B_B8A", "TOA_S2B_B11"]
_S2_5IN = ["TOA_S2B_B2", "TOA_S2B_B3", "TOA_S2B_B4", "TOA_S2B_B8", "TOA_S2B_B11"]


# ------------------------------------------------------------------------------------------------ raw products
# feature_extration.py:9-30: the product names a sample folder may hold as files; everything else is a feature to extract
S2_BANDS = ["B1", "B2", "B3", "B4", "B5", "B6", "B7", "B8", "B8A", "B9", "B10", "B11", "B12"]
S2A_BANDS = [f"TOA_S2A_{b}" for b in S2_BANDS]
S2B_BANDS = [f"TOA_S2B_{b}" for b in S2_BANDS]
# band centres of AVIRIS-NG (nm, rounded): 425 bands
AVIRIS_WAVELENGTHS = [
    376, 381, 386, 391, 396, 401, 406, 412, 417, 422, 427, 432, 437, 442, 447, 452, 457, 462, 467, 472, 477, 482, 487, 492, 497,
    502, 507, 512, 517, 522, 527, 532, 537, 542, 547, 552, 557, 562, 567, 572, 577, 582, 587, 592, 597, 602, 607, 612, 617, 622,
    627, 632, 637, 642, 647, 652, 657, 662, 667, 672, 677, 682, 687, 692, 697, 702, 707, 712, 717, 722, 727, 732, 737, 742, 747,
    752, 757, 762, 767, 772, 777, 782, 787, 792, 797, 802, 807, 812, 817, 822, 827, 832, 837, 842, 847, 852, 857, 862, 867, 872,
    877, 882, 887, 892, 897, 902, 907, 912, 917, 922, 927, 932, 937, 942, 947, 952, 957, 962, 967, 972, 977, 982, 988, 993, 998,
    1003, 1008, 1013, 1018, 1023, 1028, 1033, 1038, 1043, 1048, 1053, 1058, 1063, 1068, 1073, 1078, 1083, 1088, 1093, 1098,
    1103, 1108, 1113, 1118, 1123, 1128, 1133, 1138, 1143, 1148, 1153, 1158, 1163, 1168, 1173, 1178, 1183, 1188, 1193, 1198,
    1203, 1208, 1213, 1218, 1223, 1228, 1233, 1238, 1243, 1248, 1253, 1258, 1263, 1268, 1273, 1278, 1283, 1288, 1293, 1298,
    1303, 1308, 1313, 1318, 1323, 1328, 1333, 1338, 1343, 1348, 1353, 1358, 1363, 1368, 1373, 1378, 1383, 1388, 1393, 1398,
    1403, 1408, 1413, 1418, 1423, 1428, 1433, 1438, 1443, 1448, 1453, 1458, 1463, 1468, 1473, 1478, 1483, 1488, 1493, 1498,
    1503, 1508, 1513, 1518, 1523, 1528, 1533, 1538, 1543, 1548, 1553, 1558, 1563, 1568, 1574, 1579, 1584, 1589, 1594, 1599,
    1604, 1609, 1614, 1619, 1624, 1629, 1634, 1639, 1644, 1649, 1654, 1659, 1664, 1669, 1674, 1679, 1684, 1689, 1694, 1699,
    1704, 1709, 1714, 1719, 1724, 1729, 1734, 1739, 1744, 1749, 1754, 1759, 1764, 1769, 1774, 1779, 1784, 1789, 1794, 1799,
    1804, 1809, 1814, 1819, 1824, 1829, 1834, 1839, 1844, 1849, 1854, 1859, 1864, 1869, 1874, 1879, 1884, 1889, 1894, 1899,
    1904, 1909, 1914, 1919, 1924, 1929, 1934, 1939, 1944, 1949, 1954, 1959, 1964, 1969, 1974, 1979, 1984, 1989, 1994, 1999,
    2004, 2009, 2014, 2019, 2024, 2029, 2034, 2039, 2044, 2049, 2054, 2059, 2064, 2069, 2074, 2079, 2084, 2089, 2094, 2099,
    2104, 2109, 2114, 2119, 2124, 2129, 2134, 2139, 2144, 2150, 2155, 2160, 2165, 2170, 2175, 2180, 2185, 2190, 2195, 2200,
    2205, 2210, 2215, 2220, 2225, 2230, 2235, 2240, 2245, 2250, 2255, 2260, 2265, 2270, 2275, 2280, 2285, 2290, 2295, 2300,
    2305, 2310, 2315, 2320, 2325, 2330, 2335, 2340, 2345, 2350, 2355, 2360, 2365, 2370, 2375, 2380, 2385, 2390, 2395, 2400,
    2405, 2410, 2415, 2420, 2425, 2430, 2435, 2440, 2445, 2450, 2455, 2460, 2465, 2470, 2475, 2480, 2485, 2490, 2495, 2500
]


def raw_bands_available():
    bands = [f"TOA_AVIRIS_{wv}nm" for wv in AVIRIS_WAVELENGTHS + [550, 640, 460]]
    bands.extend(WV3_BANDS)
    bands.extend(S2A_BANDS + S2B_BANDS)
    bands.extend(["mag1c", "labelbinary", "label_rgba"])
    return bands


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
