"""WorldView-3 and Sentinel-2 bands simulated from AVIRIS-NG radiance on the GPU.

Mirrors the reference's starcop/data/aviris.py:155-331 (load_srf_s2, load_srf_wv3, transform_to_worldview_3,
transform_to_sentinel_2, transform_to_srf): each simulated band is the spectral response function (SRF) of the sensor band
resampled to the nearest AVIRIS band, normalised to sum one, applied as a float64 weighted sum over those AVIRIS bands.
The weights are built on the host (:func:`srf_weights`, the reference's pandas arithmetic); the sums run in libstarcop_hip.so
(include/starcop_hip.h: sc_srf_bands), all output bands in one pass over the cube.  With ``resolution_dst`` and ``resolution_src``
the bands are then blurred and resampled to the sensor's pixel size (:mod:`starcop_amd.resample`, sc_resize_aa), the reference's
``read.resize(..., anti_aliasing=True)``.  The file-to-file driver is ``pipeline.aviris_as_sensor``.
"""
import numpy as np
import pandas as pd
import torch

from . import _lib
from ._lib import check, ptr, stream

SRF_S2 = None
SRF_WV3 = None

BANDS_S2_RESOLUTION = {"B1": 60, "B2": 10, "B3": 10, "B4": 10, "B5": 20, "B6": 20, "B7": 20, "B8": 10, "B8A": 20, "B9": 60,
                       "B10": 60, "B11": 20, "B12": 20}

SRF_WV3_FILE = "gs://starcop/WV3/WV3-SRF.csv"
SRF_S2_FILE = "gs://starcop/S2/S2-SRF_joint.csv"

NOUT_MAX = 64                      # output bands per sc_srf_bands call

# aviris.py:31-49: band-averaged solar irradiance in W / m^2 / nm (Sentinel-2: the SOLAR_IRRADIANCE metadata of the L1C products
# divided by 1000; WorldView-3: the published SWIR band values, kept as the quotients the reference evaluates)
SOLAR_IRRADIANCE_S2B = {"B01": 1.8743, "B02": 1.95977, "B03": 1.82493, "B04": 1.51279, "B05": 1.42578, "B06": 1.29113, "B07": 1.17557,
                        "B08": 1.04128, "B8A": 0.95393, "B09": 0.81758, "B10": 0.36541, "B11": 0.24708, "B12": 0.08775}
SOLAR_IRRADIANCE_S2A = {"B01": 1.88469, "B02": 1.95972, "B03": 1.82324, "B04": 1.51206, "B05": 1.42464, "B06": 1.28761, "B07": 1.16208,
                        "B08": 1.04163, "B8A": 0.95532, "B09": 0.81292, "B10": 0.36715, "B11": 0.24559, "B12": 0.08525}
SOLAR_IRRADIANCE_WV3 = {f"SWIR{i + 1}": v / 1000 for i, v in enumerate((477.8728, 263.2926, 224.9720, 197.3366, 90.3976, 85.0757,
                                                                         76.9260, 68.0897))}
SOLAR_IRRADIANCE = {"S2A": SOLAR_IRRADIANCE_S2A, "S2B": SOLAR_IRRADIANCE_S2B, "WV3": SOLAR_IRRADIANCE_WV3}


def earth_sun_distance_correction_factor(date_of_acquisition):
    """aviris.py:53-72: ``1 - 0.01673 cos(0.0172 (t - 4))`` with t the day of the year (1 on January 1st); 0.01673 is the
    eccentricity of the Earth's orbit, 0.0172 = 2 pi / 365.256363."""
    tm_yday = date_of_acquisition.timetuple().tm_yday
    return 1 - 0.01673 * np.cos(0.0172 * (tm_yday - 4))


def observation_date_correction_factor(date_of_acquisition, solar_altitude):
    """aviris.py:75-107 with the solar altitude (degrees above the horizon at the centre of the flight line, what
    ``pysolar.solar.get_altitude`` returns there) as an INPUT: ``pi d^2 / cos(sza pi / 180)``, ``sza = 90 - solar_altitude``,
    ``d`` = :func:`earth_sun_distance_correction_factor`, evaluated in float64 in the reference's order.  pysolar is not a
    dependency of this package and no ephemeris of its own is offered in its place."""
    sza = 90 - float(solar_altitude)
    d = earth_sun_distance_correction_factor(date_of_acquisition)
    return np.pi * (d ** 2) / np.cos(sza / 180. * np.pi)


def _read_srf(path):
    """CSV indexed by SR_WL without the rows where no band is above 1e-6 (aviris.py:178-185, 206-213)"""
    if str(path).startswith("gs://"):
        raise NotImplementedError(f"{path}: reading from Google Cloud Storage is not supported; pass a local copy with "
                                  "path_override (with cache=True it is then used by the transform_to_* functions)")
    srf = pd.read_csv(path).set_index("SR_WL")
    return srf.loc[np.any((srf > 1e-6).values, axis=1)]


def load_srf_s2(cache=True, path_override=None, drop_by_minimum=False):
    """Sentinel-2 SRF table (columns S2A_SR_AV_B1.. / S2B_SR_AV_B1..).  ``drop_by_minimum``: also drop the rows
    411 .. drop_by_minimum - 1 nm, as the reference does."""
    global SRF_S2
    if cache and SRF_S2 is not None:
        return SRF_S2
    srf = _read_srf(SRF_S2_FILE if path_override is None else path_override)
    if drop_by_minimum:
        srf = srf.drop(list(range(411, drop_by_minimum)))
    if cache:
        SRF_S2 = srf
    return srf


def load_srf_wv3(cache=True, path_override=None):
    """WorldView-3 SWIR SRF table (columns SWIR1..SWIR8)"""
    global SRF_WV3
    if cache and SRF_WV3 is not None:
        return SRF_WV3
    srf = _read_srf(SRF_WV3_FILE if path_override is None else path_override)
    if cache:
        SRF_WV3 = srf
    return srf


def nearest_band(bands_nanometers, wavelengths):
    """index of the nearest AVIRIS band of every wavelength: scipy's interp1d(centres, arange, kind="nearest") -- midpoints
    computed as c[i] / 2 + c[i + 1] / 2, a wavelength exactly on one goes to the lower band, one outside [min, max] of the
    centres raises ValueError"""
    c = np.asarray(bands_nanometers, dtype=np.float64)
    order = np.argsort(c, kind="mergesort")
    cs = c[order]
    q = np.asarray(wavelengths, dtype=np.float64)
    if np.any(q < cs[0]) or np.any(q > cs[-1]):
        raise ValueError(f"SRF wavelengths outside the AVIRIS band range [{cs[0]}, {cs[-1]}] nm")
    half = cs / 2.0
    idx = np.searchsorted(half[1:] + half[:-1], q, side="left").clip(0, len(cs) - 1)
    return order[idx]


def srf_weights(bands, srf, bands_nanometers):
    """Host CSR of the AVIRIS weights of each output band (aviris.py:288-312): rows of ``srf[band]`` above 1e-4, normalised by
    their sum, summed per nearest AVIRIS band (pandas' group sum) in ascending band order.
    -> (ptr int32 [len(bands) + 1], band int32 [nnz], w float64 [nnz])"""
    nearest = nearest_band(bands_nanometers, srf.index)
    ptrs, idx, wts = [0], [], []
    for name in bands:
        col = srf[name]
        keep = ~(col <= 1e-4).values
        kept = col[keep]
        per_band = (kept / kept.sum()).groupby(nearest[keep]).sum()
        idx.append(per_band.index.values.astype(np.int32))
        wts.append(per_band.values.astype(np.float64))
        ptrs.append(ptrs[-1] + len(per_band))
    return (np.asarray(ptrs, dtype=np.int32), np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32),
            np.concatenate(wts) if wts else np.zeros(0, np.float64))


class SrfPlan:
    """Host CSR uploaded once, split into calls of at most 64 output bands; ``run`` computes them for one cube."""

    def __init__(self, ptrs, band, w, device="cuda"):
        ptrs = np.asarray(ptrs, dtype=np.int64)
        self.n_out = len(ptrs) - 1
        self.parts = []
        for j0 in range(0, self.n_out, NOUT_MAX):
            j1 = min(j0 + NOUT_MAX, self.n_out)
            k0, k1 = int(ptrs[j0]), int(ptrs[j1])
            p = np.ascontiguousarray(ptrs[j0:j1 + 1] - k0, dtype=np.int32)
            b = np.ascontiguousarray(band[k0:k1], dtype=np.int32)
            if b.size == 0:
                b = np.zeros(1, np.int32)        # every row empty: the call raises on the empty row, not on a null pointer
            wk = np.ascontiguousarray(w[k0:k1], dtype=np.float64)
            dev = [torch.from_numpy(a.copy() if a.size else np.zeros(1, a.dtype)).to(device) for a in (p, b, wk)]
            self.parts.append((j0, j1, p, b, dev))

    def run(self, x, out, fill=None):
        """x: device float32 (L, S, B) view with any non-negative strides; out: device float32 (n_out, L, S) view with dense
        samples (its plane and line strides are passed on)"""
        lib = _lib.load()
        _lib.require_device(x)
        _lib.require_device(out)
        if x.dtype != torch.float32 or out.dtype != torch.float32:
            raise ValueError("sc_srf_bands: float32 cube and output expected")
        if x.dim() != 3 or out.dim() != 3 or tuple(out.shape) != (self.n_out,) + tuple(x.shape[:2]):
            raise ValueError(f"sc_srf_bands: cube {tuple(x.shape)} and output {tuple(out.shape)} do not match {self.n_out} bands")
        if out.shape[2] > 1 and out.stride(2) != 1:
            raise ValueError("sc_srf_bands: output samples must be dense")
        L, S, B = x.shape
        for j0, j1, p, b, (pd_, bd, wd) in self.parts:
            a = _lib.sc_srf_args()
            a.x = x.data_ptr()
            a.line_stride, a.sample_stride, a.band_stride = x.stride()
            a.L, a.S, a.B, a.n_out = L, S, B, j1 - j0
            a.ptr, a.band, a.w = pd_.data_ptr(), bd.data_ptr(), wd.data_ptr()
            a.ptr_host, a.band_host = p.ctypes.data, b.ctypes.data
            a.out = out[j0].data_ptr()
            a.out_plane_stride, a.out_line_stride = out.stride(0), out.stride(1)
            a.has_fill = int(fill is not None)
            a.fill = float(fill) if fill is not None else 0.0
            check(lib.sc_srf_bands(a, stream()))
        return out


def _resample_shape(who, shape, resolution_dst, resolution_src):
    """None when nothing is to be resampled, else the (oh, ow) of the resampled planes.  Host only: raises before any device use."""
    if resolution_dst is None:
        return None
    if resolution_src is None:
        raise NotImplementedError(f"{who}: a tensor carries no pixel size (the reference reads aviris.res); pass resolution_src to "
                                  "resample to resolution_dst, or resolution_dst=None for the AVIRIS grid")
    from . import resample
    out_shape = resample.output_shape_for(shape, resolution_src, resolution_dst)
    if out_shape == tuple(int(v) for v in shape[-2:]):
        return None
    if out_shape[0] > shape[-2] or out_shape[1] > shape[-1]:
        raise ValueError(f"{who}: resolution_dst {resolution_dst} is finer than resolution_src {resolution_src}; only downscaling is "
                         "supported")
    return out_shape


def transform_to_srf(aviris, bands, srf, resolution_dst=10, bands_nanometers_aviris=None, fill_value_default=0., sigma_bands=None,
                     verbose=False, resolution_src=None, mode="constant"):
    """aviris.py:262-338 on the GPU: ``aviris`` is a (C, H, W) float32 device tensor with any strides (``bip.permute(2, 0, 1)`` is
    read in place) or numpy array; returns the (len(bands), oh, ow) float32 simulated bands as a device tensor (numpy for numpy).
    Pixels holding ``fill_value_default`` in any band of a support become ``fill_value_default`` (None: nothing is masked).
    ``bands_nanometers_aviris`` (the C band centres) is required.  ``resolution_dst=None`` keeps the AVIRIS grid.  Otherwise
    ``resolution_src`` (the pixel size of ``aviris``, a number or (y, x); a tensor carries no ``res``) is required and the spectral
    result is resampled as the reference's ``read.resize(..., anti_aliasing=True, anti_aliasing_sigma=sigma_bands)`` does
    (:func:`starcop_amd.resample.resize_antialiased`): a Gaussian of ``sigma_bands`` pixels per band (None: (scale - 1) / 2), then a
    bilinear resample to ``round(n * resolution_src / resolution_dst)`` pixels per axis, border ``mode`` with ``cval =
    fill_value_default`` (0 for None).  Fill pixels are not masked there: the reference blurs them into their neighbours too.  Equal
    input and output shapes return the spectral result."""
    out_shape = _resample_shape("transform_to_srf", aviris.shape, resolution_dst, resolution_src)
    if bands_nanometers_aviris is None:
        raise ValueError("transform_to_srf: bands_nanometers_aviris is required (a tensor carries no band descriptions)")
    if out_shape is not None:
        from . import resample
        if mode not in resample.MODES:
            raise ValueError(f"transform_to_srf: border mode '{mode}', expected one of {resample.MODES}")
        if sigma_bands is not None:
            sigma_bands = np.asarray(sigma_bands, dtype=np.float64)
            if sigma_bands.shape != (len(bands),) or not np.all(sigma_bands >= 0):
                raise ValueError(f"transform_to_srf: sigma_bands must hold one non-negative sigma per band, got {sigma_bands}")
    host = isinstance(aviris, np.ndarray)
    x = aviris
    if host:
        a = aviris if all(s >= 0 for s in aviris.strides) else np.ascontiguousarray(aviris)
        _lib.require_device()
        x = torch.from_numpy(a).cuda()
    if x.dim() != 3 or x.shape[0] != len(bands_nanometers_aviris):
        raise ValueError(f"transform_to_srf: expected a (C, H, W) cube with C = {len(bands_nanometers_aviris)} bands, "
                         f"got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"transform_to_srf: float32 radiance expected, got {x.dtype}")
    _lib.require_device(x)
    ptrs, band, w = srf_weights(list(bands), srf, bands_nanometers_aviris)
    if verbose:
        print(f"transform_to_srf: {len(bands)} bands from {len(band)} AVIRIS band weights")
    out = torch.empty((len(bands),) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    SrfPlan(ptrs, band, w, x.device).run(x.permute(1, 2, 0), out, fill_value_default)
    if out_shape is not None:
        out = resample.resize_antialiased(out, out_shape, sigma=sigma_bands, mode=mode,
                                          cval=0.0 if fill_value_default is None else fill_value_default)
    return out.cpu().numpy() if host else out


def transform_to_worldview_3(aviris, bands_wv3, resolution_dst=10, bands_nanometers_aviris=None, fill_value_default=0., verbose=False,
                             resolution_src=None):
    """aviris.py:224-234: the WV3 SWIR bands ``bands_wv3`` (e.g. ["SWIR1", ...]) with the cached SRF (load_srf_wv3); resampled with
    the default anti-aliasing sigma, as the reference does (sigma_bands=None)"""
    _resample_shape("transform_to_worldview_3", aviris.shape, resolution_dst, resolution_src)
    return transform_to_srf(aviris, bands_wv3, load_srf_wv3(), resolution_dst=resolution_dst,
                            bands_nanometers_aviris=bands_nanometers_aviris, fill_value_default=fill_value_default, verbose=verbose,
                            resolution_src=resolution_src)


def sentinel_2_srf(sensor="S2A"):
    """the columns of the joint S2 table that belong to ``sensor``, renamed from f"{sensor}_SR_AV_B1" to "B1" (aviris.py:244-245)"""
    srf_s2 = load_srf_s2()
    srf = srf_s2[[c for c in srf_s2.columns if sensor in c]].copy()
    srf.columns = [c.replace(f"{sensor}_SR_AV_", "") for c in srf.columns]
    return srf


def sentinel_2_sigmas(bands_s2, resolution_src):
    """aviris.py:248-254: the anti-aliasing sigma of every band, ``max((band GSD / max(resolution_src) - 1) / 2, 0)`` AVIRIS pixels"""
    res = max(abs(float(v)) for v in np.atleast_1d(resolution_src))
    return np.array([max((BANDS_S2_RESOLUTION[b] / res - 1) / 2, 0) for b in bands_s2])


def transform_to_sentinel_2(aviris, bands_s2, resolution_dst=10, sensor="S2A", bands_nanometers_aviris=None, fill_value_default=0.,
                            verbose=False, resolution_src=None):
    """aviris.py:237-259: the S2A or S2B bands ``bands_s2`` (e.g. ["B8A", "B11"]) with the cached joint SRF (load_srf_s2); each band is
    blurred with the sigma of its own ground sampling distance (:func:`sentinel_2_sigmas`) before the resample to ``resolution_dst``"""
    _resample_shape("transform_to_sentinel_2", aviris.shape, resolution_dst, resolution_src)
    sigma_bands = sentinel_2_sigmas(bands_s2, resolution_src) if resolution_dst is not None else None
    return transform_to_srf(aviris, bands_s2, sentinel_2_srf(sensor), resolution_dst=resolution_dst,
                            bands_nanometers_aviris=bands_nanometers_aviris, fill_value_default=fill_value_default, verbose=verbose,
                            sigma_bands=sigma_bands, resolution_src=resolution_src)
