"""Plume quantification on the host: from the radial profiles of ``plumes.component_radial`` to shape and emission rates.

numpy only, float64 throughout, no device.  The integrated mass enhancement (IME) methods follow Duren et al. 2019 (the AVIRIS-NG
California survey): with the enhancement above background integrated over the plume pixels within distance r of the source,
``IME(r)`` in kg, and an effective wind speed U in m/s, the emission rate is ``Q = U * IME(r) / r``, averaged over circles of growing
radius; the simpler single-number form takes the whole plume and ``sqrt(area)`` as its length (Varon et al. 2018).

The wind speed is used AS GIVEN, as the effective wind speed of the method.  Models that turn a 10 m wind (U10) into an
effective wind are fitted per instrument and pixel size and are not built in; neither is any source of wind data."""
import math

import numpy as np

M_CH4_KG_PER_MOL = 0.01604246
R_GAS_J_PER_MOL_K = 8.314462618
DEFAULT_MAX_FETCH_M = 150.0        # the AVIRIS-NG survey's largest circle
MAX_RADII = 64                     # bin edges of one sc_component_radial call

QUANTIFY_KEYS = ("wind_speed_m_s", "radii_m", "max_fetch_m", "origin", "origin_xy", "min_fetch_m", "temperature_k", "pressure_pa",
                 "kg_per_ppmm_m2")
QUANTIFY_COLUMNS = ("origin_row", "origin_col", "fetch_max_m", "major_axis_m", "minor_axis_m", "orientation_rad", "ime_kg",
                    "q_sqrt_area_kg_h", "q_fetch_kg_h", "q_fetch_std_kg_h", "q_fetch_n")


def kg_per_ppmm_m2(temperature_k=288.15, pressure_pa=101325.0):
    """Mass of methane, in kg, in a column of 1 ppm m over 1 m2 of ground at the given temperature and pressure:
    ``1e-6 * 0.01604246 * p / (8.314462618 * T)`` -- 1 ppm m is a layer of 1e-6 m of pure methane, an ideal gas has p / (R T) mol
    per m3 and methane weighs 0.01604246 kg per mol.  6.785e-7 kg at the defaults (15 C, 1 atm)."""
    t, p = float(temperature_k), float(pressure_pa)
    if not t > 0.0 or not p > 0.0 or not math.isfinite(t) or not math.isfinite(p):
        raise ValueError(f"kg_per_ppmm_m2: temperature_k {temperature_k!r} and pressure_pa {pressure_pa!r} must be positive and finite")
    return 1e-6 * M_CH4_KG_PER_MOL * p / (R_GAS_J_PER_MOL_K * t)


def _ints(a):
    """an array of Python integers (object dtype): products of 62-bit sums do not fit int64"""
    return np.array([int(v) for v in np.asarray(a).reshape(-1)], dtype=object)


def shape_from_moments(area, sum_row, sum_col, sum_rr, sum_cc, sum_rc):
    """Axes and orientation of the ellipse with the second moments of a component's pixel centres, from the integer sums
    ``sc_component_stats`` / ``sc_component_radial`` return (arrays of one length) -> ``(major_axis_px, minor_axis_px,
    orientation_rad)``, float64.

    With A = area, the central second moments are ``mu_rr = (A * sum_rr - sum_row^2) / A^2``, ``mu_cc = (A * sum_cc - sum_col^2) /
    A^2`` and ``mu_rc = (A * sum_rc - sum_row * sum_col) / A^2``: the numerators are evaluated exactly in Python integers, each
    is converted to float64 once and divided once by A^2.  The eigenvalues of [[mu_rr, mu_rc], [mu_rc, mu_cc]] are
    ``l = (mu_rr + mu_cc) / 2 +- hypot((mu_rr - mu_cc) / 2, mu_rc)`` (the smaller one not below 0), the axes ``4 * sqrt(l)``: the
    full axes of the ellipse with these moments, as scikit-image's ``regionprops`` reports them.  Pixels count as points, so a 1 x n
    line has the major axis ``4 * sqrt((n^2 - 1) / 12)`` and the minor axis 0, and a single pixel has both 0.

    ``orientation_rad = atan2(2 mu_rc, mu_rr - mu_cc) / 2`` is the angle of the major axis from the row axis, positive towards
    increasing columns, in (-pi/2, pi/2].  Rules for the ties: a component along the column axis (mu_rc = 0, mu_cc > mu_rr) has
    +pi/2, never -pi/2; with mu_rr = mu_cc the sign of mu_rc decides between +pi/4 and -pi/4; an isotropic component (mu_rc = 0
    and mu_rr = mu_cc: a single pixel, a square, a disc) has 0.  A row with area 0 has NaN in all three."""
    A, sr, sc, srr, scc, src = (_ints(v) for v in (area, sum_row, sum_col, sum_rr, sum_cc, sum_rc))
    n = len(A)
    major, minor, orient = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        a = A[i]
        if a <= 0:
            continue
        a2 = float(a * a)
        mu_rr = float(a * srr[i] - sr[i] * sr[i]) / a2
        mu_cc = float(a * scc[i] - sc[i] * sc[i]) / a2
        mu_rc = float(a * src[i] - sr[i] * sc[i]) / a2
        half, diff = (mu_rr + mu_cc) / 2.0, (mu_rr - mu_cc) / 2.0
        root = math.hypot(diff, mu_rc)
        major[i] = 4.0 * math.sqrt(max(half + root, 0.0))
        minor[i] = 4.0 * math.sqrt(max(half - root, 0.0))
        orient[i] = 0.0 if root == 0.0 else math.atan2(2.0 * mu_rc, mu_rr - mu_cc) / 2.0
    return major, minor, orient


def fetch_profile(bin_count, bin_sum, bg_mean=None):
    """The cumulative profile of ``component_radial``'s bins: ``bin_count`` / ``bin_sum`` of shape (..., K+1), the last bin the
    overflow beyond the last edge -> ``{"n": n_j, "sum": S_j, "sum_bgsub": S_j - bg_mean * n_j or None}``, each (..., K) float64:
    pixel count and sum over the bins 0..j, i.e. over the finite pixels with d2 <= edge2[j] (``numpy.cumsum`` along the last axis;
    the overflow bin is left out).  ``bg_mean``: the background per row (shape (...,)), NaN where there is none."""
    cnt = np.asarray(bin_count)
    s = np.asarray(bin_sum, dtype=np.float64)
    if cnt.shape != s.shape or cnt.ndim < 1 or cnt.shape[-1] < 2:
        raise ValueError(f"fetch_profile: bin_count {cnt.shape} and bin_sum {s.shape} must share a shape (..., K+1), K >= 1")
    n = np.cumsum(cnt[..., :-1].astype(np.float64), axis=-1)
    S = np.cumsum(s[..., :-1], axis=-1)
    sub = None
    if bg_mean is not None:
        bg = np.asarray(bg_mean, dtype=np.float64)
        if bg.shape != cnt.shape[:-1]:
            raise ValueError(f"fetch_profile: bg_mean {bg.shape} for rows {cnt.shape[:-1]}")
        sub = S - bg[..., None] * n
    return {"n": n, "sum": S, "sum_bgsub": sub}


def emission_rates(ime_profile_kg, radii_m, fetch_max_m, area_m2, ime_kg, wind_speed_m_s, min_fetch_m=0.0):
    """Emission rates per plume, in kg/h.  ``ime_profile_kg`` (R, K): IME_j, the mass inside the circle of radius ``radii_m[j]``
    (K increasing radii in m); ``fetch_max_m`` (R,): the distance of the plume's farthest pixel from its origin; ``area_m2``,
    ``ime_kg`` (R,): area and mass of the whole plume; ``wind_speed_m_s``: U, a scalar or (R,), used as given as the effective wind
    speed (no U10 model is applied).  -> a dict of (R,) arrays:

    ``q_sqrt_area_kg_h = 3600 * U * ime_kg / sqrt(area_m2)``;
    ``q_fetch_kg_h``, the mean of ``q_j = 3600 * U * IME_j / r_j`` over the USED radii, ``q_fetch_std_kg_h`` their population
    standard deviation (``sqrt(mean((q_j - mean)^2))``) and ``q_fetch_n`` their number (int64); and ``q_kg_h`` (R, K), every q_j,
    with ``used`` (R, K) bool.
    Radius j is used when ``r_j >= min_fetch_m`` and no smaller radius holds the whole plume already: j = 0, or
    ``r_{j-1} < fetch_max_m`` -- the circles grow up to and including the first that contains the plume, beyond it IME stays and
    IME / r only falls.  A row whose ``fetch_max_m`` is not finite (no pixels, no origin) uses none.  ``q_fetch_n == 0`` gives NaN
    for the mean and the deviation; a NaN in a used IME_j (no background) makes them NaN too."""
    prof = np.asarray(ime_profile_kg, dtype=np.float64)
    r = np.asarray(radii_m, dtype=np.float64).reshape(-1)
    if prof.ndim != 2 or prof.shape[1] != r.size or r.size < 1:
        raise ValueError(f"emission_rates: profile {prof.shape} for {r.size} radii (expected (rows, K))")
    if not np.all(np.isfinite(r)) or not np.all(r > 0.0) or not np.all(np.diff(r) > 0.0):
        raise ValueError("emission_rates: radii_m must be positive, finite and strictly increasing")
    R = prof.shape[0]
    fmax, area, ime = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (fetch_max_m, area_m2, ime_kg))
    U = np.asarray(wind_speed_m_s, dtype=np.float64)
    U = np.full(R, float(U)) if U.ndim == 0 else U.reshape(-1)
    for name, v in (("fetch_max_m", fmax), ("area_m2", area), ("ime_kg", ime), ("wind_speed_m_s", U)):
        if v.size != R:
            raise ValueError(f"emission_rates: {name} has {v.size} values for {R} rows")
    prev = np.concatenate([[-np.inf], r[:-1]])
    used = (r[None, :] >= float(min_fetch_m)) & (prev[None, :] < fmax[:, None]) & np.isfinite(fmax)[:, None]
    q = 3600.0 * U[:, None] * prof / r[None, :]
    n = used.sum(axis=1).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = np.maximum(n, 1).astype(np.float64)
        mean = np.where(n > 0, np.where(used, q, 0.0).sum(axis=1) / nn, np.nan)
        dev = np.where(used, q - mean[:, None], 0.0)
        std = np.where(n > 0, np.sqrt((dev * dev).sum(axis=1) / nn), np.nan)
        q_area = 3600.0 * U * ime / np.sqrt(area)
    return {"q_sqrt_area_kg_h": q_area, "q_fetch_kg_h": mean, "q_fetch_std_kg_h": std, "q_fetch_n": n, "q_kg_h": q, "used": used}


def check_quantify(quantify, who):
    """the ``quantify=`` dict of ``plumes.plume_table`` (``plume_quantify=`` of the scene calls): None, or a dict with
    ``wind_speed_m_s`` and keys from ``QUANTIFY_KEYS``; what can be said without the grid is checked here (no device involved)"""
    if quantify is None:
        return None
    if not isinstance(quantify, dict) or set(quantify) - set(QUANTIFY_KEYS) or "wind_speed_m_s" not in quantify:
        raise ValueError(f"{who}: quantify must be a dict with wind_speed_m_s and keys from {QUANTIFY_KEYS}, got {quantify!r}")
    if "radii_m" in quantify and "max_fetch_m" in quantify:
        raise ValueError(f"{who}: quantify takes radii_m or max_fetch_m, not both")
    U = np.asarray(quantify["wind_speed_m_s"], dtype=np.float64)
    if U.ndim > 1 or U.size == 0 or not np.all(np.isfinite(U)) or not np.all(U >= 0.0):
        raise ValueError(f"{who}: wind_speed_m_s must be a finite number >= 0, or one per plume")
    origin = quantify.get("origin", "max")
    if isinstance(origin, str):
        if origin != "max":
            raise ValueError(f"{who}: origin {origin!r}: \"max\" or an (R, 2) array")
        if quantify.get("origin_xy"):
            raise ValueError(f"{who}: origin_xy=True needs an (R, 2) array of (x, y) as origin")
    else:
        o = np.asarray(origin)
        if o.ndim != 2 or o.shape[1] != 2 or o.dtype.kind not in "iuf":
            raise ValueError(f"{who}: origin must be \"max\" or an (R, 2) array, got shape {o.shape}")
    if not float(quantify.get("min_fetch_m", 0.0)) >= 0.0:
        raise ValueError(f"{who}: min_fetch_m {quantify['min_fetch_m']!r} must be >= 0")
    if "kg_per_ppmm_m2" in quantify:
        if "temperature_k" in quantify or "pressure_pa" in quantify:
            raise ValueError(f"{who}: kg_per_ppmm_m2 replaces temperature_k / pressure_pa; pass one or the other")
        k = float(quantify["kg_per_ppmm_m2"])
        if not k > 0.0 or not math.isfinite(k):
            raise ValueError(f"{who}: kg_per_ppmm_m2 {quantify['kg_per_ppmm_m2']!r} must be positive and finite")
    else:
        kg_per_ppmm_m2(quantify.get("temperature_k", 288.15), quantify.get("pressure_pa", 101325.0))
    return quantify


def radii_for(quantify, pixel_size_m):
    """(radii_m, radii_px) of a checked ``quantify`` dict on a grid of square pixels of ``pixel_size_m``: ``radii_m`` as given
    (radii_px = radii_m / pixel_size_m), else ``r_j = j * pixel_size_m`` for j = 1 .. min(64, floor(max_fetch_m / pixel_size_m))
    with ``max_fetch_m`` = 150 m by default (radii_px = j, exactly).  ValueError for no radius at all, more than 64, radii that
    are not positive and increasing, or two radii whose ``floor(radius_px^2)`` coincide."""
    px = float(pixel_size_m)
    if "radii_m" in quantify:
        radii_m = np.asarray(quantify["radii_m"], dtype=np.float64).reshape(-1)
        radii_px = radii_m / px
    else:
        fetch = float(quantify.get("max_fetch_m", DEFAULT_MAX_FETCH_M))
        if not fetch > 0.0 or not math.isfinite(fetch):
            raise ValueError(f"quantify: max_fetch_m {fetch!r} must be positive and finite")
        radii_px = np.arange(1, min(MAX_RADII, int(math.floor(fetch / px))) + 1, dtype=np.float64)
        radii_m = radii_px * px
    if radii_m.size == 0:
        raise ValueError(f"quantify: no radius at all (max_fetch_m below the pixel size {px} m, or an empty radii_m)")
    if radii_m.size > MAX_RADII:
        raise ValueError(f"quantify: {radii_m.size} radii, at most {MAX_RADII}")
    if not np.all(np.isfinite(radii_m)) or not np.all(radii_m > 0.0) or not np.all(np.diff(radii_m) > 0.0):
        raise ValueError("quantify: radii_m must be positive, finite and strictly increasing")
    return radii_m, radii_px


def squared_edges(radii_px, who, limit):
    """``edge2[j] = floor(radii_px[j]^2)`` in float64, no epsilon (the convention of ``morphology.dilate`` and
    ``plumes.background_rings``) -> a list of ints; ValueError unless there are 1 to 64 positive finite radii whose edges increase
    strictly and stay below ``limit``"""
    r = np.asarray(radii_px, dtype=np.float64).reshape(-1)
    if not 1 <= r.size <= MAX_RADII:
        raise ValueError(f"{who}: {r.size} radii (1 to {MAX_RADII})")
    if not np.all(np.isfinite(r)) or not np.all(r > 0.0):
        raise ValueError(f"{who}: radii must be positive and finite")
    e = np.floor(r * r)
    if not np.all(np.diff(e) > 0.0):
        raise ValueError(f"{who}: floor(radius^2) must increase strictly, got {[int(v) for v in e]}")
    if not e[-1] < limit:
        raise ValueError(f"{who}: radius {r[-1]} too large: floor(radius^2) must stay below {limit}")
    return [int(v) for v in e]


def quantify_columns(quantify, radii_m, pixel_size_m, area_px, sum_row, sum_col, mag1c_sum, n_finite, radial, bg_mean=None,
                     wind_rows=None):
    """The quantification columns of ``plumes.plume_table`` for R table rows, from host arrays: the ``component_stats`` columns of
    the rows (``area_px``, ``sum_row``, ``sum_col``, ``mag1c_sum``, ``n_finite``), ``radial`` = the ``component_radial`` columns of
    the same rows plus ``origin`` (R, 2), and with a background ring ``bg_mean``.  ``wind_rows``: U per row where the dict has one
    per plume.  -> (columns dict in ``QUANTIFY_COLUMNS`` order, curves dict for ``plumes.fetch_profiles``).

    ``pixel area a = pixel_size_m^2``, ``kg`` = ``kg_per_ppmm_m2``: ``ime_kg = (mag1c_sum - bg_mean * n_finite) * a * kg`` (without a
    ring the subtraction is left out), ``IME_j = (S_j - bg_mean * n_j) * a * kg`` from ``fetch_profile``, ``fetch_max_m =
    sqrt(d2_max) * pixel_size_m``, the axes of ``shape_from_moments`` times ``pixel_size_m``, the rates of ``emission_rates``."""
    px = float(pixel_size_m)
    a = px * px
    if "kg_per_ppmm_m2" in quantify:
        kg = float(quantify["kg_per_ppmm_m2"])
    else:
        kg = kg_per_ppmm_m2(quantify.get("temperature_k", 288.15), quantify.get("pressure_pa", 101325.0))
    area_px = np.asarray(area_px)
    R = area_px.size
    origin = np.asarray(radial["origin"], dtype=np.int64).reshape(R, 2)
    skipped = origin[:, 0] < 0
    d2 = np.asarray(radial["d2_max"], dtype=np.int64).reshape(R)
    with np.errstate(invalid="ignore"):
        fetch_max = np.where(d2 >= 0, np.sqrt(np.maximum(d2, 0).astype(np.float64)) * px, np.nan)
    major, minor, orient = shape_from_moments(area_px, sum_row, sum_col, np.where(skipped, 0, radial["sum_rr"]),
                                              np.where(skipped, 0, radial["sum_cc"]), np.where(skipped, 0, radial["sum_rc"]))
    major, minor, orient = (np.where(skipped, np.nan, v) for v in (major, minor, orient))
    prof = fetch_profile(np.asarray(radial["bin_count"]), np.asarray(radial["bin_sum"]), bg_mean)
    s = np.asarray(mag1c_sum, dtype=np.float64)
    if bg_mean is not None:
        s = s - np.asarray(bg_mean, dtype=np.float64) * np.asarray(n_finite).astype(np.float64)
    ime_kg = s * a * kg
    ime_prof = (prof["sum"] if bg_mean is None else prof["sum_bgsub"]) * a * kg
    U = quantify["wind_speed_m_s"] if wind_rows is None else wind_rows
    rates = emission_rates(ime_prof, radii_m, fetch_max, area_px.astype(np.float64) * a, ime_kg, U, float(quantify.get("min_fetch_m", 0.0)))
    cols = {"origin_row": np.where(skipped, -1, origin[:, 0]), "origin_col": np.where(skipped, -1, origin[:, 1]),
            "fetch_max_m": fetch_max, "major_axis_m": major * px, "minor_axis_m": minor * px, "orientation_rad": orient,
            "ime_kg": ime_kg}
    cols.update({c: rates[c] for c in ("q_sqrt_area_kg_h", "q_fetch_kg_h", "q_fetch_std_kg_h", "q_fetch_n")})
    curves = {"radii_m": np.asarray(radii_m, dtype=np.float64), "n_px": prof["n"], "ime_kg": ime_prof, "q_kg_h": rates["q_kg_h"],
              "used": rates["used"]}
    return cols, curves
