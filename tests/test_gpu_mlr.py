"""Sanchez-Garcia MLR ratio (sc_mlr_*) against the reference's own outputs (tests/golden/g12_mlr.npz, float32 and float64 runs of
starcop/data/feature_extration.py:58-125) and the float64 host oracle of tests/mlr_util.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlr_util import fit64, load_g12, ratio64, wv3_tile  # noqa: E402
from starcop_amd import features  # noqa: E402

DEV = "cuda"
DIVS = ("c_matched_outliers", "simple_plus", "residual")
TOL64 = {"c_matched_outliers": 2e-6, "residual": 2e-6, "simple_plus": 2e-5, "autoclip": 2e-6}


@pytest.fixture(scope="module")
def g():
    return load_g12()


def _run(bands, target, div):
    b = torch.from_numpy(np.ascontiguousarray(bands)).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(target)).to(DEV)
    if div == "autoclip":
        return features.ratio_MLR_local(b, t, autoclip=True).cpu().numpy()
    return features.ratio_MLR_local(b, t, division=div).cpu().numpy()


def test_against_reference_goldens(hip, g):
    for name in g["names"]:
        if name == "zero":
            continue
        bands, target = g[f"{name}_bands"], g[f"{name}_target"]
        for div in DIVS + ("autoclip",):
            got = _run(bands, target, div).astype(np.float64)
            f64, f32 = g[f"{name}_f64_{div}"], g[f"{name}_f32_{div}"].astype(np.float64)
            assert got.shape == f64.shape and np.isfinite(got).all()
            e64 = np.abs(got - f64).max()
            assert e64 <= TOL64[div], (name, div, e64)
            own = np.abs(f32 - f64).max()                   # the reference's float32 error on this tile
            assert np.abs(got - f32).max() <= max(1e-5, 1.5 * own), (name, div, np.abs(got - f32).max(), own)


def test_coefficients(hip, g):
    for name in ("wv3a", "wv3b", "k9", "const"):
        bands, target = g[f"{name}_bands"], g[f"{name}_target"]
        coef, icpt = features.mlr_fit(torch.from_numpy(bands).to(DEV), torch.from_numpy(target).to(DEV))
        assert coef.dtype == torch.float64 and coef.shape == (bands.shape[0],) and icpt.shape == ()
        c, i = coef.cpu().numpy(), float(icpt)
        want_c, want_i = g[f"{name}_f64_coef"], float(g[f"{name}_f64_intercept"])
        if name == "const":                                  # the constant band: coefficient exactly 0, the rest as sklearn
            assert c[2] == 0.0
            assert np.abs(c - want_c).max() < 1e-8 and abs(i - want_i) < 1e-8
        else:
            assert np.abs(c - want_c).max() <= 1e-9 * np.abs(want_c).max(), name
            assert abs(i - want_i) <= 1e-9 * max(1.0, abs(want_i)), name


def test_all_zero_tile(hip, g):
    b, t = g["zero_bands"], g["zero_target"]
    assert (_run(b, t, "c_matched_outliers") == np.float32(-0.5)).all()
    assert np.isnan(_run(b, t, "simple_plus")).all()
    assert (_run(b, t, "residual") == 0).all()
    coef, icpt = features.mlr_fit(torch.from_numpy(b).to(DEV), torch.from_numpy(t).to(DEV))
    assert (coef.cpu() == 0).all() and float(icpt) == 0.0


def _check_batch(bands, target, divs=DIVS, tol=None):
    """bands (B, k, H, W), target (B, H, W): every tile of one batched call against the float64 oracle (c_matched_outliers: with
    the prediction stored as float32, see mlr_util.ratio64)"""
    bd, td = torch.from_numpy(bands).to(DEV), torch.from_numpy(target).to(DEV)
    for div in divs:
        got = features.ratio_MLR_local(bd, td, division=div).cpu().numpy().astype(np.float64)
        assert got.shape == target.shape
        for b in range(target.shape[0]):
            e = np.abs(got[b] - ratio64(bands[b], target[b], div, r_f32=div == "c_matched_outliers")).max()
            assert e <= (tol or TOL64)[div], (div, b, target.shape, e)


def test_batch_512_of_16_and_ragged(hip):
    rng = np.random.default_rng(21)
    for B, H, W in ((16, 512, 512), (3, 257, 383)):
        tiles = [wv3_tile(rng, H, W) for _ in range(B)]
        _check_batch(np.stack([t[0] for t in tiles]), np.stack([t[1] for t in tiles]))


def test_k9_and_band_views_of_a_stacked_tensor(hip):
    """nine regressors; and the bands passed as views of one (B, 10, H, W) tensor (read in place through the band offsets,
    in an order that is not the storage order) give the same bits as a dense copy"""
    rng = np.random.default_rng(22)
    tiles = [wv3_tile(rng, 200, 136, k=9) for _ in range(4)]
    bands, target = np.stack([t[0] for t in tiles]), np.stack([t[1] for t in tiles])
    _check_batch(bands, target)
    stack = torch.from_numpy(np.concatenate([target[:, None], bands[:, ::-1]], 1).copy()).to(DEV)     # (B, 10, H, W)
    views = [stack[:, 9 - j] for j in range(9)]
    for div in DIVS:
        a = features.ratio_MLR_local(views, stack[:, 0], division=div)
        b = features.ratio_MLR_local(torch.from_numpy(bands).to(DEV), torch.from_numpy(target).to(DEV), division=div)
        assert torch.equal(a, b), div


def test_large_mean_over_std_pins_moment_precision(hip):
    """bands with mean/std ~ 1e3: the raw-moment fit must still match the float64 oracle"""
    rng = np.random.default_rng(23)
    bands, target = wv3_tile(rng, 256, 256, border=0, scale=1.0, offset=150.0)
    assert bands[0].mean() / bands[0].std() > 500
    coef, icpt = features.mlr_fit(torch.from_numpy(bands).to(DEV), torch.from_numpy(target).to(DEV))
    want_c, want_i = fit64(bands, target)
    assert np.abs(coef.cpu().numpy() - want_c).max() <= 1e-6 * np.abs(want_c).max()
    _check_batch(bands[None], target[None], divs=("residual", "c_matched_outliers"))


def test_bit_identical_repeats(hip):
    rng = np.random.default_rng(24)
    tiles = [wv3_tile(rng, 384, 320) for _ in range(5)]
    bd = torch.from_numpy(np.stack([t[0] for t in tiles])).to(DEV)
    td = torch.from_numpy(np.stack([t[1] for t in tiles])).to(DEV)
    for div in DIVS:
        a = features.ratio_MLR_local(bd, td, division=div)
        b = features.ratio_MLR_local(bd, td, division=div)
        assert torch.equal(a, b), div
    assert torch.equal(features.mlr_fit(bd, td)[0], features.mlr_fit(bd, td)[0])


def test_scene_sized_tile_and_wrappers(hip):
    """a whole scene as one tile (1280 x 1242: sc_trimmed_sums' large-tile path), through the reference's 5-input wrapper"""
    rng = np.random.default_rng(25)
    bands, target = wv3_tile(rng, 1280, 1242)
    bd = [torch.from_numpy(b).to(DEV) for b in bands]
    td = torch.from_numpy(target).to(DEV)
    for div in DIVS:
        fn = features.ratio_MLR_local_5IN_simplediv if div == "simple_plus" else features.ratio_MLR_local_5IN
        got = fn(*bd, td) if div != "residual" else fn(*bd, td, division="residual")
        e = np.abs(got.cpu().numpy().astype(np.float64) - ratio64(bands, target, div, r_f32=div == "c_matched_outliers")).max()
        assert e <= TOL64[div], (div, e)
