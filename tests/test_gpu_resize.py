"""sc_resize_aa (starcop_amd/resample.py: resize_antialiased) on the GPU against the operator's definition -- scipy's gaussian_filter +
zoom(order=1, grid_mode=True) in float64 -- and, bit for bit, against the numpy restatement of its rounding contract
(tests/resize_util.py).

Gate: |got - oracle64| <= 4 * 2^-24 * M everywhere, M = max(max|x|, |cval|).  The weights are non-negative and sum to one, so no
intermediate exceeds M and the two roundings to float32 are at most 2^-24 M each: the derived bound is 2 * 2^-24 M; the factor 2 over
it covers the summation order of the folded weights and nothing else.  Measured worst distance: profiles/resize_parity.txt."""
import numpy as np
import pytest
import torch

import resize_util as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", R.SHAPES, ids=lambda c: "{}x{}-{}x{}-s{}".format(*c[:5]))
def test_matches_the_oracle_and_the_restatement(hip, case):
    from starcop_amd import resample
    H, W, oh, ow, sigma, cval = case
    x = R.make_plane(H, W, seed=H * 1000 + W, cval=cval if cval else None)
    xd = torch.from_numpy(x).cuda()
    for mode in R.MODES:
        got = resample.resize_antialiased(xd, (oh, ow), sigma=sigma, mode=mode, cval=cval)
        assert tuple(got.shape) == (oh, ow) and got.dtype == torch.float32 and got.is_cuda
        got = got.cpu().numpy()
        want = R.oracle64(x, (oh, ow), sigma, mode, cval)
        print(f"resize {H}x{W}->{oh}x{ow} sigma {sigma} cval {cval} {mode}: {R.ulps(got, want, x, cval):.3f} x 2^-24 M")
        assert np.abs(got.astype(np.float64) - want).max() <= R.gate(x, cval), mode
        assert np.array_equal(_bits(got), _bits(R.restatement(x, (oh, ow), sigma, mode, cval))), mode


def test_batch_equals_single_planes_and_repeats(hip):
    """three planes with the sigmas of B2 / B11 / B1 at 5 m in one call == the three single-plane calls, in bits; a second call gives
    identical bits; numpy in gives numpy out"""
    from starcop_amd import resample
    x = np.stack([R.make_plane(70, 90, seed=s) for s in (1, 2, 3)])
    xd = torch.from_numpy(x).cuda()
    sig = [0.5, 1.5, 5.5]
    for mode in ("constant", "reflect"):
        got = resample.resize_antialiased(xd, (18, 23), sigma=sig, mode=mode, cval=-3.0)
        assert tuple(got.shape) == (3, 18, 23)
        again = resample.resize_antialiased(xd, (18, 23), sigma=sig, mode=mode, cval=-3.0)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        for p in range(3):
            one = resample.resize_antialiased(xd[p], (18, 23), sigma=sig[p], mode=mode, cval=-3.0)
            assert torch.equal(got[p].view(torch.int32), one.view(torch.int32)), (mode, p)
            assert np.array_equal(_bits(one.cpu().numpy()), _bits(R.restatement(x[p], (18, 23), sig[p], mode, -3.0))), (mode, p)
    host = resample.resize_antialiased(x, (18, 23), sigma=sig, mode="reflect", cval=-3.0)
    assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(got.cpu().numpy()))


def test_default_and_anisotropic_sigma(hip):
    from starcop_amd import resample
    x = R.make_plane(48, 40, seed=9)
    xd = torch.from_numpy(x).cuda()
    got = resample.resize_antialiased(xd, (12, 20)).cpu().numpy()                      # skimage's default: (1.5, 0.5)
    want = R.oracle64(x, (12, 20), (1.5, 0.5), "constant", 0.0)
    assert np.abs(got - want).max() <= R.gate(x, 0.0)
    assert np.array_equal(_bits(got), _bits(R.restatement(x, (12, 20), (1.5, 0.5), "constant", 0.0)))
    for mode in R.MODES:
        got = resample.resize_antialiased(xd[None], (9, 13), sigma=[[2.5, 0.75]], mode=mode, cval=50.0)[0].cpu().numpy()
        want = R.oracle64(x, (9, 13), (2.5, 0.75), mode, 50.0)
        assert np.abs(got - want).max() <= R.gate(x, 50.0), mode
        assert np.array_equal(_bits(got), _bits(R.restatement(x, (9, 13), (2.5, 0.75), mode, 50.0))), mode
    same = resample.resize_antialiased(xd, (48, 40), sigma=0.0, cval=7.0)              # equal shape, sigma 0: the identity
    assert torch.equal(same.view(torch.int32), xd.view(torch.int32))


def test_views_are_read_and_written_in_place(hip):
    """a (H, W, P).permute(2, 0, 1) view and a column slice of a wider buffer are read in place (the aligned 16-byte path, the element
    path and a strided sample axis all give the same bits); an output at a line offset of a larger buffer leaves the rest untouched"""
    from starcop_amd import resample
    x = np.stack([R.make_plane(41, 36, seed=s) for s in (11, 12)])
    dense = torch.from_numpy(x).cuda()
    want = resample.resize_antialiased(dense, (10, 9), sigma=[1.5, 2.5], mode="mirror")
    for p in range(2):
        assert np.array_equal(_bits(want[p].cpu().numpy()), _bits(R.restatement(x[p], (10, 9), (1.5, 2.5)[p], "mirror", 0.0)))
    hwp = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0))).cuda()
    view = hwp.permute(2, 0, 1)
    assert not view.is_contiguous() and view.stride(2) == 2
    assert torch.equal(resample.resize_antialiased(view, (10, 9), sigma=[1.5, 2.5], mode="mirror"), want)
    wide = torch.full((2, 41, 50), 777.0, device="cuda")
    wide[:, :, 7:43] = dense                                                          # misaligned line starts: the element path
    assert torch.equal(resample.resize_antialiased(wide[:, :, 7:43], (10, 9), sigma=[1.5, 2.5], mode="mirror"), want)

    big = torch.full((2, 30, 9), -5.0, device="cuda")
    ret = resample.resize_antialiased(dense, (10, 9), sigma=[1.5, 2.5], mode="mirror", out=big[:, 13:23])
    assert ret.data_ptr() == big[:, 13:23].data_ptr()
    assert torch.equal(big[:, 13:23], want)
    assert bool((big[:, :13] == -5.0).all()) and bool((big[:, 23:] == -5.0).all())
    pitched = torch.full((2, 10, 16), -5.0, device="cuda")                            # an output with a line pitch wider than ow
    resample.resize_antialiased(dense, (10, 9), sigma=[1.5, 2.5], mode="mirror", out=pitched[:, :, :9])
    assert torch.equal(pitched[:, :, :9], want) and bool((pitched[:, :, 9:] == -5.0).all())


def test_bad_arguments_surface_as_value_errors(hip):
    from starcop_amd import resample
    x = torch.zeros((300, 300), device="cuda")
    with pytest.raises(ValueError, match="T=258"):                                    # sigma 32: radius 128, 258 taps > 256
        resample.resize_antialiased(x, (75, 75), sigma=32.0)
    with pytest.raises(ValueError):
        resample.resize_antialiased(x, (75, 75), out=torch.zeros((75, 76), device="cuda"))
    with pytest.raises(ValueError):
        resample.resize_antialiased(x.double(), (75, 75))
