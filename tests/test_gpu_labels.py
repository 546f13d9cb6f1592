"""Connected components (sc_connected_components) bit-equal to scipy.ndimage.label, and the plume label mask (sc_proposed_mask)
bit-equal to the scipy restatement of starcop/data/mask_creation.py:6-27 in tests/labels_util.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import labels_util as lu  # noqa: E402
from starcop_amd import _lib, mask_creation as mc  # noqa: E402

DEV = "cuda"
STRUCT = {1: None, 2: lu.EIGHT}            # scipy's default structure is the cross (4-connectivity)


def _scipy_label(m, conn):
    from scipy import ndimage
    lab, n = ndimage.label(m, structure=STRUCT[conn])
    return lab.astype(np.int32), n


def _check_cc(m, conn):
    """m: (H, W) or (N, H, W) bool numpy"""
    lab, cnt = mc.connected_components(torch.from_numpy(m).to(DEV), connectivity=conn)
    lab = lab.cpu().numpy()
    if m.ndim == 2:
        want, n = _scipy_label(m, conn)
        assert cnt == n, (m.shape, conn, cnt, n)
        assert np.array_equal(lab, want), (m.shape, conn, int((lab != want).sum()))
        return
    cnt = cnt.cpu().numpy()
    for i in range(m.shape[0]):
        want, n = _scipy_label(m[i], conn)
        assert cnt[i] == n, (m.shape, i, conn, cnt[i], n)
        assert np.array_equal(lab[i], want), (m.shape, i, conn, int((lab[i] != want).sum()))


SHAPES = [(1, 1), (1, 300), (300, 1), (7, 13), (65, 127), (512, 512), (16, 512, 512), (1280, 1242), (700, 8000)]
DENSITIES = (0.05, 0.3, 0.41, 0.5, 0.59, 0.7, 0.95)


@pytest.mark.parametrize("conn", (1, 2))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cc_random_vs_scipy(hip, shape, conn):
    rng = np.random.default_rng(1000 * conn + sum(shape))
    big = np.prod(shape) > 2_000_000
    for dens in (DENSITIES[2], DENSITIES[4]) if big else DENSITIES:
        _check_cc(rng.uniform(size=shape) < dens, conn)


@pytest.mark.parametrize("conn", (1, 2))
def test_cc_special_masks(hip, conn):
    for shape in [(1, 1), (7, 13), (130, 200), (512, 512)]:
        _check_cc(np.zeros(shape, bool), conn)
        _check_cc(np.ones(shape, bool), conn)
    # checkerboard: one component with 8-connectivity, H*W/2 with 4-connectivity
    H, W = 256, 384
    cb = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0
    lab, cnt = mc.connected_components(cb, connectivity=conn)
    assert cnt == (1 if conn == 2 else H * W // 2)
    _check_cc(cb, conn)
    # a one-pixel diagonal line through every 64 x 64 tile corner (and the anti-diagonal), joined only across the corners
    n = 512
    d = np.eye(n, dtype=bool)
    _check_cc(d, conn)
    _check_cc(d[:, ::-1].copy(), conn)
    _check_cc(d | d[:, ::-1], conn)
    # a comb: a spine along the bottom row with one-pixel teeth in every other column, plus a comb hanging from the top
    comb = np.zeros((300, 257), bool)
    comb[-1, :] = True
    comb[:, ::2] = True
    comb[0, 1::4] = True
    _check_cc(comb, conn)
    comb2 = np.zeros((300, 257), bool)
    comb2[0, :] = True
    comb2[:-1, 1::2] = True
    _check_cc(comb2, conn)


def _spiral(n):
    """a one-pixel path spiralling clockwise into the centre of an n x n image, its turns one empty line apart: one component
    whose pixels are joined only along the path (it crosses every tile many times)"""
    m = np.zeros((n, n), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):                      # straight on, else turn right once
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= fy < n and 0 <= fx < n and m[fy, fx]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def test_cc_spiral(hip):
    from scipy import ndimage
    m = _spiral(512)
    _, n4 = ndimage.label(m)
    assert n4 == 1 and m.mean() > 0.45             # the wall is one path that fills about half the image
    for conn in (1, 2):
        lab, cnt = mc.connected_components(m, connectivity=conn)
        assert cnt == 1
        assert np.array_equal(lab, m.astype(np.int32))


def test_cc_numpy_and_repeats(hip):
    rng = np.random.default_rng(5)
    m = rng.uniform(size=(4, 300, 411)) < 0.59
    lab, cnt = mc.connected_components(m)
    assert isinstance(lab, np.ndarray) and lab.dtype == np.int32 and cnt.shape == (4,)
    md = torch.from_numpy(m).to(DEV)
    a, ca = mc.connected_components(md, connectivity=1)
    b, cb = mc.connected_components(md.to(torch.uint8), connectivity=1)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    # batch == image by image
    for i in range(4):
        li, ci = mc.connected_components(m[i])
        assert np.array_equal(lab[i], li) and cnt[i] == ci


def _pm_inputs(seed, B, H, W):
    rng = np.random.default_rng(seed)
    fields = [lu.plume_field(rng, H, W, blobs=max(4, (H * W) // 30000)) for _ in range(B)]
    mag = np.stack([f[0] for f in fields])          # (B, 1, H, W)
    rgba = np.stack([f[1] for f in fields])         # (B, 4, H, W)
    return mag, rgba


@pytest.mark.parametrize("shape", [(1, 512, 512), (16, 512, 512), (1, 1280, 1242)], ids=lambda s: "x".join(map(str, s)))
def test_proposed_mask_vs_oracle(hip, shape):
    B, H, W = shape
    mag, rgba = _pm_inputs(11 + B + H, B, H, W)
    magd, rgbad = torch.from_numpy(mag).to(DEV), torch.from_numpy(rgba).to(DEV)
    got = mc.proposed_mask(rgbad, magd)                       # alpha read in place from channel 3 of the (B, 4, H, W) tensor
    assert got.dtype == torch.bool and got.shape == (B, H, W)
    got = got.cpu().numpy()
    nsel = 0
    for i in range(B):
        want = lu.proposed_mask(rgba[i], mag[i])
        assert np.array_equal(got[i], want), (shape, i, int((got[i] != want).sum()))
        nsel += int(want.sum())
    assert nsel > 0                                            # the fields do select plumes
    # repeated calls give identical bytes; batch == image by image; numpy in -> numpy out
    again = mc.proposed_mask(rgbad, magd).cpu().numpy()
    assert np.array_equal(got, again)
    for i in range(min(B, 3)):
        one = mc.proposed_mask(rgbad[i], magd[i]).cpu().numpy()
        assert np.array_equal(one, got[i])
        host = mc.proposed_mask(rgba[i], mag[i])
        assert isinstance(host, np.ndarray) and host.dtype == bool and np.array_equal(host, got[i])


def test_proposed_mask_small_and_odd_shapes(hip):
    rng = np.random.default_rng(17)
    for (H, W) in [(1, 1), (1, 300), (300, 1), (7, 13), (65, 127), (64, 64), (129, 63)]:
        for _ in range(3):
            mag = rng.choice(np.array([0.0, 150.0, 199.99, 200.0, 900.0, np.nan], np.float32), size=(1, H, W),
                             p=[.2, .1, .05, .1, .5, .05])
            rgba = np.zeros((4, H, W), np.uint8)
            rgba[3] = (rng.uniform(size=(H, W)) < 0.05) * 255
            want = lu.proposed_mask(rgba, mag)
            got = mc.proposed_mask(rgba, mag)
            assert np.array_equal(got, want), (H, W, int((got != want).sum()))


def test_proposed_mask_strided_inputs(hip):
    """mag1c as band 0 of a multi-band stack and alpha as the last band of a float label tensor"""
    B, H, W = 3, 200, 333
    mag, rgba = _pm_inputs(23, B, H, W)
    stack = torch.from_numpy(np.concatenate([mag, np.full_like(mag, 7.0)], 1)).to(DEV)   # (B, 2, H, W), band 0 mag1c
    lab = torch.from_numpy(rgba.astype(np.float32)).to(DEV)
    got = mc.proposed_mask(lab, stack).cpu().numpy()
    for i in range(B):
        assert np.array_equal(got[i], lu.proposed_mask(rgba[i], mag[i])), i


def test_bad_arguments_raise(hip):
    lib = _lib.load()
    work = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    m = torch.ones((2, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        mc.connected_components(m, connectivity=3)
    with pytest.raises(ValueError):
        mc.connected_components(m, connectivity=0)
    with pytest.raises(ValueError):
        mc.connected_components(torch.ones((0, 8, 8), dtype=torch.uint8, device=DEV))
    lab = torch.empty((2, 8, 8), dtype=torch.int32, device=DEV)
    cnt = torch.empty(2, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    for N, H, W in [(0, 8, 8), (2, 0, 8), (2, 8, -1), (65536, 8, 8), (1, 65536, 65536)]:
        assert lib.sc_connected_components(p(m), 2, p(lab), p(cnt), p(work), work.numel(), N, H, W, _lib.stream()) == -1
        with pytest.raises(ValueError, match="bad dims"):
            _lib.check(lib.sc_proposed_mask(p(work), 64, p(m), 64, 200.0, _lib.SE_CROSS, p(m), p(work), work.numel(), N, H, W,
                                            _lib.stream()))
    assert lib.sc_label_workspace_bytes(0, 8, 8) == 0
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(lib.sc_connected_components(p(m), 2, p(lab), p(cnt), p(work), 8, 2, 8, 8, _lib.stream()))
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(lib.sc_connected_components(None, 2, p(lab), p(cnt), p(work), work.numel(), 2, 8, 8, _lib.stream()))
    with pytest.raises(ValueError, match="se_bits"):
        _lib.check(lib.sc_proposed_mask(p(work), 64, p(m), 64, 200.0, 512, p(m), p(work), work.numel(), 1, 8, 8, _lib.stream()))
    with pytest.raises(ValueError):
        mc.proposed_mask(torch.zeros((4, 8, 8), dtype=torch.uint8, device=DEV), torch.zeros((1, 8, 9), device=DEV))
    with pytest.raises(_lib.StarcopHipError):
        mc.connected_components(torch.ones((8, 8), dtype=torch.uint8), connectivity=2)     # a CPU tensor is not a device tensor
