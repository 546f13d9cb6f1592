"""``sc_tile_window_sums`` / ``datamodule.tile_window_sums``: fp64 window sums of resident label tiles -- exact for {0,1}
labels, inside the fp64 recursive-summation bound for real values, bit-identical between calls, equal to the integral-image
fractions ``ResidentTileSet.tiled_table`` used before on the production grid, and ValueError for bad arguments."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from starcop_amd import datamodule as dm  # noqa: E402

DEV = "cuda"
SHAPES = [(96, 80), (70, 45)]          # 45 floats = 180 bytes per row: the 16-byte phase of a row changes from row to row


def _windows(H, W):
    return [(0, 0, H, W),                        # the whole tile
            (5, 7, 1, 1),                        # one pixel
            (3, W - 2, H - 6, 1),                # a width-1 column
            (3, 5, 31, 17),                      # odd offsets, odd size
            (10, 12, 40, 24), (30, 20, 40, 24),  # two overlapping windows
            (3, 5, 31, 17),                      # a duplicate
            (H - 33, W - 21, 33, 21)]            # ends at the last row and column


def _ref(labels, wins):
    return np.array([[labels[m, r:r + h, c:c + w].sum(dtype=np.float64) for (r, c, h, w) in wins] for m in range(labels.shape[0])])


@pytest.mark.parametrize("shape", SHAPES)
def test_binary_labels_are_summed_exactly(hip, shape):
    rng = np.random.default_rng(11)
    labels = (rng.random((3,) + shape) < 0.3).astype(np.float32)
    wins = _windows(*shape)
    got = dm.tile_window_sums(torch.from_numpy(labels).to(DEV), wins)
    assert got.dtype == torch.float64 and got.shape == (3, len(wins)) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), _ref(labels, wins))


@pytest.mark.parametrize("shape", SHAPES)
def test_real_values_within_the_summation_bound_and_reproducible(hip, shape):
    rng = np.random.default_rng(12)
    labels = rng.uniform(-100, 100, (3,) + shape).astype(np.float32)
    wins = _windows(*shape)
    x = torch.from_numpy(labels).to(DEV)
    got_t = dm.tile_window_sums(x, wins)
    got, ref = got_t.cpu().numpy(), _ref(labels, wins)
    for m in range(3):
        for k, (r, c, h, w) in enumerate(wins):
            bound = (h * w) * 2.0 ** -53 * np.abs(labels[m, r:r + h, c:c + w]).sum(dtype=np.float64)
            err = abs(got[m, k] - ref[m, k])
            print(f"shape {shape} tile {m} window {k}: |got - ref| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (m, k, err, bound)
    again = dm.tile_window_sums(x, wins)
    assert torch.equal(got_t.view(torch.int64), again.view(torch.int64))


def test_unaligned_storage_takes_the_element_path(hip):
    """a label tensor that starts 4 bytes past a 16-byte boundary (a view into a larger buffer)"""
    rng = np.random.default_rng(13)
    labels = (rng.random((2, 70, 45)) < 0.5).astype(np.float32)
    buf = torch.zeros(labels.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = torch.from_numpy(labels).to(DEV).flatten()
    x = buf[1:].view(2, 70, 45)
    assert x.data_ptr() % 16 == 4
    wins = _windows(70, 45)
    assert np.array_equal(dm.tile_window_sums(x, wins).cpu().numpy(), _ref(labels, wins))


def test_production_grid_equals_the_integral_image_fractions(hip):
    """M=2 tiles of 512 x 512 on the 128 / 64 grid (49 windows): the fractions equal the float64 integral-image ones that
    ``tiled_table`` computed before this kernel (restated here), and ``tiled_table`` itself returns them"""
    rng = np.random.default_rng(14)
    y = np.zeros((2, 1, 512, 512), np.float32)
    y[0, 0, 40:300, 100:420] = rng.random((260, 320)) < 0.6
    y[1, 0, 500:512, 0:9] = 1
    wins = dm.create_windows((512, 512), (128, 128), (64, 64))
    assert len(wins) == 49
    lab = torch.from_numpy(y[:, 0]).to(DEV)
    ii = torch.zeros((2, 513, 513), dtype=torch.float64, device=DEV)
    ii[:, 1:, 1:] = lab.double().cumsum(1).cumsum(2)
    r = torch.tensor([w[0] for w in wins], device=DEV)
    c = torch.tensor([w[1] for w in wins], device=DEV)
    k = torch.arange(49, device=DEV)
    old = (ii[:, r + 128][:, k, c + 128] - ii[:, r][:, k, c + 128] - ii[:, r + 128][:, k, c] + ii[:, r][:, k, c]) / (128 * 128)
    new = dm.tile_window_sums(lab, wins) / (128 * 128)
    assert torch.equal(old, new)
    ts = dm.ResidentTileSet(np.zeros((2, 1, 512, 512), np.float32), y, ids=["a", "b"], device=DEV)
    table = ts.tiled_table((128, 128), (64, 64))
    assert np.array_equal(table["frac_positives"].values.reshape(2, 49), new.cpu().numpy())


def test_bad_arguments_raise_value_error(hip):
    x = torch.zeros((2, 32, 40), dtype=torch.float32, device=DEV)
    for win in ([(0, 0, 33, 40)], [(0, 1, 32, 40)], [(-1, 0, 4, 4)], [(0, 0, 0, 4)], [(0, 0, 8, 8), (30, 38, 3, 2)]):
        with pytest.raises(ValueError):
            dm.tile_window_sums(x, win)
    with pytest.raises(ValueError):
        dm.tile_window_sums(x, [])
    with pytest.raises(ValueError):
        dm.tile_window_sums(x.double(), [(0, 0, 4, 4)])
    with pytest.raises(ValueError):
        dm.tile_window_sums(x[:0], [(0, 0, 4, 4)])
    torch.cuda.synchronize()
    assert float(dm.tile_window_sums(x + 1, [(0, 0, 32, 40)])[1, 0]) == 32 * 40          # the library is still usable afterwards
