"""The scipy restatement of proposed_mask (tests/labels_util.py, what the GPU label tests compare against) pinned on hand-derived
answers that do not depend on scipy: the borders of the opening, 8-connectivity, the >= 200 threshold, alpha on the background
and NaN.  CPU only."""
import numpy as np

import labels_util as lu
from oracle import host_ref
from starcop_amd import mask_creation  # noqa: F401  (the module under test on the GPU must import on a CPU-only box)


def _case(mag, alpha):
    mag = np.asarray(mag, np.float32)
    rgba = np.zeros((4,) + mag.shape, np.uint8)
    rgba[3] = alpha
    return lu.proposed_mask(rgba, mag[None])


def test_opening_borders_by_hand():
    H, W = 12, 10
    # a 2-row band in the interior: every pixel has a cross neighbour outside the band -> the erosion is empty
    m = np.zeros((H, W), bool); m[5:7] = True
    assert not lu.dilated_opening(m).any()
    # the same band along the top edge: outside the image counts as set, so row 0 survives the erosion, and the two
    # dilations give back rows 0..2
    m = np.zeros((H, W), bool); m[0:2] = True
    want = np.zeros((H, W), bool); want[0:3] = True
    assert np.array_equal(lu.dilated_opening(m), want)
    # a 3-row interior band: the erosion keeps the middle row, the opening restores rows 4..6 and the dilation adds 3 and 7
    m = np.zeros((H, W), bool); m[4:7] = True
    want = np.zeros((H, W), bool); want[3:8] = True
    assert np.array_equal(lu.dilated_opening(m), want)
    # the restatement's opening equals the project's host opening with the cross (pinned against kornia's convention)
    rng = np.random.default_rng(3)
    m = rng.uniform(size=(33, 29)) < 0.6
    from scipy import ndimage
    e = ndimage.binary_dilation(host_ref.binary_opening(m, lu.CROSS), lu.CROSS, border_value=0)
    assert np.array_equal(lu.dilated_opening(m), e)


def test_diagonal_blobs_are_one_component():
    mag = np.zeros((14, 14), np.float32)
    mag[1:5, 1:5] = 500          # 4x4 blob, the opening keeps it whole
    mag[5:9, 5:9] = 500          # the next 4x4 blob touches it at one corner only: after the dilation they join diagonally
    alpha = np.zeros((14, 14), np.uint8); alpha[2, 2] = 255                     # label in the first blob only
    got = _case(mag, alpha)
    want = mag >= 200
    assert np.array_equal(got, want)
    # without the label nothing is selected
    assert not _case(mag, np.zeros_like(alpha)).any()


def test_threshold_keeps_exactly_200():
    # a 9x9 blob with one pixel exactly at the threshold and one just below it: D covers the whole blob (the hole is refilled
    # by the dilations) and one ring around it; the result keeps the blob's >= 200 pixels only
    mag = np.zeros((11, 11), np.float32)
    mag[1:10, 1:10] = 250
    mag[3, 3], mag[5, 5] = 200.0, 199.99
    alpha = np.zeros((11, 11), np.uint8); alpha[5, 5] = 1        # the label sits on the below-threshold pixel, inside D
    got = _case(mag, alpha)
    want = np.zeros((11, 11), bool); want[1:10, 1:10] = True; want[5, 5] = False
    assert np.array_equal(got, want)
    assert got[3, 3] and not got[5, 5]
    d = lu.dilated_opening(mag >= 200)
    assert d[5, 5] and d[0, 2] and not d[0, 1]         # the opening rounds the corners off: (1, 1) is not in it


def test_alpha_on_background_selects_nothing():
    mag = np.zeros((10, 10), np.float32); mag[1:5, 1:5] = 900
    alpha = np.zeros((10, 10), np.uint8); alpha[8, 8] = 255                    # far from the blob: outside D
    assert not _case(mag, alpha).any()
    alpha[5, 2] = 255                                                          # in D (the dilation's rim) but not in T
    got = _case(mag, alpha)
    want = np.zeros((10, 10), bool); want[1:5, 1:5] = True
    assert np.array_equal(got, want)


def test_nan_is_unset():
    mag = np.full((8, 8), 900, np.float32)
    mag[3, 4] = np.nan
    alpha = np.zeros((8, 8), np.uint8); alpha[0, 0] = 9
    got = _case(mag, alpha)
    want = np.ones((8, 8), bool); want[3, 4] = False
    assert np.array_equal(got, want)
    assert not _case(np.full((8, 8), np.nan, np.float32), np.full((8, 8), 1, np.uint8)).any()
