"""Host side of starcop_amd.morphology (no GPU): the oracles of the GPU tests agree with each other, every argument error is
raised before the device is asked for, the row-pass rule and the workspace size are pure host functions, and the ctypes mirror
of sc_edt_args is laid out as gcc lays out the header."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import morphology_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def lib():
    from starcop_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("name,mask", U.case_table(), ids=[c[0] for c in U.case_table()])
def test_oracles_agree(name, mask):
    """brute force (the definition) == rint(scipy's distances squared), for both target conventions; on the two large cases
    where the brute force is affordable, with few targets"""
    for targets in (mask != 0, mask == 0):
        if targets.size <= U.BRUTE_MAX_PIXELS or targets.sum() <= 64:
            assert np.array_equal(U.d2_brute(targets), U.d2_scipy(targets))


def test_disc_oracles_are_thresholds_of_the_distance():
    """scipy's dilation / erosion by the disc == d2 <= floor(r^2) / mask & (d2 to the unset pixels > floor(r^2))"""
    for seed, density in ((1, 0.05), (2, 0.5), (3, 0.9)):
        m = U.bernoulli((37, 53), density, seed)
        for r in (1, 1.5, 2, 3.2, 5, 17.5):
            t = int(np.floor(r * r))
            assert np.array_equal(U.dilate(m, r), (U.d2_brute(m != 0) <= t).astype(np.uint8))
            assert np.array_equal(U.erode(m, r), ((m != 0) & (U.d2_brute(m == 0) > t)).astype(np.uint8))
    assert U.disc(1).tolist() == [[False, True, False], [True, True, True], [False, True, False]]


def test_argument_errors_come_before_the_device(monkeypatch):
    from starcop_amd import _lib, morphology as mo, plumes, products

    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_device", no_device)
    m = np.zeros((8, 9), dtype=np.uint8)
    bad = [lambda: mo.distance_transform(m, pixel_size=0.0), lambda: mo.distance_transform(m, pixel_size=-1.0),
           lambda: mo.distance_transform(m, max_distance=-0.5), lambda: mo.distance_transform(m, to="zero"),
           lambda: mo.distance_transform(m, variant="banding"), lambda: mo.distance_transform(m[0]),
           lambda: mo.distance_transform(m[None, None]), lambda: mo.distance_transform(m, variant="window"),
           lambda: mo.distance_transform(m, max_distance=mo.WINDOW_MAX_R + 1, variant="window"),
           lambda: mo.distance_transform(np.zeros((2, 32768), dtype=np.uint8)),
           lambda: mo.dilate(m, -1), lambda: mo.erode(m, -0.1), lambda: mo.opening(m, -2), lambda: mo.closing(m, float("nan")),
           lambda: mo.dilate(m[0], 1), lambda: mo.remove_small_objects(m[0], 3), lambda: mo.remove_small_objects(m, 3, connectivity=3),
           lambda: plumes.match_plumes(m, m, tolerance_px=-1.0),
           lambda: products.clean({"pred_binary": torch.zeros(8, 9, dtype=torch.uint8)}, exclude=np.zeros((8, 8), dtype=np.uint8)),
           lambda: products.clean({"pred_binary": torch.zeros(8, 9, dtype=torch.uint8)}, open_radius=-1.0),
           lambda: products.check_clean({"radius": 1}, "test"), lambda: products.check_clean([1], "test")]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} raised nothing")
    with pytest.raises(ValueError, match="reproject_like"):
        products.clean({"pred_binary": torch.zeros(8, 9, dtype=torch.uint8)}, exclude=torch.zeros(9, 8))
    products.check_clean(None, "test")
    products.check_clean({"open_radius": 1, "min_area": 4}, "test")


def test_no_fallback_without_a_device():
    from starcop_amd import _lib, morphology as mo
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = np.ones((8, 9), dtype=np.uint8)
    for call in (lambda: mo.opening(m, 1), lambda: mo.distance_transform(m), lambda: mo.remove_small_objects(m, 4),
                 lambda: mo.dilate(m, 0)):
        with pytest.raises(_lib.StarcopHipError):
            call()


def test_edt_variant_rule(lib):
    from starcop_amd import _lib, morphology as mo
    R = _lib.EDT_WINDOW_MAX_R
    header = open(os.path.join(INCLUDE, "starcop_hip.h")).read()
    assert int(re.search(r"#define SC_EDT_WINDOW_MAX_R (\d+)", header).group(1)) == R
    assert int(re.search(r"#define SC_EDT_FAR (0x[0-9A-Fa-f]+)", header).group(1), 16) == _lib.EDT_FAR == 2 ** 31 - 1
    W, E = _lib.EDT_WINDOW, _lib.EDT_ENVELOPE
    v = lib.sc_edt_variant
    assert v(100, 200, 0, 0) == E                                     # no cap
    assert v(100, 200, 1, 0) == W and v(100, 200, 2, 0) == W
    assert v(100, 200, R * R, 0) == W and v(100, 200, (R + 1) ** 2 - 1, 0) == W       # floor(sqrt(cap)) == R
    assert v(100, 200, (R + 1) ** 2, 0) == E                          # one above
    assert v(100, 200, 2 ** 31 - 2, 0) == E
    assert v(100, 200, R * R, E) == E and v(100, 200, 0, E) == E and v(100, 200, R * R, W) == W
    assert v(100, 200, (R + 1) ** 2, W) == -1 and b"window" in lib.sc_last_error()
    assert v(100, 200, 0, W) == -1
    assert v(100, 200, 4, 3) == -1 and v(0, 200, 4, 0) == -1 and v(100, 32768, 4, 0) == -1
    assert mo.edt_variant(100, 200, R * R) == "window" and mo.edt_variant(100, 200, (R + 1) ** 2) == "envelope"
    assert mo.edt_variant(100, 200, 9, "envelope") == "envelope"
    with pytest.raises(ValueError):
        mo.edt_variant(100, 200, (R + 1) ** 2, "window")


def test_edt_workspace_bytes(lib):
    w = lib.sc_edt_workspace_bytes
    assert w(1, 1, 1) > 0 and w(3, 37, 53) > w(1, 37, 53) > 0
    assert w(1, 2000, 2300) >= 2000 * 2300 * 10                       # bits and carries, g, the envelope's stack and result
    assert w(1, 32767, 32767) > 0
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (65536, 8, 8), (1, 32768, 8), (1, 8, 32768)):
        assert w(*bad) == 0
    # the calls themselves refuse bad arguments before anything is launched (no device needed to be refused)
    from starcop_amd import _lib
    a = _lib.sc_edt_args()
    assert lib.sc_edt(a, None, 0, None) == -1
    a.mask, a.N, a.H, a.W, a.within = 256, 1, 8, 32768, 256
    assert lib.sc_edt(a, ctypes.c_void_p(256), 1 << 30, None) == -1 and b"bad dims" in lib.sc_last_error()
    a.W = 8
    assert lib.sc_edt(a, ctypes.c_void_p(256), 16, None) == -1 and b"workspace" in lib.sc_last_error()
    assert lib.sc_edt(a, ctypes.c_void_p(264), 1 << 30, None) == -1 and b"aligned" in lib.sc_last_error()
    a.thresh2 = _lib.EDT_FAR
    assert lib.sc_edt(a, ctypes.c_void_p(256), 1 << 30, None) == -1 and b"thresh2" in lib.sc_last_error()
    assert lib.sc_edt_call_workspace_bytes(a) == 0                   # 0 where the call would refuse
    # the size of a call follows its row pass: a thresholded mask at a small radius needs the band tables and g only
    a.H, a.W, a.thresh2 = 2000, 2300, 9
    small, full = lib.sc_edt_call_workspace_bytes(a), w(1, 2000, 2300)
    assert 2000 * 2300 * 2 < small < 2000 * 2300 * 3 and small < full
    a.thresh2 = (_lib.EDT_WINDOW_MAX_R + 1) ** 2
    assert lib.sc_edt_call_workspace_bytes(a) == full
    a.thresh2, a.variant = 9, _lib.EDT_ENVELOPE
    assert lib.sc_edt_call_workspace_bytes(a) == full
    a.H, a.W, a.thresh2, a.variant = 8, 8, 0, 0
    a.within = None
    assert lib.sc_edt(a, ctypes.c_void_p(256), 1 << 30, None) == -1 and b"no output" in lib.sc_last_error()
    a.dist, a.pixel_size = 256, 0.0
    assert lib.sc_edt(a, ctypes.c_void_p(256), 1 << 30, None) == -1 and b"pixel_size" in lib.sc_last_error()
    a.pixel_size, a.variant = 1.0, _lib.EDT_WINDOW                   # distances without a cap cannot take the window
    assert lib.sc_edt(a, ctypes.c_void_p(256), 1 << 30, None) == -1 and b"window" in lib.sc_last_error()
    assert lib.sc_label_keep(None, None, None, 1, 1, 8, 8, None) == -1
    assert lib.sc_label_keep(ctypes.c_void_p(256), ctypes.c_void_p(256), ctypes.c_void_p(256), 1, -1, 8, 8, None) == -1


def test_edt_args_layout_matches_the_c_compiler(tmp_path):
    from starcop_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in _lib.sc_edt_args._fields_]
    src = tmp_path / "edt_layout.c"
    prints = "".join(f'printf("%zu\\n", offsetof(sc_edt_args, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){printf("%zu\\n", sizeof(sc_edt_args));'
                   + prints + "return 0;}\n")
    exe = tmp_path / "edt_layout"
    subprocess.run(["gcc", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.sc_edt_args)] + [getattr(_lib.sc_edt_args, f).offset for f in fields]
