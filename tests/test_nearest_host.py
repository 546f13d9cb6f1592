"""Host side of the feature transform (no GPU): the brute-force oracle against scipy and against a result written out by hand,
every refusal of sc_edt_nearest before any launch, the ctypes mirror of sc_edt_nearest_args laid out as gcc lays out the header,
and the ValueErrors of the Python functions before the device is asked for."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

import morphology_util as U
import nearest_util as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def lib():
    from starcop_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


SEEDED = [(shape, d, 7000 + 10 * k + j) for k, shape in enumerate(((1, 70), (70, 1), (37, 53), (9, 65), (30, 41)))
          for j, d in enumerate((0.002, 0.05, 0.5))]


@pytest.mark.parametrize("shape,density,seed", SEEDED, ids=[f"{s[0]}x{s[1]}_{d}" for s, d, _ in SEEDED])
def test_brute_force_against_scipy(shape, density, seed):
    """the squared distance to scipy's nearest index equals ours everywhere; the indices are equal wherever the nearest target
    is unique (scipy breaks ties by a rule of its own)"""
    targets = U.bernoulli(shape, density, seed) != 0
    if not targets.any():
        targets[shape[0] // 2, shape[1] // 3] = True
    H, W = shape
    index, d2 = NU.nearest_brute(targets)
    assert np.array_equal(d2, U.d2_brute(targets))
    assert targets.reshape(-1)[index.reshape(-1)].all()
    sr, sc = ndimage.distance_transform_edt(~targets, return_indices=True)[1].astype(np.int64)
    py, px = np.mgrid[0:H, 0:W]
    assert np.array_equal((py - sr) ** 2 + (px - sc) ** 2, d2)
    ty, tx = np.nonzero(targets)
    all_d = (py.reshape(-1, 1) - ty[None, :]) ** 2 + (px.reshape(-1, 1) - tx[None, :]) ** 2
    unique = ((all_d == d2.reshape(-1, 1)).sum(1) == 1).reshape(H, W)
    assert unique.any() and np.array_equal((sr * W + sc)[unique], index[unique])


def test_tie_rule_by_hand():
    m, index, d2 = NU.four_symmetric()
    got_i, got_d = NU.nearest_brute(m)
    assert np.array_equal(got_i, index) and np.array_equal(got_d, d2)
    # the same column twice: the smaller row
    m = np.zeros((5, 3), dtype=np.uint8)
    m[0, 1] = m[4, 1] = 1
    assert NU.nearest_brute(m)[0][2].tolist() == [1, 1, 1]
    assert NU.nearest_brute(np.zeros((3, 4), dtype=np.uint8))[0].tolist() == [[-1] * 4] * 3
    ci, cd = NU.capped(index, d2, 1)
    assert np.array_equal(ci == -1, d2 > 1) and np.array_equal(cd == NU.FAR, d2 > 1)


def test_derived_oracles():
    lab = np.zeros((6, 9), dtype=np.int64)
    lab[1, 1], lab[4, 7] = 3, 5
    e = NU.expand_labels_ref(lab, 1)
    assert e.dtype == np.int32 and e[1, 2] == 3 and e[0, 1] == 3 and e[2, 2] == 0 and e[4, 6] == 5 and (e != 0).sum() == 10
    assert np.array_equal(NU.expand_labels_ref(lab, 0), lab)
    assert (NU.expand_labels_ref(lab, 20) != 0).all()
    r = NU.rings_ref(lab, 2, 1)
    assert r[1, 1] == 0 and r[1, 2] == 0 and r[2, 2] == 3 and r[1, 3] == 3 and r[1, 4] == 0 and r[4, 5] == 5
    data = np.arange(54, dtype=np.float32).reshape(6, 9)
    data[1, 1] = np.uint32(0x7FC01234).view(np.float32)
    f = NU.fill_nearest_ref(data, lab == 0)
    assert f.view(np.uint32)[0, 0] == 0x7FC01234 and f[5, 8] == data[4, 7]
    f = NU.fill_nearest_ref(data, lab == 0, max_distance=1)
    assert f.view(np.uint32)[0, 1] == 0x7FC01234 and f[0, 0] == 0.0 and f[5, 8] == 53.0


def _args(_lib, **kw):
    a = _lib.sc_edt_nearest_args()
    a.mask, a.N, a.H, a.W, a.index = 256, 1, 8, 8, 256
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_nearest_refusals_come_before_any_launch(lib):
    from starcop_amd import _lib
    call, wk, big = lib.sc_edt_nearest, ctypes.c_void_p(256), 1 << 30

    def refused(a, word, work=wk, nbytes=big):
        assert call(a, work, nbytes, None) == -1 and word in lib.sc_last_error(), lib.sc_last_error()
    assert call(None, wk, big, None) == -1
    refused(_lib.sc_edt_nearest_args(), b"null")
    refused(_args(_lib, W=32768), b"bad dims")
    refused(_args(_lib, H=0), b"bad dims")
    refused(_args(_lib, N=65536), b"bad dims")
    refused(_args(_lib, index=None), b"no output")
    refused(_args(_lib, stride_h=-1), b"stride")
    refused(_args(_lib, max_dist2=-1), b"max_dist2")
    refused(_args(_lib, variant=3), b"variant")
    refused(_args(_lib, variant=_lib.EDT_WINDOW), b"window")                         # no cap
    refused(_args(_lib, variant=_lib.EDT_WINDOW, max_dist2=(_lib.EDT_WINDOW_MAX_R + 1) ** 2), b"window")
    refused(_args(_lib, n_planes=9), b"n_planes")
    refused(_args(_lib, n_planes=-1), b"n_planes")
    refused(_args(_lib, n_planes=1), b"plane 0")                                      # null source and destination
    a = _args(_lib, n_planes=2)
    a.src[0], a.dst[0], a.src[1], a.dst[1] = 512, 1024, 2048, 2048
    refused(a, b"plane 1")                                                            # gathered in place
    a.dst[1], a.src_stride[1] = 4096, -64
    refused(a, b"plane 1")
    a.src_stride[1] = 64
    refused(a, b"workspace", nbytes=16)
    refused(a, b"aligned", work=ctypes.c_void_p(264))
    refused(a, b"null", work=None)
    for bad in (_args(_lib, W=32768), _args(_lib, index=None), _args(_lib, variant=_lib.EDT_WINDOW), _args(_lib, n_planes=9)):
        assert lib.sc_edt_nearest_call_workspace_bytes(bad) == 0
    assert lib.sc_edt_nearest_call_workspace_bytes(None) == 0


def test_nearest_workspace_bytes(lib):
    """the window needs what sc_edt's window needs; the envelope sc_edt's and two more bytes per padded pixel"""
    from starcop_amd import _lib
    w, edt = lib.sc_edt_nearest_workspace_bytes, lib.sc_edt_workspace_bytes
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (65536, 8, 8), (1, 32768, 8), (1, 8, 32768)):
        assert w(*bad) == 0
    for N, H, W in ((1, 1, 1), (3, 37, 53), (1, 2000, 2300), (2, 129, 257)):
        Hp = (H + 63) // 64 * 64
        assert w(N, H, W) == edt(N, H, W) + (N * W * Hp * 2 + 255) // 256 * 256
    e = _lib.sc_edt_args()
    e.mask, e.N, e.H, e.W, e.dist2, e.max_dist2 = 256, 1, 2000, 2300, 256, 9
    a = _args(_lib, H=2000, W=2300, max_dist2=9)
    assert lib.sc_edt_nearest_call_workspace_bytes(a) == lib.sc_edt_call_workspace_bytes(e) < 2000 * 2300 * 3
    a.variant = _lib.EDT_ENVELOPE
    assert lib.sc_edt_nearest_call_workspace_bytes(a) == w(1, 2000, 2300)
    a.variant, a.max_dist2 = 0, (_lib.EDT_WINDOW_MAX_R + 1) ** 2
    assert lib.sc_edt_nearest_call_workspace_bytes(a) == w(1, 2000, 2300)
    a.max_dist2 = 0
    assert lib.sc_edt_nearest_call_workspace_bytes(a) == w(1, 2000, 2300)


def test_nearest_args_layout_matches_the_c_compiler(tmp_path):
    from starcop_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    header = open(os.path.join(INCLUDE, "starcop_hip.h")).read()
    assert f"#define SC_EDT_NEAREST_MAX_PLANES {_lib.EDT_NEAREST_MAX_PLANES}\n" in header and _lib.EDT_NEAREST_MAX_PLANES == 8
    fields = [f[0] for f in _lib.sc_edt_nearest_args._fields_]
    src = tmp_path / "nearest_layout.c"
    prints = "".join(f'printf("%zu\\n", offsetof(sc_edt_nearest_args, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\n'
                   'int main(void){printf("%zu\\n", sizeof(sc_edt_nearest_args));' + prints + "return 0;}\n")
    exe = tmp_path / "nearest_layout"
    subprocess.run(["gcc", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.sc_edt_nearest_args)] + [getattr(_lib.sc_edt_nearest_args, f).offset for f in fields]


def test_argument_errors_come_before_the_device(monkeypatch):
    from starcop_amd import _lib, morphology as mo, plumes, products

    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_device", no_device)
    m = np.zeros((8, 9), dtype=np.uint8)
    lab = np.zeros((8, 9), dtype=np.int32)
    f = np.zeros((8, 9), dtype=np.float32)
    bad = [lambda: mo.nearest_index(m, to="zero"), lambda: mo.nearest_index(m, variant="banding"), lambda: mo.nearest_index(m[0]),
           lambda: mo.nearest_index(m, max_distance=-1.0), lambda: mo.nearest_index(m, variant="window"),
           lambda: mo.nearest_index(m, max_distance=mo.WINDOW_MAX_R + 1, variant="window"),
           lambda: mo.nearest_index(np.zeros((2, 32768), dtype=np.uint8)), lambda: mo.nearest_index([[0, 1]]),
           lambda: mo.expand_labels(lab, -1.0), lambda: mo.expand_labels(lab[0]), lambda: mo.expand_labels(f),
           lambda: mo.expand_labels(torch.zeros(8, 9)), lambda: mo.expand_labels(lab, float("nan")),
           lambda: mo.fill_nearest([f] * 9, m), lambda: mo.fill_nearest([], m), lambda: mo.fill_nearest(f[:4], m),
           lambda: mo.fill_nearest(f.astype(np.float64), m), lambda: mo.fill_nearest(f, m, max_distance=-2),
           lambda: mo.fill_nearest(torch.zeros(8, 9), m), lambda: mo.fill_nearest(f, m[0]),
           lambda: plumes.background_rings(lab, 0.5), lambda: plumes.background_rings(lab, 4, -1),
           lambda: plumes.background_rings(lab, 4, 4), lambda: plumes.background_rings(f, 4),
           lambda: plumes.background_rings(lab[0], 4), lambda: plumes.background_rings(lab, float("nan")),
           lambda: plumes.plume_table(m, background_ring_px=4), lambda: plumes.plume_table(m, mag1c=f, background_ring_px=0.0),
           lambda: plumes.plume_table(m, mag1c=f, background_ring_px=4, background_gap_px=5),
           lambda: plumes.table_from_stats({"area": np.zeros((1, 0))}, [0], 9, ring_stats={}),
           lambda: products.check_plume_background({"radius": 4}, "test"), lambda: products.check_plume_background({"gap_px": 1}, "test"),
           lambda: products.check_plume_background([4], "test"),
           lambda: products.annotate({}, m, None, None, plumes=True, plume_background={"ring_px": 4, "width": 2})]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} raised nothing")
    assert products.check_plume_background(None, "test") == {}
    assert products.check_plume_background({"ring_px": 8}, "test") == {"background_ring_px": 8, "background_gap_px": 0.0}
    assert products.check_plume_background({"ring_px": 8, "gap_px": 2}, "test") == {"background_ring_px": 8, "background_gap_px": 2}


def test_no_fallback_without_a_device():
    from starcop_amd import _lib, morphology as mo, plumes
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = np.ones((8, 9), dtype=np.uint8)
    f = np.ones((8, 9), dtype=np.float32)
    for call in (lambda: mo.nearest_index(m), lambda: mo.nearest_index(m, max_distance=0), lambda: mo.expand_labels(m, 0),
                 lambda: mo.expand_labels(m, 2), lambda: mo.fill_nearest(f, m), lambda: plumes.background_rings(m, 3)):
        with pytest.raises(_lib.StarcopHipError):
            call()
