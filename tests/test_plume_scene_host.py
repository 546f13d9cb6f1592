"""Host side of whole-flight-line plume detection: the layout of sc_scene_planes_args, the argument checks of sc_scene_gather_planes /
sc_scene_core_counts / sc_head_conv_fwd_mosaic_prob (refused before anything touches a device), the product parsing and error paths
of pipeline.aviris_scene_predict and the argument errors of ModelModule.predict_scene (no GPU)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from starcop_amd import _lib, model_module as mm, pipeline, sentinel2
from starcop_amd._lib import StarcopHipError, check

FAKE = 0x10000        # a non-null, 16-byte aligned "device" address: every call below is refused before it could be used


def test_struct_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sc_scene_planes_args as gcc lays it out == the ctypes mirror"""
    a = _lib.sc_scene_planes_args
    assert _lib.SCENE_MAX_PLANES == 16 and a.src.size == 16 * 8 and a.clip_hi.size == 16 * 4
    assert [f[0] for f in a._fields_] == ["P", "H", "W", "pad_top", "pad_left", "n", "win_h", "win_w", "src", "row_stride", "col_stride",
                                          "ops", "fill_bits", "scale", "clip_lo", "clip_hi", "win", "win_host", "out"]
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = ["win_w", "src", "row_stride", "col_stride", "ops", "fill_bits", "scale", "clip_lo", "clip_hi", "win", "win_host", "out"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){'
                   'printf("%zu %d", sizeof(sc_scene_planes_args), SC_SCENE_MAX_PLANES);'
                   + "".join(f'printf(" %zu", offsetof(sc_scene_planes_args, {n}));' for n in names) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(a), 16] + [getattr(a, n).offset for n in names]


def _table(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 8))


def _planes_args(**kw):
    a = _lib.sc_scene_planes_args()
    a.P, a.H, a.W, a.pad_top, a.pad_left, a.n, a.win_h, a.win_w = 1, 40, 45, 12, 9, 1, 32, 32
    a.src[0], a.row_stride[0], a.col_stride[0] = FAKE, 45, 1
    a.win, a.out = FAKE, FAKE
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,match", [
    (dict(P=0), "P=0 outside"), (dict(P=17), "P=17 outside"), (dict(H=0), "bad scene dims"), (dict(pad_top=40), "larger than the pad"),
    (dict(n=0), "n=0 outside"), (dict(win_w=30), "multiple of 4"), (dict(out=FAKE + 4), "misaligned"), (dict(out=0), "null pointer"),
    (dict(src=(0, 0)), "null source plane 0"), (dict(src=(0, FAKE + 2)), "not aligned"), (dict(row_stride=(0, -1)), "negative stride"),
    (dict(ops=(0, 8)), "unknown ops"), (dict(ops=(0, 2), scale=(0, float("nan"))), "NaN"),
    (dict(ops=(0, 4), clip_lo=(0, 1.0), clip_hi=(0, 0.0)), "not ordered"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_gather_planes_refuses_bad_arguments(kw, match):
    lib = _lib.load()
    tab = _table([0, 0, 0, 0, 0, 0, 0, 0])
    a = _planes_args(**kw)
    a.win_host = tab.ctypes.data
    with pytest.raises(ValueError, match="sc_scene_gather_planes.*" + match):
        check(lib.sc_scene_gather_planes(C.byref(a), None))


def test_gather_planes_refuses_windows_outside_the_padded_scene():
    lib = _lib.load()
    tab = _table([64, 32, 0, 0, 0, 0, 0, 0])        # the last row would need a second reflection (64 + 32 - 12 > 2 * 40 - 1)
    a = _planes_args()
    a.win_host = tab.ctypes.data
    with pytest.raises(ValueError, match="sc_scene_gather_planes: window 0 .* leaves the reflect-padded scene"):
        check(lib.sc_scene_gather_planes(C.byref(a), None))
    with pytest.raises(ValueError, match="sc_scene_gather_planes: null arguments"):
        check(lib.sc_scene_gather_planes(None, None))


def test_core_counts_refuses_bad_arguments():
    lib = _lib.load()
    ok = _table([0, 0, 2, 12, 3, 13, 30, 35])
    call = lambda plane=FAKE, rs=45, cs=1, H=40, W=45, tab=ok, n=1, counts=FAKE, win=FAKE: check(      # noqa: E731
        lib.sc_scene_core_counts(plane, rs, cs, H, W, 0, win, tab.ctypes.data, n, counts, None))
    for kw, match in ((dict(plane=0), "null pointer"), (dict(counts=0), "null pointer"), (dict(win=0), "null pointer"),
                      (dict(H=0), "bad plane dims"), (dict(rs=-1), "negative stride"), (dict(n=0), "n=0 outside"),
                      (dict(plane=FAKE + 2), "misaligned"),
                      (dict(tab=_table([0, 0, 2, 13, 3, 13, 30, 35])), "core 0 .* does not fit"),          # 30 + 11 rows > 40
                      (dict(tab=_table([0, 0, 2, 12, 3, 13, 30, 36])), "core 0 .* does not fit"),
                      (dict(tab=_table([0, 0, 2, 12, 3, 13, -1, 0])), "core 0 .* does not fit")):
        with pytest.raises(ValueError, match="sc_scene_core_counts.*" + match):
            call(**kw)


def test_mosaic_prob_head_refuses_bad_arguments():
    lib = _lib.load()
    ok = _table([0, 0, 0, 19, 0, 37, 0, 0])

    def call(Cin=16, mode=_lib.SRC_RAW, x=FAKE, w=FAKE, prob=FAKE, ppitch=101, mask=FAKE, mpitch=101, mh=40, mw=101, valid=0, vrs=101, vcs=1,
             tab=ok, win=FAKE, N=1, H=32, W=64, C_=None):
        s = _lib.sc_src()
        s.x, s.C, s.mode = x, Cin if C_ is None else C_, mode
        check(lib.sc_head_conv_fwd_mosaic_prob(C.byref(s), w, None, prob, ppitch, mask, mpitch, mh, mw, valid, vrs, vcs, 0, -9999.0, win,
                                               tab.ctypes.data, N, Cin, H, W, None))
    for kw, match in ((dict(C_=8), "source channels"), (dict(Cin=33), "Cin must be"), (dict(mode=_lib.SRC_NORM), "unsupported source mode"),
                      (dict(w=0), "bad argument"), (dict(N=0), "bad argument"), (dict(prob=0, mask=0), "at least one of prob / mask"),
                      (dict(ppitch=100), "bad mosaic"), (dict(mpitch=100), "bad mosaic"), (dict(prob=FAKE + 2), "misaligned"),
                      (dict(valid=FAKE, vrs=-1), "negative stride"),
                      (dict(tab=_table([0, 0, 0, 33, 0, 37, 0, 0])), "core 0 .* is not inside the 32 x 64 plane"),
                      (dict(tab=_table([0, 0, 0, 19, 0, 37, 22, 0])), "core 0 does not fit the 40 x 101 mosaic"),
                      (dict(tab=_table([0, 0, 0, 19, 0, 37, 0, 65])), "core 0 does not fit the 40 x 101 mosaic")):
        with pytest.raises(ValueError, match="sc_head_conv_fwd_mosaic_prob.*" + match):
            call(**kw)


def test_input_products_parsing():
    assert pipeline.aviris_scene_products(mm.default_settings().dataset.input_products) == \
        [("mag1c", None), ("band", 640.0), ("band", 550.0), ("band", 460.0)]
    assert pipeline.aviris_scene_products(["2310nm", "mag1c"], normalize_by_acquisition_date=False) == [("band", 2310.0), ("mag1c", None)]
    for bad, norm in (("TOA_WV3_SWIR1", True), ("640nm", True), ("TOA_AVIRIS_640nm", False), ("ratio_aviris_2350_2310_out", True), ("rgb", True)):
        with pytest.raises(NotImplementedError, match=bad):
            pipeline.aviris_scene_products(["mag1c", bad], norm)


class _Stub:
    """what aviris_scene_predict reads of a model before it uses a device"""
    def __init__(self, products):
        self.input_products = products

    def predict_scene(self, *a, **kw):
        raise AssertionError("reached the device path")


def test_aviris_scene_predict_error_paths(tmp_path):
    folder = str(tmp_path / "ang20190101t000000_rdn")
    with pytest.raises(NotImplementedError, match="TOA_WV3_SWIR1"):
        pipeline.aviris_scene_predict(_Stub(["mag1c", "TOA_WV3_SWIR1"]), folder, toa_correction_factor=1.0)
    default = _Stub(mm.default_settings().dataset.input_products)
    with pytest.raises(ValueError, match="toa_correction_factor= or solar_altitude="):
        pipeline.aviris_scene_predict(default, folder)
    with pytest.raises(ValueError, match="no acquisition date"):
        pipeline.aviris_scene_predict(default, str(tmp_path / "flightline"), solar_altitude=50.0)
    with pytest.raises(NotImplementedError, match="Google Cloud Storage"):
        pipeline.aviris_scene_predict(default, folder, out_folder="gs://bucket/out", toa_correction_factor=1.0)
    with pytest.raises(NotImplementedError, match="Google Cloud Storage"):
        pipeline.aviris_scene_predict(default, "gs://bucket/ang20190101t000000_rdn", toa_correction_factor=1.0)
    with pytest.raises(FileNotFoundError):           # the factor is settled, the radiance file is not there
        pipeline.aviris_scene_predict(default, folder, solar_altitude=50.0)


def test_predict_scene_argument_errors():
    model = mm.ModelModule(mm.default_settings())
    planes = np.zeros((4, 40, 45), dtype=np.float32)
    with pytest.raises(ValueError, match="3 planes for the 4 input products"):
        model.predict_scene(planes[:3])
    with pytest.raises(ValueError, match="expected .C, H, W."):
        model.predict_scene(planes[0])
    with pytest.raises(TypeError, match="float32"):
        model.predict_scene(planes.astype(np.float64))
    with pytest.raises(TypeError, match="all numpy arrays or all device tensors"):
        model.predict_scene([planes[0], planes[1], planes[2], torch.zeros(40, 45)])
    with pytest.raises(ValueError, match="one shape"):
        model.predict_scene([planes[0], planes[1], planes[2], planes[3, :30]])
    with pytest.raises(ValueError, match="scales needs one entry per plane"):
        model.predict_scene(planes, scales=[1.0])
    with pytest.raises(ValueError, match="fill_value needs one entry per plane"):
        model.predict_scene(planes, fill_value=[-9999.0, 0.0])
    with pytest.raises(ValueError, match="multiple of 32"):
        model.predict_scene(planes, tile=100)
    with pytest.raises(ValueError, match="larger than the pad"):
        model.predict_scene(planes[:, :10])
    with pytest.raises(StarcopHipError):             # a CPU model: no fallback
        model.predict_scene(planes, fill_value=-9999.0)
    assert model.training                            # nothing was toggled on the way out


def test_predict_masks_into_argument_errors():
    net = mm.ModelModule(mm.default_settings()).network
    tab = (torch.zeros(1, 8, dtype=torch.int32), np.zeros((1, 8), np.int32), 0)
    x, prob, mask = torch.zeros(1, 4, 32, 32), torch.zeros(32, 32), torch.zeros(32, 32, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="eval mode"):
        net.train().predict_masks_into(x, prob, mask, tab)
    net.eval()
    with pytest.raises(ValueError, match="at least one of prob / mask"):
        net.predict_masks_into(x, None, None, tab)
    k4 = sentinel2.CDModel(device=torch.device("cpu")).model
    with pytest.raises(ValueError, match="1-class"):
        k4.predict_masks_into(torch.zeros(1, 13, 32, 32), prob, mask, tab)
