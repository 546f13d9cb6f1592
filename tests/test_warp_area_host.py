"""The host side of the footprint resampling modes (warp.reproject with average / max / min / mode, sc_warp_area_args): what is refused
before a device is needed, the struct layout against the C compiler, and the numpy restatement of tests/warp_area_util.py against
an independent form.  No device."""
import numpy as np
import pytest
import torch

import warp_area_util as A
from starcop_amd import mosaic, products, warp

GT = (-104.03127, 5.4223e-4, 0.0, 32.51731, 0.0, -5.4223e-4)


def test_resampling_names():
    assert set(warp.RESAMPLING) == {"nearest", "bilinear", "average", "max", "min", "mode"}
    assert len(set(warp.RESAMPLING.values())) == 6
    assert set(warp.AREA_RESAMPLING) | set(warp.POINT_RESAMPLING) == set(warp.RESAMPLING)


@pytest.mark.parametrize("mode, dtype", [("average", "uint8"), ("average", "float64"), ("average", "int16"), ("mode", "float32"),
                                         ("mode", "int8"), ("mode", "uint16"), ("max", "int16"), ("min", "float64"), ("max", "bool")])
def test_dtype_refusals_name_resampling(mode, dtype):
    """numpy input and torch input, both before any device use"""
    with pytest.raises(ValueError, match="resampling"):
        warp.reproject(np.zeros((4, 5), dtype=dtype), GT, 4326, GT, 4326, (4, 5), resampling=mode)
    with pytest.raises(ValueError, match="resampling"):
        warp.reproject(torch.from_numpy(np.zeros((4, 5), dtype=dtype)), GT, 4326, GT, 4326, (4, 5), resampling=mode)


def test_other_refusals():
    a = np.zeros((4, 5), dtype=np.float32)
    for name in ("cubic", "lanczos", "sum"):
        with pytest.raises(ValueError, match="resampling"):
            warp.reproject(a, GT, 4326, GT, 4326, (4, 5), resampling=name)
    for name in ("nearest", "bilinear"):
        with pytest.raises(ValueError, match="return_coverage"):
            warp.reproject(a, GT, 4326, GT, 4326, (4, 5), resampling=name, return_coverage=True)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_coverage"):
            warp.reproject(a, GT, 4326, GT, 4326, (4, 5), resampling="average", min_coverage=bad)
    with pytest.raises(ValueError, match="variant"):
        warp.reproject(a, GT, 4326, GT, 4326, (4, 5), resampling="nearest", variant="lanes")
    with pytest.raises(NotImplementedError, match="3857"):
        warp.reproject(a, GT, 4326, GT, 3857, (4, 5), resampling="average")


@pytest.mark.parametrize("name", ["average", "max", "min", "mode"])
def test_mosaic_refuses_the_footprint_modes(name):
    src = [(np.zeros((4, 5), dtype=np.float32), GT, 4326)]
    with pytest.raises(ValueError, match="resampling"):
        mosaic.mosaic(src, GT, 4326, (4, 5), resampling=name)


def test_regrid_refusals():
    out = {"mf": np.zeros((4, 5), dtype=np.float32), "pred_binary": np.zeros((4, 5), dtype=np.uint8)}
    with pytest.raises(ValueError, match="mask_resampling"):
        products.regrid(out, GT, 4326, 32613, 60.0, mask_resampling="average")
    with pytest.raises(ValueError, match="mask_resampling"):
        products.regrid(out, GT, 4326, 32613, 60.0, mask_resampling="bilinear")
    with pytest.raises(ValueError, match="resampling"):
        products.regrid(out, GT, 4326, 32613, 60.0, resampling="mode")
    with pytest.raises(ValueError, match="min_coverage"):
        products.regrid(out, GT, 4326, 32613, 60.0, resampling="average", min_coverage=2.0)


def test_auto_variant_is_a_host_decision():
    for name, want in (("down12_aligned", "lanes"), ("up3", "thread")):
        ds, dgt, dcrs, ss, sgt, scrs = A.GRIDS[name]
        assert warp.area_variant(ds, dgt, dcrs, sgt, scrs) == want


def test_warp_area_args_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sc_warp_area_args as gcc lays it out == the ctypes mirror in _lib.py"""
    import ctypes
    import os
    import shutil
    import subprocess
    from starcop_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f for f, _ in _lib.sc_warp_area_args._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){printf("%zu %d %d %d %d %d", '
                   'sizeof(sc_warp_area_args), SC_WARP_AREA_AVERAGE, SC_WARP_AREA_MAX, SC_WARP_AREA_MIN, SC_WARP_AREA_MODE, '
                   'SC_WARP_AREA_THREAD * 10 + SC_WARP_AREA_LANES);'
                   + "".join(f'printf(" %zu", offsetof(sc_warp_area_args, {f}));' for f in fields) + "return 0;}\n")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_lib.sc_warp_area_args), _lib.WARP_AREA_AVERAGE, _lib.WARP_AREA_MAX, _lib.WARP_AREA_MIN, _lib.WARP_AREA_MODE,
            _lib.WARP_AREA_THREAD * 10 + _lib.WARP_AREA_LANES] + [getattr(_lib.sc_warp_area_args, f).offset for f in fields]
    assert got == want
    assert [warp.RESAMPLING[k] for k in ("average", "max", "min", "mode")] == want[1:5]


def test_restatement_against_block_reductions():
    """a 108 x 156 plane without holes, 12x onto a shared-lattice 9 x 13 grid in one CRS: the restatement is the block mean / max,
    and every pixel is covered entirely"""
    rng = np.random.default_rng(5)
    a = (rng.standard_normal((108, 156)) * 300 + 200).astype(np.float32)
    sgt, dgt = (600120.0, 5.0, 0.0, 3590460.0, 0.0, -5.0), (600120.0, 60.0, 0.0, 3590460.0, 0.0, -60.0)
    fp = A.Footprints(A.boxes_ref((9, 13), dgt, 32613, sgt, 32613), a.shape)
    assert not fp.geom_tie.any() and len(fp.pix) == 9 * 13
    blocks = a.astype(np.float64).reshape(9, 12, 13, 12)
    for mode, want in (("average", blocks.mean((1, 3))), ("max", blocks.max((1, 3))), ("min", blocks.min((1, 3)))):
        for mc in (0.0, 0.5, 1.0 - 1e-6):
            val, cov, valid, tie = A.reduce_ref(a, -9999.0, fp, mode, mc)
            assert valid.all() and not tie.any()
            assert float(np.abs(val.astype(np.float64) - want).max()) <= 1e-12
            assert float(np.abs(cov - 1.0).max()) <= 1e-12
    # the sliver rule: the same grids with corners 1e-11 px off the lattice take the same 144 samples
    off = (sgt[0] - 5e-11, 5.0, 0.0, sgt[3] + 5e-11, 0.0, -5.0)
    fp2 = A.Footprints(A.boxes_ref((9, 13), dgt, 32613, off, 32613), a.shape)
    assert all(len(fp2.pix[k][0]) == 12 and len(fp2.pix[k][1]) == 12 for k in fp2.pix) and not fp2.geom_tie.any()
    assert np.array_equal(A.reduce_ref(a, -9999.0, fp2, "max")[0], blocks.max((1, 3)).astype(np.float32))
    # a class map: the mode of a block, ties to the smallest value
    m = A.class_map((108, 156), 4)
    got = A.reduce_ref(m, 255, fp, "mode")[0]
    want = np.array([[np.bincount(m[r * 12:(r + 1) * 12, c * 12:(c + 1) * 12].ravel(), minlength=256).argmax() for c in range(13)]
                     for r in range(9)], dtype=np.uint8)
    assert np.array_equal(got, want) and len(np.unique(m)) == 4
    t = np.zeros((12, 12), dtype=np.uint8)
    t[:6] = 9
    t[6:] = 3                                                                    # 72 against 72
    one = A.Footprints(A.boxes_ref((1, 1), (0.0, 12.0, 0.0, 0.0, 0.0, -12.0), None, (0.0, 1.0, 0.0, 0.0, 0.0, -1.0), None), t.shape)
    assert A.reduce_ref(t, 255, one, "mode")[0][0, 0] == 3


def test_restatement_counts_and_coverage():
    """holes lower the coverage, the part of a box outside the raster too; min_coverage decides"""
    a = np.full((4, 4), 2.0, dtype=np.float32)
    a[0, 0], a[1, 1] = -9999.0, np.nan
    sgt = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
    fp = A.Footprints(A.boxes_ref((2, 2), (-2.0, 4.0, 0.0, 0.0, 0.0, -4.0), None, sgt, None), a.shape)      # pixel (0, 0): half outside
    val, cov, valid, _ = A.reduce_ref(a, -9999.0, fp, "average", 0.0)
    assert cov[0, 0] == 6.0 / 16.0 and val[0, 0] == 2.0 and valid[0, 0]
    assert cov[0, 1] == 8.0 / 16.0 and not valid[1, 0] and not valid[1, 1]      # rows 4..8 are below the raster
    assert not A.reduce_ref(a, -9999.0, fp, "average", 0.5)[2][0, 0] and A.reduce_ref(a, -9999.0, fp, "average", 0.5)[2][0, 1]
