"""The host side of the mosaic (starcop_amd.mosaic): footprint boxes and the union grid against the restated scene of
tests/mosaic_util.py, the refusals of ``mosaic`` that need no device, and the layout of the structs of sc_mosaic."""
import numpy as np
import pytest
import torch

import mosaic_util as MU
from starcop_amd import mosaic as M
from starcop_amd import warp


# ------------------------------------------------------------------------------------------------ the restated scene
def test_scene_counts():
    """the numbers the scene was built for (on the restatement alone): inside pixels per source, coverage, nothing near a boundary"""
    ins = MU.inside((45, 88))
    assert ins.sum(axis=(1, 2)).tolist() == [1688, 2273, 1200, 673, 717, 0]
    assert np.bincount(ins.sum(axis=0).ravel()).tolist() == [670, 1450, 758, 743, 339]
    for shape in MU.SHAPES:
        assert (~MU.compared(shape)).mean() <= 1e-3
    assert not MU.inside((45, 152))[:, :, 128:].any()                     # the last tile column of the wide shape is empty


# ------------------------------------------------------------------------------------------------ footprint_box
@pytest.mark.parametrize("shape", MU.SHAPES)
def test_footprint_box_holds_every_inside_pixel(shape):
    for (name, ss, sgt, scrs), ins in zip(MU.SOURCES, MU.inside(shape)):
        r0, r1, c0, c1 = M.footprint_box(ss, sgt, scrs, MU.DST_GT, MU.DST_CRS, shape)
        assert 0 <= r0 and r1 <= shape[0] and 0 <= c0 and c1 <= shape[1], name
        rows, cols = np.nonzero(ins)
        if name == "far":
            assert rows.size == 0 and (r0 >= r1 or c0 >= c1)              # an empty intersection with the grid
            continue
        assert rows.min() >= r0 and rows.max() < r1 and cols.min() >= c0 and cols.max() < c1, name
        slack = (rows.min() - r0, r1 - (rows.max() + 1), cols.min() - c0, c1 - (cols.max() + 1))
        assert max(slack) <= 3, (name, slack)                             # at most 3 pixels beyond the tight bounding box per side


def test_footprint_box_without_coordinates_is_the_whole_grid():
    """an outline that reaches more than 30 degrees from the destination zone's central meridian (105 W) has no coordinates there"""
    box = M.footprint_box((10, 50), (-140.0, 1.0, 0.0, 40.0, 0.0, -1.0), 4326, MU.DST_GT, MU.DST_CRS, (45, 88))
    assert box == (0, 45, 0, 88)


# ------------------------------------------------------------------------------------------------ union_grid
def test_union_grid():
    grids = [(ss, sgt, scrs) for _, ss, sgt, scrs in MU.SOURCES[:5]]
    each = [warp.suggest_grid(ss, sgt, scrs, 32613) for ss, sgt, scrs in grids]
    (H, W), gt = M.union_grid(grids, 32613)
    res = gt[1]
    assert res == min(g[1] for _, g in each) and gt[5] == -res and gt[2] == gt[4] == 0.0      # the finest suggestion
    for v in (gt[0], gt[3]):
        assert abs(v / res - round(v / res)) < 1e-9                       # origins are multiples of the resolution
    for ss, sgt, scrs in grids:                                           # it covers every suggestion at its resolution
        (h, w), g = warp.suggest_grid(ss, sgt, scrs, 32613, res)
        assert g[0] >= gt[0] - 1e-6 and g[0] + w * res <= gt[0] + W * res + 1e-6
        assert g[3] <= gt[3] + 1e-6 and g[3] - h * res >= gt[3] - H * res - 1e-6
    (H60, W60), gt60 = M.union_grid(grids, 32613, 60.0)
    assert gt60[1] == 60.0 and gt60[0] % 60.0 == 0.0 and gt60[3] % 60.0 == 0.0
    # one grid alone is its own suggestion
    assert M.union_grid(grids[:1], 32613, 60.0) == warp.suggest_grid(*grids[0], 32613, 60.0)
    with pytest.raises(ValueError, match="2\\^31"):
        M.union_grid(grids, 32613, 1e-3)
    with pytest.raises(ValueError, match="no grids"):
        M.union_grid([], 32613)


# ------------------------------------------------------------------------------------------------ refusals without a device
GT = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)


def src(dtype=torch.float32, P=2, crs=None):
    return (torch.zeros((P, 4, 5), dtype=dtype), GT, crs)


def test_mosaic_refusals_need_no_device():
    with pytest.raises(ValueError, match="64"):
        M.mosaic([], GT, None, (4, 5))
    with pytest.raises(ValueError, match="64"):
        M.mosaic([src()] * 65, GT, None, (4, 5))
    with pytest.raises(ValueError, match="one dtype and plane count"):
        M.mosaic([src(), src(torch.float64)], GT, None, (4, 5))
    with pytest.raises(ValueError, match="one dtype and plane count"):
        M.mosaic([src(), src(P=3)], GT, None, (4, 5))
    for rule in ("max", "min", "mean"):
        with pytest.raises(ValueError, match="float32"):
            M.mosaic([src(torch.int16)], GT, None, (4, 5), rule=rule)
        with pytest.raises(ValueError, match="float32"):
            M.mosaic([(np.zeros((4, 5)), GT, None)], GT, None, (4, 5), rule=rule)
    with pytest.raises(ValueError, match="float32"):
        M.mosaic([src(torch.uint8)], GT, None, (4, 5), resampling="bilinear")
    sel = torch.zeros((4, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="select"):
        M.mosaic([src()], GT, None, (4, 5), rule="first", select=sel)
    with pytest.raises(ValueError, match="select"):
        M.mosaic([src()], GT, None, (4, 5), rule="index")
    with pytest.raises(ValueError, match="select"):
        M.mosaic([src()], GT, None, (4, 5), rule="index", select=torch.zeros((4, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="select"):
        M.mosaic([src()], GT, None, (4, 5), rule="index", select=torch.zeros((4, 5), dtype=torch.int64))
    with pytest.raises(ValueError, match="rule"):
        M.mosaic([src()], GT, None, (4, 5), rule="median")
    with pytest.raises(ValueError, match="key plane"):
        M.mosaic([src()], GT, None, (4, 5), key=2)
    # CRS pairs as warp.reproject refuses them
    with pytest.raises(NotImplementedError, match="3857"):
        M.mosaic([src(crs=4326), src(crs=3857)], GT, 4326, (4, 5))
    with pytest.raises(ValueError, match="None"):
        M.mosaic([src(crs=4326), src(crs=None)], GT, 4326, (4, 5))


# ------------------------------------------------------------------------------------------------ struct layout
def test_mosaic_structs_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sc_mosaic_source and sc_mosaic_args as gcc lays them out == the ctypes mirrors in _lib.py"""
    import ctypes
    import os
    import shutil
    import subprocess
    from starcop_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    sf = ("src_crs", "src_w", "box", "src", "row_stride", "col_stride")
    af = ("dst_crs", "N", "P", "elem_bytes", "rule", "key_plane", "resampling", "flags", "nodata_bits", "sources", "table", "out",
          "index", "count", "select")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){'
                    'printf("%zu %zu %d %d", sizeof(sc_mosaic_source), sizeof(sc_mosaic_args), SC_MOSAIC_MAX_SOURCES, SC_MOSAIC_MEAN_PLANES);'
                    'printf(" %d %d %d %d %d %d %d", SC_MOSAIC_FIRST, SC_MOSAIC_LAST, SC_MOSAIC_MAX, SC_MOSAIC_MIN, SC_MOSAIC_MEAN, '
                    'SC_MOSAIC_BY_INDEX, SC_MOSAIC_KEY_FLOAT);'
                    + "".join(f'printf(" %zu", offsetof(sc_mosaic_source, {f}));' for f in sf)
                    + "".join(f'printf(" %zu", offsetof(sc_mosaic_args, {f}));' for f in af) + "return 0;}\n")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(prog), "-o", str(tmp_path / "sz")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_lib.sc_mosaic_source), ctypes.sizeof(_lib.sc_mosaic_args), _lib.MOSAIC_MAX_SOURCES, _lib.MOSAIC_MEAN_PLANES,
            _lib.MOSAIC_FIRST, _lib.MOSAIC_LAST, _lib.MOSAIC_MAX, _lib.MOSAIC_MIN, _lib.MOSAIC_MEAN, _lib.MOSAIC_BY_INDEX,
            _lib.MOSAIC_KEY_FLOAT]
    want += [getattr(_lib.sc_mosaic_source, f).offset for f in sf] + [getattr(_lib.sc_mosaic_args, f).offset for f in af]
    assert got == want
