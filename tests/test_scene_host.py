"""Host side of the whole-scene cloud mask: the window plan of scene.scene_windows (under its sentinel2 spelling), the table check
and batch loop of starcop_amd.scene and the argument checks of CDModel.predict_scene (no GPU)."""
import itertools

import numpy as np
import pytest
import torch

from scene_util import coverage
from starcop_amd import sentinel2
from starcop_amd._lib import StarcopHipError

SIZES = (33, 50, 64, 150, 217, 790)


@pytest.mark.parametrize("tile,halo", list(itertools.product((32, 96, 256), (0, 32, 320))), ids=lambda v: str(v))
def test_plan_properties(tile, halo):
    for H, W in itertools.product(SIZES, SIZES):
        plan = sentinel2.scene_windows(H, W, tile, halo)
        assert plan.pad_rows == sentinel2.find_padding(H, 32) and plan.pad_cols == sentinel2.find_padding(W, 32)
        Hp, Wp = plan.padded
        assert (Hp, Wp) == (H + sum(plan.pad_rows), W + sum(plan.pad_cols)) and Hp % 32 == 0 and Wp % 32 == 0
        wh, ww = plan.window
        assert (wh, ww) == (min(Hp, tile + 2 * halo), min(Wp, tile + 2 * halo)) and wh % 32 == 0 and ww % 32 == 0
        off, cores, dests = plan.offsets, plan.cores, plan.dests
        n = off.shape[0]
        assert off.dtype == cores.dtype == dests.dtype == np.int32 and cores.shape == (n, 4) and dests.shape == (n, 2) and n >= 1
        # one shape, whole multiples of 32, inside the padded scene
        assert (off % 32 == 0).all() and (off >= 0).all() and (off[:, 0] + wh <= Hp).all() and (off[:, 1] + ww <= Wp).all()
        # every pixel of the image belongs to exactly one core
        assert (coverage(plan, H, W) == 1).all(), (H, W, tile, halo)
        for (r, c), (y0, y1, x0, x1), (dr, dc) in zip(off.tolist(), cores.tolist(), dests.tolist()):
            if y1 <= y0 or x1 <= x0:
                continue
            assert 0 <= y0 and y1 <= wh and 0 <= x0 and x1 <= ww
            # the core sits where the image is: window + core offset - pad = destination
            assert (r + y0 - plan.pad_rows[0], c + x0 - plan.pad_cols[0]) == (dr, dc)
            # >= halo away from every window side that is not a border of the padded scene
            assert r == 0 or y0 >= halo
            assert r + wh == Hp or wh - y1 >= halo
            assert c == 0 or x0 >= halo
            assert c + ww == Wp or ww - x1 >= halo
        if Hp <= wh and Wp <= ww:
            assert n == 1 and off.tolist() == [[0, 0]]
            assert cores.tolist() == [[plan.pad_rows[0], plan.pad_rows[0] + H, plan.pad_cols[0], plan.pad_cols[0] + W]]


def test_plan_of_the_exactness_case():
    """790 x 500, tile 96, halo 320: nine shifted 736 x 512 windows over the 800 x 512 padded scene"""
    plan = sentinel2.scene_windows(790, 500, 96, 320)
    assert plan.padded == (800, 512) and plan.window == (736, 512)
    assert plan.offsets.tolist() == [[0, 0]] * 4 + [[64, 0]] * 5


def test_default_plan_of_a_sentinel2_tile():
    plan = sentinel2.scene_windows(10980, 10980, tile=1024)
    assert plan.padded == (11008, 11008) and plan.window == (1664, 1664) and plan.offsets.shape[0] == 121
    assert sentinel2.SCENE_BATCH_PIXELS // (1664 * 1664) == 1
    plan = sentinel2.scene_windows(10980, 10980)            # the default tile: the faster of the two measured ones
    assert sentinel2.SCENE_TILE == 2048 and plan.window == (2688, 2688) and plan.offsets.shape[0] == 36


@pytest.mark.parametrize("kw", [dict(tile=100), dict(tile=0), dict(tile=-32), dict(halo=16), dict(halo=-32)], ids=str)
def test_plan_argument_errors(kw):
    with pytest.raises(ValueError, match="multiple of 32"):
        sentinel2.scene_windows(64, 64, **kw)


def test_pad_not_below_the_image():
    with pytest.raises(ValueError, match="larger than the pad"):
        sentinel2.scene_windows(10, 64)          # 10 rows -> pads (11, 11)
    with pytest.raises(ValueError, match="larger than the pad"):
        sentinel2.scene_windows(64, 10)


def test_predict_scene_argument_errors():
    model = sentinel2.CDModel(device=torch.device("cpu"))
    bands = np.zeros((13, 40, 45), dtype=np.float32)
    with pytest.raises(AssertionError, match="Expected 13 channels found 12"):
        model.predict_scene(bands[:12])
    with pytest.raises(TypeError, match="uint16 or float32"):
        model.predict_scene(bands.astype(np.int32))
    with pytest.raises(TypeError, match="uint16 or float32"):
        model.predict_scene(torch.zeros(13, 40, 45, dtype=torch.int32))
    with pytest.raises(ValueError, match="multiple of 32"):
        model.predict_scene(bands, tile=100)
    with pytest.raises(ValueError, match="larger than the pad"):
        model.predict_scene(bands[:, :10])
    with pytest.raises(StarcopHipError):         # a CPU model: no fallback
        model.predict_scene(bands)
    with pytest.raises(StarcopHipError):
        model.predict_scene(bands.astype(np.uint16))


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof / offsetof of sc_scene_win and sc_scene_args as gcc lays them out == the ctypes mirrors; a plan's table rows are sc_scene_win"""
    import ctypes
    import os
    import shutil
    import subprocess
    from starcop_amd import _lib
    plan = sentinel2.scene_windows(150, 217, 64, 32)
    tab = sentinel2.scene_table(plan)
    assert tab.dtype == np.int32 and tab.flags.c_contiguous and tab.shape == (12, 8) and tab.strides[0] == ctypes.sizeof(_lib.sc_scene_win) == 32
    assert [f[0] for f in _lib.sc_scene_win._fields_] == ["row_off", "col_off", "core_y0", "core_y1", "core_x0", "core_x1", "dst_row", "dst_col"]
    assert tab[5].tolist() == plan.offsets[5].tolist() + plan.cores[5].tolist() + plan.dests[5].tolist()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sc_scene_win), offsetof(sc_scene_win, dst_row), sizeof(sc_scene_args), '
                   'offsetof(sc_scene_args, chan_stride), offsetof(sc_scene_args, pad_top), offsetof(sc_scene_args, scale), '
                   'offsetof(sc_scene_args, win), offsetof(sc_scene_args, out));return 0;}\n')
    exe = tmp_path / "sz"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    a = _lib.sc_scene_args
    assert got == [32, _lib.sc_scene_win.dst_row.offset, ctypes.sizeof(a), a.chan_stride.offset, a.pad_top.offset, a.scale.offset,
                   a.win.offset, a.out.offset]


def test_moved_names_are_the_scene_module_s():
    """sentinel2 / pipeline re-export the window machinery of starcop_amd.scene: the same objects, not copies"""
    from starcop_amd import pipeline, scene
    moved = [name for name in sentinel2.__all__ if hasattr(scene, name)]
    assert set(moved) >= {"RECEPTIVE_HALO", "SCENE_TILE", "ScenePlan", "scene_windows", "scene_table", "scene_gather", "scene_gather_planes",
                          "scene_core_counts", "float_bits"}
    for name in moved:
        assert getattr(sentinel2, name) is getattr(scene, name), name
    assert sentinel2.SCENE_BATCH_PIXELS is scene.SCENE_BATCH_PIXELS
    assert pipeline.RECEPTIVE_HALO is scene.RECEPTIVE_HALO


def test_window_batches():
    from starcop_amd import scene
    cpu = torch.device("cpu")
    got = list(scene.window_batches(5, (64, 96), 3, cpu, batch=2))
    assert [(first, k) for first, k, _ in got] == [(0, 2), (2, 2), (4, 1)]
    for _, k, buf in got:
        assert buf.shape == (k, 3, 64, 96) and buf.dtype == torch.float32 and buf.device == cpu
    assert got[0][2] is got[1][2] and got[2][2] is not got[0][2]
    # batch=None: the most windows below SCENE_BATCH_PIXELS, clamped to [1, n]
    per = scene.SCENE_BATCH_PIXELS // (64 * 96)
    assert per > 5 and [(f, k) for f, k, _ in scene.window_batches(5, (64, 96), 1, cpu)] == [(0, 5)]
    assert [(f, k) for f, k, _ in scene.window_batches(per + 3, (64, 96), 1, cpu)] == [(0, per), (per, 3)]
    big = (4096, 2048)                              # one window above the pixel budget: still one per batch
    assert scene.SCENE_BATCH_PIXELS // (big[0] * big[1]) == 0
    assert [(f, k) for f, k, _ in scene.window_batches(2, big, 1, torch.device("meta"))] == [(0, 1), (1, 1)]
    assert [(f, k) for f, k, _ in scene.window_batches(3, (32, 32), 1, cpu, batch=0)] == [(0, 1), (1, 1), (2, 1)]
    assert [(f, k) for f, k, _ in scene.window_batches(3, (32, 32), 1, cpu, batch=99)] == [(0, 3)]


def test_table_rows():
    import ctypes
    from starcop_amd import _lib, scene
    host = scene.scene_table(scene.scene_windows(150, 217, 64, 32))         # (12, 8)
    dev = torch.from_numpy(host.copy())
    bad = [(dev.to(torch.int64), host, 0, 1), (torch.from_numpy(np.zeros((12, 16), np.int32))[:, ::2], host, 0, 1),
           (dev[:, :7].contiguous(), np.ascontiguousarray(host[:, :7]), 0, 1), (dev, host[:11], 0, 1), (dev, host, -1, 1), (dev, host, 8, 5),
           (dev, host.astype(np.int64), 0, 1), (dev, host, 0, 0)]
    for who in ("scene_gather", "predict_masks_into"):
        for args in bad:
            with pytest.raises(ValueError, match=f"^{who}: the table must be"):
                scene.table_rows(who, *args)
    row = ctypes.sizeof(_lib.sc_scene_win)
    for first, n in ((0, 12), (5, 7), (11, 1)):
        assert scene.table_rows("t", dev, host, first, n) == (dev.data_ptr() + first * row, host.ctypes.data + first * row)


def test_scene_module_imports_nothing_above_it():
    """scene.py sits below network / model_module / pipeline / sentinel2 (they import it), and model_module imports it at module level"""
    import ast
    import inspect
    from starcop_amd import model_module, scene

    def imported(tree):
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom):
                yield from ([node.module] if node.module else [a.name for a in node.names])
            elif isinstance(node, ast.Import):
                yield from (a.name.split(".")[-1] for a in node.names)
    assert not {"network", "model_module", "pipeline", "sentinel2"} & set(imported(ast.parse(inspect.getsource(scene))))
    mm = ast.parse(inspect.getsource(model_module))
    assert "scene" in set(imported(ast.Module(body=[n for n in mm.body if isinstance(n, (ast.Import, ast.ImportFrom))], type_ignores=[])))
    assert "sentinel2" not in set(imported(mm))
