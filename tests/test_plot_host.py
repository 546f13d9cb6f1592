"""Host side of the validation panels (starcop_amd/plot.py, io_formats.write_png): the shipped viridis table, the registry, the
tensor selection of plot_batch, mask_to_rgb on numpy and the PNG writer.  No GPU, and neither matplotlib nor PIL is required:
the expectations are recorded in tests/golden/g15_panels.npz (tests/golden/make_golden_panels.py)."""
import ctypes
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import plot_util as pu
from starcop_amd import _lib, io_formats, plot

CONFIG_PRODUCTS = ["rgb_aviris", "mag1c", "label", "pred"]                 # products_plot of the reference's config.yaml (+ differences)
INPUTS = ["mag1c", "TOA_AVIRIS_640nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_460nm"]


@pytest.fixture(scope="module")
def golden():
    return np.load(pu.GOLDEN)


def test_shipped_viridis_table_is_the_fixtures(golden):
    assert np.array_equal(plot.viridis8(), golden["viridis8"])
    assert plot.viridis8().dtype == np.uint8 and plot.viridis8().shape == (256, 3)


def test_registry_keys_and_fields(golden):
    want = json.loads(str(golden["registry"]))
    assert list(plot.PLOTTING_FUNCTIONS) == [k for k, _, _ in want]
    for key, products, tensor in want:
        entry = plot.PLOTTING_FUNCTIONS[key]
        assert entry.get("input_products") == products and entry["tensor"] == tensor, key
        assert set(entry) <= {"input_products", "tensor", "kind", "vmin", "vmax"} and entry["kind"] in ("band", "rgb", "categorical")
    reg = plot.PLOTTING_FUNCTIONS
    assert reg["pred_binary"]["tensor"] == "prediction"                                    # the reference's quirks stay
    assert all(reg[k]["input_products"] == ["TOA_S2B_B1"] for k in ("s2_b1", "s2_b2", "s2_b3", "s2_b4"))
    assert (reg["mag1c"]["vmin"], reg["mag1c"]["vmax"]) == (0, 2) and (reg["label"]["vmin"], reg["label"]["vmax"]) == (0, 1)
    assert reg["wv3_b3"]["vmin"] is None and reg["rgb_aviris"]["kind"] == "rgb" and reg["differences"]["kind"] == "categorical"
    assert np.array_equal(np.round(plot.COLORS_DIFFERENCES * 255), [[0, 0, 0], [255, 0, 0], [220, 220, 0], [0, 200, 0]])
    assert plot.INTERPRETATION_DIFFERENCES == ["correct no-plume", "false plume", "false no-plume", "correct plume"]


def _batch(B=2, H=6, W=5):
    g = torch.Generator().manual_seed(0)
    return {"input": torch.rand(B, 4, H, W, generator=g), "input_norm": torch.rand(B, 4, H, W, generator=g),
            "output_norm": torch.rand(B, 1, H, W, generator=g), "prediction": torch.rand(B, 1, H, W, generator=g),
            "differences": torch.zeros(B, 1, H, W, dtype=torch.int64)}


def test_select_panels_config_products():
    b = _batch()
    specs = plot.select_panels(b, INPUTS, CONFIG_PRODUCTS)
    assert [s.name for s in specs] == CONFIG_PRODUCTS
    rgb, mag, lab, pred = specs
    # channels are picked in the order of input_products (640, 550, 460 nm = r, g, b), not of the registry entry
    assert (rgb.kind, rgb.key, rgb.channels, rgb.autoscale) == ("rgb", "input_norm", (1, 2, 3), False)
    assert torch.equal(rgb.tensor, b["input_norm"][:, 1:4])
    assert (mag.kind, mag.key, mag.channels, mag.vmin, mag.vmax, mag.div, mag.autoscale) == ("band", "input_norm", (0,), 0, 2, 1.0, False)
    assert torch.equal(mag.tensor, b["input_norm"][:, 0:1])
    assert (lab.key, lab.channels, lab.vmin, lab.vmax) == ("output_norm", None, 0, 1) and lab.tensor is b["output_norm"]
    assert (pred.key, pred.vmin, pred.vmax) == ("prediction", 0, 1) and pred.tensor is b["prediction"]
    d = plot.select_panels(b, INPUTS, ["differences", "pred_binary"])
    assert d[0].kind == "categorical" and [c for _, c in d[0].categories] == [(0, 0, 0), (255, 0, 0), (220, 220, 0), (0, 200, 0)]
    assert [v for v, _ in d[0].categories] == [0.0, 1.0, 2.0, 3.0]
    assert d[1].key == "prediction"


def test_select_panels_outside_the_registry_and_batch_keys():
    b = _batch()
    s, = plot.select_panels(b, INPUTS, ["TOA_AVIRIS_550nm"])                  # not registered: its channel of input_norm
    assert (s.kind, s.key, s.channels, s.autoscale, s.vmin) == ("band", "input_norm", (2,), True, None)
    assert torch.equal(s.tensor, b["input_norm"][:, 2])
    b["albedo"] = torch.rand(2, 1, 6, 5)
    s, = plot.select_panels(b, INPUTS, ["albedo"])                            # not registered, but a batch key
    assert (s.key, s.channels, s.autoscale, s.div) == ("albedo", None, True, 1.0) and s.tensor is b["albedo"]
    # mag1c delivered under its own key (an extra product of the plotting datasets): raw ppm*m, divided by 1750
    b["mag1c"] = torch.rand(2, 1, 6, 5) * 1750
    s, = plot.select_panels(b, ["TOA_AVIRIS_640nm"], ["mag1c"])
    assert (s.key, s.div, s.vmin, s.vmax, s.autoscale) == ("mag1c", 1750.0, 0, 2, False) and s.tensor is b["mag1c"]
    b["rgb_aviris"] = torch.rand(2, 3, 6, 5)
    s, = plot.select_panels(b, ["mag1c"], ["rgb_aviris"])
    assert (s.kind, s.key, s.channels) == ("rgb", "rgb_aviris", None) and s.tensor is b["rgb_aviris"]
    s, = plot.select_panels(_batch(), ["TOA_WV3_SWIR3", "mag1c"], ["wv3_b3"])  # registered without limits: autoscale
    assert (s.key, s.channels, s.autoscale) == ("input_norm", (0,), True)


def test_select_panels_from_the_keys_of_the_input_products():
    """the three bands of rgb_aviris delivered under their own keys: stacked as channels in the registry entry's order
    (460, 550, 640 nm, as the reference's cat would order them), whatever input_products says"""
    b = _batch()
    names = plot.PLOTTING_FUNCTIONS["rgb_aviris"]["input_products"]
    assert names == ["TOA_AVIRIS_460nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_640nm"]
    for k, name in enumerate(names):
        b[name] = torch.full((2, 1, 6, 5), float(k))
    s, = plot.select_panels(b, ["mag1c"], ["rgb_aviris"])
    assert (s.kind, s.key, s.channels, s.autoscale) == ("rgb", tuple(names), None, False)
    assert s.tensor.shape == (2, 3, 6, 5) and all(bool((s.tensor[:, k] == k).all()) for k in range(3))
    for k, name in enumerate(names):                                         # (B, H, W) planes stack the same way
        b[name] = torch.full((2, 6, 5), float(k))
    s, = plot.select_panels(b, ["mag1c"], ["rgb_aviris"])
    assert s.tensor.shape == (2, 3, 6, 5) and all(bool((s.tensor[:, k] == k).all()) for k in range(3))
    del b[names[1]]                                                          # one key missing: back to the channels of input_norm
    s, = plot.select_panels(b, INPUTS, ["rgb_aviris"])
    assert (s.key, s.channels) == ("input_norm", (1, 2, 3))


class _FakeDevicePlane:
    """stands in for a tensor on a GPU where there is none: _check_planes looks at is_cuda and device only"""
    is_cuda = True

    def __init__(self, index=0):
        self.device = torch.device("cuda", index)


def test_planes_off_the_device_raise_before_any_address_is_taken(monkeypatch):
    def reached(*a, **k):
        raise AssertionError("_layout was reached")
    monkeypatch.setattr(plot, "_layout", reached)
    on0 = plot.PanelSpec("mag1c", "band", [_FakeDevicePlane(0)])
    with pytest.raises(_lib.StarcopHipError, match=r"panel 'label' of batch item 0 is on cpu"):        # a CPU tensor in the second column
        plot._render([[on0, plot.PanelSpec("label", "band", [torch.zeros(4, 4)])]], 512, 4)
    with pytest.raises(_lib.StarcopHipError, match=r"panel 'rgb' of batch item 1 is on cpu"):          # ... in the last plane of a later row
        plot._render([[on0], [plot.PanelSpec("rgb", "rgb", [_FakeDevicePlane(0), _FakeDevicePlane(0), torch.zeros(4, 4)])]], 512, 4)
    with pytest.raises(_lib.StarcopHipError, match=r"panel 'pred' of batch item 0 is on cuda:1, the figure's first panel on cuda:0"):
        plot._render([[on0, plot.PanelSpec("pred", "band", [_FakeDevicePlane(1)])]], 512, 4)
    with pytest.raises(_lib.StarcopHipError, match=r"panel 'x' of batch item 0 is on (cpu|ndarray)"):
        plot._render([[on0, plot.PanelSpec("x", "band", [np.zeros((4, 4), np.float32)])]], 512, 4)
    b = _batch()
    b["albedo"] = np.zeros((2, 1, 6, 5), np.float32)                         # a numpy extra product (to_device leaves it alone)
    with pytest.raises(_lib.StarcopHipError, match="panel 'albedo' is a ndarray, not a tensor"):
        plot.render_batch(b, INPUTS, ["mag1c", "albedo"])
    with pytest.raises(_lib.StarcopHipError, match="is on cpu"):
        plot.render_batch(_batch(), INPUTS, ["mag1c", "label"])


def test_select_panels_raises_the_references_messages():
    b = _batch()
    with pytest.raises(AssertionError, match=r"nope not registered in dict_keys\(\[.*\]\) and not in \['mag1c'"):
        plot.select_panels(b, INPUTS, ["nope"])
    with pytest.raises(AssertionError, match="Unexpected number of products"):
        plot.select_panels(b, ["mag1c", "TOA_AVIRIS_640nm"], ["rgb_aviris"])
    del b["prediction"]
    with pytest.raises(AssertionError, match=r"Batch does not have keys: pred prediction\. Keys in batch: dict_keys"):
        plot.select_panels(b, INPUTS, ["pred"])


def test_mask_to_rgb_numpy():
    rng = np.random.default_rng(3)
    mask = rng.integers(0, 5, size=(9, 7))
    got = plot.mask_to_rgb(mask, [0, 1, 2, 3], plot.COLORS_DIFFERENCES)
    assert got.shape == (9, 7, 3) and got.dtype == np.uint8
    assert np.array_equal(got, pu.cat_bytes(mask, plot._DIFF_CATEGORIES))
    assert not got[mask == 4].any()                                           # no match: black
    rgba = np.array([[1, 0, 0, 1], [0, 0.5, 0, 0.25], [0, 0, 1, 0.5]])
    got = plot.mask_to_rgb(torch.from_numpy(mask), [1, 2, 1], rgba)           # a repeated value: the last entry wins
    assert got.shape == (9, 7, 4)
    assert (got[mask == 1] == [0, 0, 255, 128]).all() and (got[mask == 2] == [0, 128, 0, 64]).all() and not got[mask == 0].any()
    with pytest.raises(AssertionError, match="Values and colors should have same length 2 4"):
        plot.mask_to_rgb(mask, [0, 1], plot.COLORS_DIFFERENCES)
    with pytest.raises(AssertionError, match="Expected only 2D array found"):
        plot.mask_to_rgb(mask[None], [0, 1, 2, 3], plot.COLORS_DIFFERENCES)


def test_write_png_decodes(tmp_path):
    rng = np.random.default_rng(4)
    Hc, Wc = 19, 23
    img = rng.integers(0, 256, size=(Hc, Wc, 3), dtype=np.uint8)
    lines = np.concatenate([np.zeros((Hc, 1), np.uint8), img.reshape(Hc, -1)], axis=1)
    meta = {"names": ["mag1c", "label"], "ranges": [[0.0, 2.0], None]}
    path = tmp_path / "a.png"
    io_formats.write_png(path, lines, Wc, Hc, text=json.dumps(meta))
    w, h, got, text = pu.decode_png(path)
    assert (w, h) == (Wc, Hc) and np.array_equal(got, img) and pu.png_comment(text) == meta
    io_formats.write_png(path, lines.reshape(-1), Wc, Hc)                     # flat buffer, no text
    assert pu.decode_png(path)[3] == {} and np.array_equal(pu.decode_png(path)[2], img)
    if importlib.util.find_spec("PIL") is not None:
        from PIL import Image
        io_formats.write_png(path, lines, Wc, Hc, text=json.dumps(meta))
        with Image.open(path) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), img) and json.loads(im.text["Comment"]) == meta
    with pytest.raises(ValueError, match="scanlines"):
        io_formats.write_png(path, lines[:, :-1], Wc, Hc)
    lines[3, 0] = 1
    with pytest.raises(ValueError, match="filter byte"):
        io_formats.write_png(path, lines, Wc, Hc)


def test_restatement_matches_the_fixture(golden):
    """tests/plot_util.py (what the GPU tests compare the kernel with) gives matplotlib's recorded bytes"""
    x = golden["plane"]
    fin = np.isfinite(x)
    assert (~fin).sum() == 5
    for k, (lo, hi) in enumerate(golden["ranges"]):
        got = pu.band_bytes(x, lo, hi)
        assert np.array_equal(got[fin], golden[f"band_{k}"][fin]) and (got[~fin] == 255).all(), (lo, hi)
    assert np.array_equal(pu.rgb_bytes(*golden["rgb_planes"]), golden["rgb"])
    lo, hi = pu.finite_minmax(x)
    assert (float(lo), float(hi)) == tuple(golden["ranges"][3])


def test_fixture_is_what_matplotlib_gives(golden):
    if importlib.util.find_spec("matplotlib") is None:
        pytest.skip("matplotlib is not installed: the recorded expectations stand")
    sys.path.insert(0, os.path.join(pu.ROOT, "tests", "golden"))
    try:
        import make_golden_panels as mk
    finally:
        sys.path.pop(0)
    x, rgb = mk.planes()
    assert np.array_equal(x, golden["plane"], equal_nan=True) and np.array_equal(rgb, golden["rgb_planes"])
    for k, v in mk.expectations().items():
        assert np.array_equal(v, golden[k]), k


def test_sc_panel_layout_matches_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sc_panel), offsetof(sc_panel, row_stride), offsetof(sc_panel, scale), '
                   'offsetof(sc_panel, autoscale), offsetof(sc_panel, vmin), offsetof(sc_panel, cat_value), offsetof(sc_panel, cat_rgb));'
                   'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(pu.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    p = _lib.sc_panel
    assert got == [ctypes.sizeof(p), p.row_stride.offset, p.scale.offset, p.autoscale.offset, p.vmin.offset, p.cat_value.offset,
                   p.cat_rgb.offset]
    assert (_lib.PANEL_MAX, _lib.PANEL_MAX_CAT) == (1024, 8)


def test_render_needs_a_device():
    """no fall-back: without a GPU render_batch raises instead of drawing on the host"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.StarcopHipError):
        plot.render_batch(_batch(), INPUTS, ["mag1c"])
