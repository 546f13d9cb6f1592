"""Validation panels on the GPU (starcop_amd/csrc/panels.hip, starcop_amd/plot.py): sc_render_panels and sc_panel_minmax against
the numpy restatement of the per-pixel contract (tests/plot_util.py) and against matplotlib's recorded bytes
(tests/golden/g15_panels.npz), byte for byte; the argument checks; run_validation's images/ folder; ImageLogger."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import plot_util as pu  # noqa: E402
from starcop_amd import _lib, baselines, data_logger, plot, validation  # noqa: E402
from starcop_amd._lib import (PANEL_BAND, PANEL_CATEGORICAL, PANEL_F32, PANEL_I64, PANEL_RGB, PANEL_U8)  # noqa: E402

DEV = "cuda"
GUARD = 64                      # bytes in front of and behind the canvas that must keep their fill
FILL = 0xA5
CATS = plot._DIFF_CATEGORIES
DTYPES = {torch.float32: PANEL_F32, torch.int64: PANEL_I64, torch.uint8: PANEL_U8}


def _fill(t, planes, kind, scale, y, x, vmin=0.0, vmax=1.0, autoscale=0, div=1.0, cats=(), dtype=None):
    for c, pl in enumerate(planes):
        assert pl.stride(1) == 1
        t.src[c] = pl.data_ptr()
    t.row_stride, t.dtype, t.kind = planes[0].stride(0), DTYPES[planes[0].dtype] if dtype is None else dtype, kind
    t.H, t.W, t.scale, t.dst_y, t.dst_x = planes[0].shape[0], planes[0].shape[1], scale, y, x
    t.autoscale, t.vmin, t.vmax, t.div, t.n_cat = autoscale, vmin, vmax, div, len(cats)
    for k, (v, rgb) in enumerate(cats):
        t.cat_value[k] = v
        for j in range(3):
            t.cat_rgb[k][j] = rgb[j]


def _launch(hip, table, Hc, Wc, minmax=True, shift=0):
    """(scanlines (Hc, 1 + 3 Wc), minmax (n, 2)) of one sc_panel_minmax + sc_render_panels; the canvas is pre-filled with 0xA5 and
    sits between two guard zones that must keep that fill; ``shift`` moves its first byte off the 4-byte boundary"""
    n = len(table)
    dev_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    size = Hc * (1 + 3 * Wc)
    buf = torch.full((size + 2 * GUARD + shift,), FILL, dtype=torch.uint8, device=DEV)
    mm = torch.full((n, 2), -7.0, dtype=torch.float32, device=DEV)
    if minmax:
        _lib.check(hip.sc_panel_minmax(dev_table.data_ptr(), table, n, mm.data_ptr(), _lib.stream()))
    _lib.check(hip.sc_render_panels(dev_table.data_ptr(), table, n, mm.data_ptr(), buf.data_ptr() + GUARD + shift, Hc, Wc, _lib.stream()))
    host = buf.cpu().numpy()
    assert (host[:GUARD + shift] == FILL).all() and (host[-GUARD:] == FILL).all(), "wrote outside the canvas"
    return host[GUARD + shift:-GUARD].reshape(Hc, 1 + 3 * Wc), mm.cpu().numpy()


def _assert_same(got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{len(bad)} bytes differ, first at row {bad[0][0]} byte {bad[0][1]}: got {got[tuple(bad[0])]}, "
                             f"want {want[tuple(bad[0])]}")


def _five_panel_inputs(rng, B, H, W):
    """per batch item: float32 band (strided, raw ppm*m), float32 rgb, int64 band, int64 categorical (strided), uint8 band"""
    mag = rng.normal(600, 900, size=(B, 2, H, W + 7)).astype(np.float32)
    mag[:, 1, 0, 3:8] = [np.nan, np.inf, -np.inf, 0.0, 3500.0]
    rgb = rng.uniform(-0.2, 1.2, size=(B, 3, H, W)).astype(np.float32)
    rgb[:, 1, 1, :3] = [np.nan, np.inf, -np.inf]
    rgb[:, :, 2, :2] = np.array([0.0, 1.0], np.float32)
    lab = rng.integers(-1, 3, size=(B, 1, H, W)).astype(np.int64)
    dif = rng.integers(0, 5, size=(B, H, W + 3)).astype(np.int64)
    u8 = rng.integers(3, 250, size=(B, H, W)).astype(np.uint8)
    return [torch.from_numpy(a).to(DEV) for a in (mag, rgb, lab, dif, u8)], (mag, rgb, lab, dif, u8)


@pytest.mark.parametrize("H,W,scale,shift", [(37, 53, 1, 0), (37, 53, 3, 0), (64, 96, 2, 0), (5, 700, 2, 0), (3, 1030, 1, 0),
                                             (37, 53, 3, 1), (9, 40, 1, 2), (9, 40, 1, 3)])
def test_render_matches_restatement(hip, H, W, scale, shift):
    """batch of 2 x five panels: float32, int64 and uint8 sources, all three kinds, non-contiguous rows; two shapes are wider
    than one 1024-pixel chunk of the kernel; with ``shift`` the canvas itself starts 1, 2 or 3 bytes past a 4-byte boundary
    (torch allocations never do; a caller's buffer may)"""
    rng = np.random.default_rng(H * 1000 + W + scale)
    B, gap = 2, 5
    dev, (mag, rgb, lab, dif, u8) = _five_panel_inputs(rng, B, H, W)
    ph, pw = H * scale, W * scale
    Hc, Wc = B * ph + gap + 3, 5 * pw + 4 * gap + 2                  # a margin below and to the right as well
    table = (_lib.sc_panel * (5 * B))()
    want = []
    for b in range(B):
        y, xs = b * (ph + gap), [p * (pw + gap) for p in range(5)]
        m = dev[0][b, 1, :, 3:3 + W]
        auto = b == 1                                                 # row 1 draws the band with its own range
        _fill(table[5 * b + 0], [m], PANEL_BAND, scale, y, xs[0], 0.0, 2.0, autoscale=int(auto), div=1750.0)
        _fill(table[5 * b + 1], [dev[1][b, c] for c in range(3)], PANEL_RGB, scale, y, xs[1])
        _fill(table[5 * b + 2], [dev[2][b, 0]], PANEL_BAND, scale, y, xs[2], 0.0, 1.0)
        _fill(table[5 * b + 3], [dev[3][b, :, 2:2 + W]], PANEL_CATEGORICAL, scale, y, xs[3], cats=CATS)
        _fill(table[5 * b + 4], [dev[4][b]], PANEL_BAND, scale, y, xs[4], autoscale=1)
        mm = mag[b, 1, :, 3:3 + W]
        r0 = pu.finite_minmax(mm, 1750.0) if auto else (0.0, 2.0)
        want += [(pu.band_bytes(mm, *r0, div=1750.0), scale, y, xs[0]), (pu.rgb_bytes(*rgb[b]), scale, y, xs[1]),
                 (pu.band_bytes(lab[b, 0], 0.0, 1.0), scale, y, xs[2]), (pu.cat_bytes(dif[b, :, 2:2 + W], CATS), scale, y, xs[3]),
                 (pu.band_bytes(u8[b], *pu.finite_minmax(u8[b])), scale, y, xs[4])]
    assert not dev[0][0, 1, :, 3:3 + W].is_contiguous() and not dev[3][0, :, 2:2 + W].is_contiguous()
    got, ranges = _launch(hip, table, Hc, Wc, shift=shift)
    _assert_same(got, pu.compose(want, Hc, Wc))
    assert tuple(ranges[0]) == (0.0, 2.0) and tuple(ranges[5]) == tuple(pu.finite_minmax(mag[1, 1, :, 3:3 + W], 1750.0))
    assert tuple(ranges[4]) == (float(u8[0].min()), float(u8[0].max()))


def test_render_512_figure_at_scale_1(hip):
    """the flagship figure: rgb, mag1c, label, differences of one 512 x 512 tile; several work-groups per panel"""
    rng = np.random.default_rng(512)
    S, gap = 512, 4
    x = np.concatenate([np.abs(rng.normal(0, 0.4, size=(1, S, S))), rng.uniform(0, 1.1, size=(3, S, S))]).astype(np.float32)
    lab = (rng.uniform(size=(S, S)) < 0.2).astype(np.float32)
    dif = rng.integers(0, 4, size=(S, S)).astype(np.int64)
    xd, ld, dd = (torch.from_numpy(a).to(DEV) for a in (x, lab, dif))
    Hc, Wc = S, 4 * S + 3 * gap
    table = (_lib.sc_panel * 4)()
    xs = [p * (S + gap) for p in range(4)]
    _fill(table[0], [xd[1], xd[2], xd[3]], PANEL_RGB, 1, 0, xs[0])
    _fill(table[1], [xd[0]], PANEL_BAND, 1, 0, xs[1], 0.0, 2.0)
    _fill(table[2], [ld], PANEL_BAND, 1, 0, xs[2], 0.0, 1.0)
    _fill(table[3], [dd], PANEL_CATEGORICAL, 1, 0, xs[3], cats=CATS)
    got, _ = _launch(hip, table, Hc, Wc)
    want = [(pu.rgb_bytes(x[1], x[2], x[3]), 1, 0, xs[0]), (pu.band_bytes(x[0], 0, 2), 1, 0, xs[1]),
            (pu.band_bytes(lab, 0, 1), 1, 0, xs[2]), (pu.cat_bytes(dif, CATS), 1, 0, xs[3])]
    _assert_same(got, pu.compose(want, Hc, Wc))


def test_fixture_planes_give_matplotlibs_bytes(hip):
    g = np.load(pu.GOLDEN)
    x, rgb = g["plane"], g["rgb_planes"]
    H, W = x.shape
    xd, rd = torch.from_numpy(x).to(DEV), torch.from_numpy(rgb).to(DEV)
    gap = 3
    table = (_lib.sc_panel * 5)()
    xs = [p * (W + gap) for p in range(5)]
    for k, (lo, hi) in enumerate(g["ranges"]):
        _fill(table[k], [xd], PANEL_BAND, 1, 0, xs[k], float(lo), float(hi), autoscale=int(k == 3))   # the last range is the plane's own
    _fill(table[4], [rd[0], rd[1], rd[2]], PANEL_RGB, 1, 0, xs[4])
    got, ranges = _launch(hip, table, H, 5 * W + 4 * gap)
    img = got[:, 1:].reshape(H, -1, 3)
    fin = np.isfinite(x)
    for k in range(4):
        panel = img[:, xs[k]:xs[k] + W]
        assert np.array_equal(panel[fin], g[f"band_{k}"][fin]), k
        assert (panel[~fin] == 255).all(), k
    assert tuple(ranges[3]) == tuple(g["ranges"][3])
    assert np.array_equal(img[:, xs[4]:xs[4] + W], g["rgb"])


def test_panel_minmax(hip):
    rng = np.random.default_rng(6)
    H, W = 67, 131
    a = rng.normal(0, 3, size=(H, W + 5)).astype(np.float32)
    a[0, :4] = [np.nan, np.inf, -np.inf, 100.0]                       # the infinities are not part of the range
    const = np.full((H, W), 0.75, np.float32)
    nans = np.full((H, W), np.nan, np.float32)
    nans[3, 3] = np.inf
    i64 = rng.integers(-50, 50, size=(H, W)).astype(np.int64)
    dev = [torch.from_numpy(v).to(DEV) for v in (a, const, nans, i64)]
    table = (_lib.sc_panel * 5)()
    xs = [p * (W + 2) for p in range(5)]
    _fill(table[0], [dev[0][:, 2:2 + W]], PANEL_BAND, 1, 0, xs[0], autoscale=1)
    _fill(table[1], [dev[1]], PANEL_BAND, 1, 0, xs[1], autoscale=1)
    _fill(table[2], [dev[2]], PANEL_BAND, 1, 0, xs[2], autoscale=1)
    _fill(table[3], [dev[3]], PANEL_BAND, 1, 0, xs[3], autoscale=1, div=4.0)
    _fill(table[4], [dev[1]], PANEL_BAND, 1, 0, xs[4], 0.25, 3.0)      # not flagged: the descriptor's limits
    got, mm = _launch(hip, table, H, 5 * W + 8)
    sub = a[:, 2:2 + W]
    fin = sub[np.isfinite(sub)]
    assert tuple(mm[0]) == (fin.min(), fin.max()) and mm[0, 1] == 100.0
    assert tuple(mm[1]) == (0.75, 0.75) and tuple(mm[2]) == (0.0, 1.0)
    assert tuple(mm[3]) == (np.float32(i64.min()) / np.float32(4), np.float32(i64.max()) / np.float32(4))
    assert tuple(mm[4]) == (0.25, 3.0)
    img = got[:, 1:].reshape(H, -1, 3)
    assert (img[:, xs[1]:xs[1] + W] == pu.viridis8()[0]).all()          # a constant plane: index 0
    assert (img[:, xs[2]:xs[2] + W] == 255).all()                       # nothing finite: white
    want = [(pu.band_bytes(sub, *mm[0]), 1, 0, xs[0]), (pu.band_bytes(const, 0.75, 0.75), 1, 0, xs[1]),
            (pu.band_bytes(nans, 0, 1), 1, 0, xs[2]), (pu.band_bytes(i64, *mm[3], div=4.0), 1, 0, xs[3]),
            (pu.band_bytes(const, 0.25, 3.0), 1, 0, xs[4])]
    _assert_same(got, pu.compose(want, H, 5 * W + 8))


def test_argument_checks_launch_nothing(hip):
    H, W = 8, 12
    a = torch.rand(H, W, device=DEV)
    Hc, Wc = 10, 30
    canvas = torch.full((Hc * (1 + 3 * Wc),), FILL, dtype=torch.uint8, device=DEV)
    mm = torch.zeros((2, 2), device=DEV)

    def table(second_x=15, scale=1, dtype=None, y=0):
        t = (_lib.sc_panel * 2)()
        _fill(t[0], [a], PANEL_BAND, 1, 0, 0)
        _fill(t[1], [a], PANEL_BAND, scale, y, second_x, dtype=dtype)
        return t

    def render(t):
        d = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(DEV)
        _lib.check(hip.sc_render_panels(d.data_ptr(), t, 2, mm.data_ptr(), canvas.data_ptr(), Hc, Wc, _lib.stream()))

    with pytest.raises(ValueError, match="overlap"):
        render(table(second_x=11))
    with pytest.raises(ValueError, match="leaves the 10 x 30 canvas"):
        render(table(second_x=19))
    with pytest.raises(ValueError, match="leaves the 10 x 30 canvas"):
        render(table(y=3))
    with pytest.raises(ValueError, match="scale 0"):
        render(table(scale=0))
    with pytest.raises(ValueError, match="unknown dtype 7"):
        render(table(dtype=7))
    t = table()
    t[1].kind = 9
    with pytest.raises(ValueError, match="unknown kind 9"):
        render(t)
    t = table()
    d = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(DEV)
    with pytest.raises(ValueError, match="n_panels=0"):
        _lib.check(hip.sc_render_panels(d.data_ptr(), t, 0, mm.data_ptr(), canvas.data_ptr(), Hc, Wc, _lib.stream()))
    with pytest.raises(ValueError, match="scale 0"):
        _lib.check(hip.sc_panel_minmax(d.data_ptr(), table(scale=0), 2, mm.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    assert (canvas.cpu().numpy() == FILL).all() and not mm.cpu().numpy().any()        # nothing was launched
    render(table())                                                                      # and the valid table draws
    assert (canvas.cpu().numpy() != FILL).any()


def test_a_plane_off_the_device_raises(hip):
    """a CPU tensor or a numpy array in a later column is an error, not an address handed to the kernel"""
    B, H, W = 2, 8, 8
    batch = {"input": torch.rand(B, 4, H, W, device=DEV), "input_norm": torch.rand(B, 4, H, W, device=DEV),
             "output_norm": torch.rand(B, 1, H, W)}                          # the label stayed on the host
    with pytest.raises(_lib.StarcopHipError, match="panel 'label' of batch item 0 is on cpu"):
        plot.render_batch(batch, PRODUCTS, ["mag1c", "label"])
    batch["albedo"] = np.zeros((B, 1, H, W), np.float32)
    with pytest.raises(_lib.StarcopHipError, match="panel 'albedo' is a ndarray"):
        plot.render_batch(batch, PRODUCTS, ["mag1c", "albedo"])
    assert plot.render_batch(batch, PRODUCTS, ["mag1c"]).image.shape == (2 * 512 + 4, 512, 3)        # the device part still draws


def test_mask_to_rgb_on_the_device(hip):
    rng = np.random.default_rng(8)
    mask = rng.integers(0, 5, size=(21, 34))
    md = torch.from_numpy(mask).to(DEV)
    assert np.array_equal(plot.mask_to_rgb(md, [0, 1, 2, 3], plot.COLORS_DIFFERENCES), plot.mask_to_rgb(mask, [0, 1, 2, 3], plot.COLORS_DIFFERENCES))
    rgba = np.array([[1, 0, 0, 1], [0, 0.5, 0, 0.25], [0, 0, 1, 0.5]])
    assert np.array_equal(plot.mask_to_rgb(md, [1, 2, 1], rgba), plot.mask_to_rgb(mask, [1, 2, 1], rgba))
    with pytest.raises(ValueError, match="9 values"):
        plot.mask_to_rgb(md, list(range(9)), np.zeros((9, 3)))


# ---- run_validation / ImageLogger ----------------------------------------------------------------------------------------------
PRODUCTS = ["mag1c", "TOA_AVIRIS_640nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_460nm"]
PRODUCTS_PLOT = ["mag1c", "label", "pred", "differences"]


def _tiles(rng, n_tiles, H=96, W=96):
    """tiles covering every (has_plume, difficulty) group of run_validation: none, a large (> 1000 px) and a small plume"""
    batches = []
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n_tiles):
        kind = i % 3
        mag = np.abs(rng.normal(0, 200, size=(H, W))).astype(np.float32)
        lab = np.zeros((H, W), np.float32)
        if kind:
            r = 30 if kind == 1 else 6
            cy, cx = rng.integers(r, H - r), rng.integers(r, W - r)
            blob = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
            lab[blob] = 1.0
            mag += 900.0 * np.roll(blob, (rng.integers(-3, 4), rng.integers(-3, 4)), (0, 1))
        if i == 0:
            mag[10:20, 10:25] += 800.0                 # false positives on a plume-free tile
        rgb = rng.uniform(5, 110, size=(3, H, W)).astype(np.float32)
        batches.append({"input": torch.from_numpy(np.concatenate([mag[None], rgb])[None]),
                        "output": torch.from_numpy(lab[None, None]), "id": [f"tile_{i:02d}"],
                        "has_plume": torch.tensor([int(kind != 0)])})
    return batches


def _same_metrics(a, b):
    assert list(a) == list(b)
    for k in a:
        if k == "thresholded":
            assert len(a[k]) == len(b[k])
            for u, v in zip(a[k], b[k]):
                _same_metrics(u, v)
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert np.array_equal(np.float64(a[k]), np.float64(b[k]), equal_nan=True), k


def test_run_validation_writes_the_panels(hip, tmp_path):
    batches = _tiles(np.random.default_rng(11), 7)
    model = baselines.Mag1cBaseline(PRODUCTS).to(DEV)
    thr = [200.0, 350.0, 500.0, 700.0, 1000.0]
    plain, plotted = tmp_path / "plain", tmp_path / "plotted"
    with np.errstate(all="ignore"):
        with warnings.catch_warnings(record=True) as rec_plain:
            warnings.simplefilter("always")
            df0, met0 = validation.run_validation(model, batches, thresholds=thr, path_save_results=str(plain), verbose=False)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            df1, met1 = validation.run_validation(model, batches, products_plot=PRODUCTS_PLOT, thresholds=thr,
                                                  path_save_results=str(plotted), verbose=False)
    assert [str(w.message) for w in rec] == [str(w.message) for w in rec_plain] == []
    assert df0.equals(df1)
    _same_metrics(met0, met1)
    for name in ("results.csv", "results_agg.json"):
        assert open(plain / name, "rb").read() == open(plotted / name, "rb").read(), name
    assert not (plain / "images").exists()
    assert sorted(os.listdir(plotted / "images")) == [f"tile_{i:02d}.png" for i in range(7)]
    scale, gap = 512 // 96, 4
    side = 96 * scale
    for i, b in enumerate(batches):
        out = model.batch_with_preds(validation.to_device(b, DEV))
        panels = plot.render_batch(out, PRODUCTS, PRODUCTS_PLOT)
        w, h, img, text = pu.decode_png(plotted / "images" / f"tile_{i:02d}.png")
        assert (w, h) == (4 * side + 3 * gap, side) == (panels.width, panels.height)
        assert np.array_equal(img, panels.image)
        meta = pu.png_comment(text)
        assert meta["names"] == PRODUCTS_PLOT and meta["ranges"] == [[0.0, 2.0], [0.0, 1.0], [0.0, 1.0], None]
        if i == 1:                                                     # and the canvas is what the contract says
            xs = [p * (side + gap) for p in range(4)]
            want = [(pu.band_bytes(out["input_norm"][0, 0].cpu().numpy(), 0, 2), scale, 0, xs[0]),
                    (pu.band_bytes(out["output_norm"][0, 0].cpu().numpy(), 0, 1), scale, 0, xs[1]),
                    (pu.band_bytes(out["prediction"][0, 0].cpu().numpy(), 0, 1), scale, 0, xs[2]),
                    (pu.cat_bytes(out["differences"][0, 0].cpu().numpy(), CATS), scale, 0, xs[3])]
            _assert_same(panels.scanlines, pu.compose(want, h, w))
            assert len(np.unique(img.reshape(-1, 3), axis=0)) > 20     # a picture, not a flat canvas
    # skip_saving_plots: the folder, no files (validation.py:146-151)
    skipped = tmp_path / "skipped"
    with np.errstate(all="ignore"):
        validation.run_validation(model, batches[:3], products_plot=PRODUCTS_PLOT, thresholds=thr, path_save_results=str(skipped),
                                  verbose=False, skip_saving_plots=True)
    assert os.listdir(skipped / "images") == []

    class Bare(torch.nn.Module):
        """neither a dataset nor a model that names the input channels"""

        def __init__(self, inner):
            super().__init__()
            self.device, self.batch_with_preds, self.threshold_spec = inner.device, inner.batch_with_preds, inner.threshold_spec
    with pytest.raises(ValueError, match="dataloader.dataset.input_products nor model.input_products"):
        validation.run_validation(Bare(model), batches[:1], products_plot=PRODUCTS_PLOT)


def _collate(batches):
    out = {k: torch.cat([b[k] for b in batches]) for k in ("input", "output", "has_plume")}
    out["id"] = [b["id"][0] for b in batches]
    return out


def test_image_logger_writes_both_splits(hip, tmp_path):
    tiles = _tiles(np.random.default_rng(12), 4, 64, 64)
    model = baselines.Mag1cBaseline(PRODUCTS).to(DEV)
    logged = []

    class Experiment:
        def log(self, what, commit=True):
            logged.append((what, commit))

    class Logger:
        experiment = Experiment()

    class Trainer:
        current_epoch, logger = 3, Logger()
    cb = data_logger.ImageLogger(_collate(tiles[:2]), _collate(tiles[2:]), PRODUCTS, ["rgb_aviris", "mag1c", "pred_binary", "differences"],
                                 folder=str(tmp_path / "log"))
    out_train = cb.on_train_epoch_end(Trainer(), model)
    out_val = cb.on_validation_epoch_end(Trainer(), model)
    assert list(out_train) == ["train_batch"] and list(out_val) == ["val_batch"]
    assert isinstance(out_train["train_batch"], plot.Panels) and isinstance(out_val["val_batch"], plot.Panels)
    # the logger gets something it can serialise: the image array (a wandb.Image where wandb is installed), never the Panels
    assert [list(w) for w, _ in logged] == [["train_batch"], ["val_batch"]] and [c for _, c in logged] == [False, False]
    if importlib.util.find_spec("wandb") is None:
        assert np.array_equal(logged[0][0]["train_batch"], out_train["train_batch"].image)
        assert np.array_equal(logged[1][0]["val_batch"], out_val["val_batch"].image)
    assert not any(isinstance(v, plot.Panels) for w, _ in logged for v in w.values())
    assert sorted(os.listdir(tmp_path / "log")) == ["train_epoch3.png", "val_epoch3.png"]
    p = out_val["val_batch"]
    scale = 512 // 64
    assert (p.height, p.width) == (2 * 64 * scale + 4, 4 * 64 * scale + 12) and len(p.rects) == 2 and p.names[0] == "rgb_aviris"
    w, h, img, text = pu.decode_png(tmp_path / "log" / "val_epoch3.png")
    assert np.array_equal(img, p.image) and pu.png_comment(text)["rows"] == 2
    out = model.batch_with_preds(validation.to_device(_collate(tiles[2:]), DEV))
    x = out["input_norm"].cpu().numpy()
    assert np.array_equal(p.panel(1, 0), np.repeat(np.repeat(pu.rgb_bytes(x[1, 1], x[1, 2], x[1, 3]), scale, 0), scale, 1))
    # "pred_binary" is a key of the batch, so that tensor is shown (the registry's "prediction" only stands in when it is not)
    assert np.array_equal(p.panel(1, 2), np.repeat(np.repeat(pu.band_bytes(out["pred_binary"][1, 0].cpu().numpy(), 0, 1), scale, 0), scale, 1))

    class NoLogger:
        current_epoch, logger = 0, None
    plain = data_logger.ImageLogger(_collate(tiles[:2]), _collate(tiles[2:]), PRODUCTS, ["label"])
    assert isinstance(plain.on_split_epoch_end(plain.batch_test, model, "val")["val_batch"], plot.Panels)
    assert isinstance(plain.on_train_epoch_end(NoLogger(), model)["train_batch"], plot.Panels) and len(logged) == 2


def test_plot_batch_returns_the_references_figure(hip):
    if importlib.util.find_spec("matplotlib") is None:
        with pytest.raises(ImportError):
            plot.plot_batch({}, PRODUCTS, PRODUCTS_PLOT)
        return
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    model = baselines.Mag1cBaseline(PRODUCTS).to(DEV)
    out = model.batch_with_preds(validation.to_device(_collate(_tiles(np.random.default_rng(13), 2, 64, 64)), DEV))
    fig, ax = plot.plot_batch(out, PRODUCTS, PRODUCTS_PLOT, add_id_to_title=False)
    assert ax.shape == (2, 4) and [a.get_title() for a in ax[0]] == PRODUCTS_PLOT and ax[1, 0].get_title() == ""
    assert tuple(fig.get_size_inches()) == (8.0, 4.0)
    shown = ax[1, 3].get_images()[0].get_array()
    assert np.array_equal(np.asarray(shown), plot.render_batch(out, PRODUCTS, PRODUCTS_PLOT).panel(1, 3))
    plt.close(fig)
