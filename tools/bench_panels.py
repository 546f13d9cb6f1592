"""One validation figure of a 512 x 512 tile (rgb_aviris, mag1c, label, differences; scale 1, gap 4), drawn four ways:

    python tools/bench_panels.py [--size 512] [--rounds 6] [--out profiles/panels.txt]

(a) sc_panel_minmax + sc_render_panels on a prebuilt table: two launches, the canvas is PNG scanlines;
(a') plot.render_batch: the same plus selecting the tensors, building and uploading the table and allocating the canvas;
(b) the same canvas from stock torch ops in the same process: normalise, LUT gather by index, repeat_interleave, cat;
(c) io_formats.write_png alone on the finished canvas (host, zlib level 6);
(d) where matplotlib is importable: a figure built the way the reference's plot_batch builds it (subplots, one imshow per panel,
    titles) + savefig, on host copies of the tensors (the copies are not timed).
(a) and (b) are asserted equal, byte for byte, and equal to the numpy restatement of tests/plot_util.py, before anything is timed.
(a) and (b) alternate in rounds of 10 calls after 10 warm-up calls each and are timed with device events; the figure is the mean
over the rounds, the spread their minimum and maximum.  (c) and (d) are host clocks over 5 calls.
"""
import argparse
import importlib.util
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import plot_util as pu  # noqa: E402
from starcop_amd import _lib, io_formats, plot  # noqa: E402
from starcop_amd._lib import check, stream  # noqa: E402

PRODUCTS = ["mag1c", "TOA_AVIRIS_640nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_460nm"]
PRODUCTS_PLOT = ["rgb_aviris", "mag1c", "label", "differences"]
GAP = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    S = args.size
    rng = np.random.default_rng(512)
    x = np.concatenate([np.abs(rng.normal(0, 0.4, size=(1, S, S))), rng.uniform(-0.05, 1.1, size=(3, S, S))]).astype(np.float32)
    x[0, 5, :3] = [np.nan, np.inf, 2.5]
    lab = (rng.uniform(size=(S, S)) < 0.2).astype(np.float32)
    dif = rng.integers(0, 4, size=(S, S)).astype(np.int64)
    batch = {"input": torch.from_numpy(x[None]).cuda(), "input_norm": torch.from_numpy(x[None]).cuda(),
             "output_norm": torch.from_numpy(lab[None, None]).cuda(), "differences": torch.from_numpy(dif[None, None]).cuda()}
    Hc, Wc = S, 4 * S + 3 * GAP
    xs = [p * (S + GAP) for p in range(4)]
    cats = plot._DIFF_CATEGORIES
    want = pu.compose([(pu.rgb_bytes(x[1], x[2], x[3]), 1, 0, xs[0]), (pu.band_bytes(x[0], 0, 2), 1, 0, xs[1]),
                       (pu.band_bytes(lab, 0, 1), 1, 0, xs[2]), (pu.cat_bytes(dif, cats), 1, 0, xs[3])], Hc, Wc)

    # (a): the table render_batch builds, kept
    rows = plot._item_rows(plot.select_panels(batch, PRODUCTS, PRODUCTS_PLOT), 1)
    table, rects, hc, wc = plot._layout(rows, S, GAP)
    assert (hc, wc) == (Hc, Wc) and [r[1] for r in rects[0]] == xs
    first = plot.render_batch(batch, PRODUCTS, PRODUCTS_PLOT, panel_px=S, gap=GAP)
    n = len(table)
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    minmax = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    canvas = torch.empty(Hc * (1 + 3 * Wc), dtype=torch.uint8, device="cuda")

    def run_a():
        check(lib.sc_panel_minmax(table_dev.data_ptr(), table, n, minmax.data_ptr(), stream()))
        check(lib.sc_render_panels(table_dev.data_ptr(), table, n, minmax.data_ptr(), canvas.data_ptr(), Hc, Wc, stream()))

    def run_a2():
        return plot.render_batch(batch, PRODUCTS, PRODUCTS_PLOT, panel_px=S, gap=GAP)

    # (b): tables built once
    lut = torch.from_numpy(plot.viridis8()).cuda()
    catlut = torch.tensor([c for _, c in cats], dtype=torch.uint8, device="cuda")
    white = torch.full((), 255, dtype=torch.uint8, device="cuda")
    gapcol = torch.full((S, GAP, 3), 255, dtype=torch.uint8, device="cuda")
    filt = torch.zeros((Hc, 1), dtype=torch.uint8, device="cuda")
    inp, labd, difd = batch["input_norm"][0], batch["output_norm"][0, 0], batch["differences"][0, 0]

    def band(v, vmin, vmax):
        xa = (v - vmin) / (vmax - vmin) * 256.0
        rgb = lut[xa.clamp(0.0, 255.0).nan_to_num(0.0).long()]
        return torch.where(torch.isfinite(v)[..., None], rgb, white)

    def enlarge(p, scale=1):
        return p.repeat_interleave(scale, 0).repeat_interleave(scale, 1)

    def run_b():
        c = inp[1:4].permute(1, 2, 0)
        rgb = torch.where(torch.isnan(c).any(-1, keepdim=True), white, (c.clamp(0.0, 1.0) * 255.0).to(torch.uint8))
        panels = [enlarge(rgb), enlarge(band(inp[0], 0.0, 2.0)), enlarge(band(labd, 0.0, 1.0)), enlarge(catlut[difd])]
        img = torch.cat([panels[0], gapcol, panels[1], gapcol, panels[2], gapcol, panels[3]], dim=1)
        return torch.cat([filt, img.reshape(Hc, 3 * Wc)], dim=1)

    def events(fn, reps=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    run_a()
    got_b = run_b()
    torch.cuda.synchronize()
    got_a = canvas.cpu().numpy().reshape(Hc, 1 + 3 * Wc)
    assert np.array_equal(got_a, want), "sc_render_panels disagrees with the numpy restatement"
    assert np.array_equal(first.scanlines, want), "render_batch disagrees with the numpy restatement"
    assert np.array_equal(got_b.cpu().numpy(), want), "the torch restatement disagrees with the numpy restatement"
    for fn in (run_a, run_a2, run_b):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ta, ta2, tb = [], [], []
    for _ in range(args.rounds):
        ta.append(events(run_a))
        ta2.append(events(run_a2))
        tb.append(events(run_b))

    def host(fn, reps=5):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps * 1e3

    tmp = tempfile.mkdtemp(prefix="panels")
    png = os.path.join(tmp, "a.png")
    tc = host(lambda: io_formats.write_png(png, got_a, Wc, Hc, text="{}"))
    png_bytes = os.path.getsize(png)
    t0 = time.perf_counter()
    for _ in range(5):
        run_a2().save(png)
    tsave = (time.perf_counter() - t0) / 5 * 1e3
    td = None
    if importlib.util.find_spec("matplotlib") is not None:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        hx, hl, hd = x, lab, plot.mask_to_rgb(dif, [0, 1, 2, 3], plot.COLORS_DIFFERENCES)

        def run_d():
            fig, ax = plt.subplots(1, 4, figsize=(16, 4), tight_layout=True, squeeze=False)
            ax[0, 0].imshow(np.transpose(np.clip(hx[1:4], 0, 1), (1, 2, 0)))
            ax[0, 1].imshow(hx[0], vmin=0, vmax=2)
            ax[0, 2].imshow(hl, vmin=0, vmax=1, interpolation="nearest")
            ax[0, 3].imshow(hd, interpolation="nearest")
            for k, name in enumerate(PRODUCTS_PLOT):
                ax[0, k].set_title(name)
            plt.savefig(os.path.join(tmp, "ref.png"), format="png")
            plt.close(fig)
        td = host(run_d)

    shutil.rmtree(tmp, ignore_errors=True)
    read = S * S * (3 * 4 + 4 + 4 + 8)
    written = Hc * (1 + 3 * Wc)
    ma, ma2, mb = float(np.mean(ta)), float(np.mean(ta2)), float(np.mean(tb))
    lines = [
        f"validation figure of one {S} x {S} tile: {', '.join(PRODUCTS_PLOT)}; scale 1, gap {GAP}: canvas {Hc} x {Wc} pixels "
        f"({written / 1e6:.2f} MB of PNG scanlines); {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; (a), (a') and (b) equal the numpy "
        f"restatement in all {written} bytes",
        f"(a)  sc_panel_minmax + sc_render_panels, prebuilt table {ma * 1e3:9.1f} us per call   (rounds {min(ta) * 1e3:.1f} .. {max(ta) * 1e3:.1f})",
        f"(a') plot.render_batch (select, table upload, 2 launches) {ma2 * 1e3:9.1f} us per call   (rounds {min(ta2) * 1e3:.1f} .. {max(ta2) * 1e3:.1f})",
        f"(b)  stock torch ops (LUT gather, repeat_interleave, cat) {mb * 1e3:9.1f} us per call   (rounds {min(tb) * 1e3:.1f} .. {max(tb) * 1e3:.1f})"
        f"   (b) / (a) = {mb / ma:.2f}, (b) / (a') = {mb / ma2:.2f}",
        f"(c)  write_png alone (zlib level 6, host)                {tc:9.2f} ms per call   ({png_bytes / 1e6:.2f} MB file); "
        f"render_batch + read-back + save: {tsave:.2f} ms per figure",
        (f"(d)  matplotlib {matplotlib.__version__} figure (4 imshow + titles) + savefig, host {td:9.1f} ms per call" if td is not None
         else "(d)  matplotlib is not importable here: not measured"),
        f"(a) bytes per call: {read / 1e6:.2f} MB read + {written / 1e6:.2f} MB written = {(read + written) / 1e6:.2f} MB -> "
        f"{(read + written) / (ma * 1e-3) / 1e12:.3f} TB/s, next to this project's access-pattern copy figures of 4.25 / 4.70 TB/s "
        f"on hundreds of MB",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
