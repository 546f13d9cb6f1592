"""Time of writing a scene product as a Cloud-Optimized GeoTIFF from the device (cog.write_cog) against the writer the pipelines
use by default (io_formats.write_tiff of the host copy), in one process.

    python tools/bench_write_cog.py [--rows 9000] [--cols 4000] [--rounds 6] [--out profiles/write_cog.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_write_cog.py --kernels-only [--predictor auto]

Case: the seeded flight-line-like scene of tools/bench_aviris_scene.py on the device: a --rows x --cols rectangle of fill (-9999)
with a slanted valid strip |x - (0.175 cols + 0.29 y)| < 0.1625 cols; one float32 plane (a probability U(0, 1) inside the strip,
nodata -9999 outside: pred.tif) and one uint8 mask (plane > 0.5 inside the strip, 0 outside: predbinary.tif).
  (a) io_formats.write_tiff(x.cpu().numpy(), blocksize=128): the default path of the pipelines, the yardstick
  (b) cog.write_cog(x, overviews=(), sparse=False): the same single-resolution file, tiles cut on the device, deflate on the pool
  (c) cog.write_cog(x): overviews and sparse tiles, as it defaults
Results are asserted equal before anything is timed: the full resolution of every file reads back equal to the source (bits), and
every level of (c) equals the numpy restatement (tests/cog_util.py).  (a), (b) and (c) then alternate in rounds of one call after a
warm-up call each, timed with a host clock around work that ends in a device synchronise and a closed file.  The kernels alone are
timed with device events (10 calls per round): the pyramid launches, the flag launches and the pack launches of all levels (the
pack figure includes the read-back of the slot table that its argument check makes).  Bytes moved are computed from the shapes.
--kernels-only launches the kernels of both products --reps times and nothing else: the run to put under a kernel trace, whose
per-kernel durations are free of the read-back and of launch gaps (--predictor none / auto picks the pack variant).
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cog_util  # noqa: E402
from starcop_amd import _lib, cog, io_formats  # noqa: E402

FILL = -9999.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=9000)
    ap.add_argument("--cols", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--predictor", default="none", choices=["none", "auto"])
    args = ap.parse_args()
    _lib.require_device()
    H, W = args.rows, args.cols
    gd = torch.Generator(device="cuda").manual_seed(2)
    yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    valid = (xx - (0.175 * W + 0.29 * yy)).abs() < 0.1625 * W
    plane = torch.where(valid, torch.rand((H, W), generator=gd, device="cuda"), torch.tensor(FILL, device="cuda"))
    mask = ((plane > 0.5) & valid).to(torch.uint8)
    del yy, xx
    products = [("float32 plane (pred.tif)", plane, FILL, "average"), ("uint8 mask (predbinary.tif)", mask, None, "mode")]
    workers = cog.default_workers()
    lines = [f"cog.write_cog against io_formats.write_tiff, {H} x {W} flight-line-like scene ({H * W / 1e6:.1f} Mpx, "
             f"{100 * float(valid.float().mean()):.1f} % valid: a slanted strip in a fill rectangle), 128 x 128 tiles, deflate level 6; "
             f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); {workers} deflate threads "
             f"({len(os.sched_getaffinity(0))} CPUs in this process's affinity mask)",
             f"{args.rounds} alternating rounds of one call after a warm-up call each; host clock around device synchronise + closed file"]
    if args.kernels_only:
        for name, x, nodata, resampling in products:
            n_over = len(cog.overview_levels(H, W))
            levels = [x[None]] + cog.build_overviews(x[None], n_over, resampling, nodata)
            pred = 1 if args.predictor == "none" else (3 if x.element_size() == 4 else 2)
            stored = 0
            for _ in range(args.reps):
                cog.build_overviews(x[None], n_over, resampling, nodata)
                for im in levels:
                    keep = cog.tile_flags(im, 128, nodata) == 0
                    s = torch.where(keep, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
                    sh = s.cpu().numpy()
                    stored = int((sh >= 0).sum())
                    cog.pack_tiles(im, 128, pred, s, sh, stored)
            torch.cuda.synchronize()
            print(f"{name}: {args.reps} x ({-(-n_over // 3)} pyramid launches, {len(levels)} flag launches, {len(levels)} pack launches, predictor {pred})")
        return
    tmp = tempfile.TemporaryDirectory()

    def path(name):
        return os.path.join(tmp.name, name)

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def fig(v, unit=1.0):
        return f"{float(np.mean(v)) * unit:9.1f}   (rounds {min(v) * unit:.1f} .. {max(v) * unit:.1f})"

    for name, x, nodata, resampling in products:
        tags = {42113: (2, (f"{nodata:.9g}",))} if nodata is not None else {}
        eb = x.element_size()

        def run_a():
            torch.cuda.synchronize()
            io_formats.write_tiff(path("a.tif"), x.cpu().numpy(), blocksize=128, extra_tags=tags)

        def run_b():
            r = cog.write_cog(path("b.tif"), x, overviews=(), sparse=False, nodata=nodata)
            torch.cuda.synchronize()
            return r

        def run_c():
            r = cog.write_cog(path("c.tif"), x, nodata=nodata)
            torch.cuda.synchronize()
            return r

        # ---- equal results first
        run_a()
        rb, rc = run_b(), run_c()
        host = x.cpu().numpy()[None]
        for f in ("a.tif", "b.tif", "c.tif"):
            assert cog_util.same_bits(io_formats.read_tiff(path(f)), host), f"{name}: {f} does not read back equal to the source"
        n_lev = io_formats.tiff_ifd_count(path("c.tif"))
        want = cog_util.pyramid(host, n_lev - 1, resampling, nodata)
        for k, w in enumerate(want):
            got = io_formats.read_tiff(path("c.tif"), info=io_formats.tiff_info(path("c.tif"), ifd=k + 1))
            assert cog_util.same_bits(got, w), f"{name}: overview {k + 1} differs from the numpy restatement"
        problems = io_formats.cog_layout_problems(path("c.tif")) + io_formats.cog_layout_problems(path("b.tif"))
        assert not problems, problems
        size_a, size_b, size_c = (os.path.getsize(path(f)) for f in ("a.tif", "b.tif", "c.tif"))
        auto = cog.write_cog(path("p.tif"), x, nodata=nodata, predictor="auto")
        assert cog_util.same_bits(io_formats.read_tiff(path("p.tif")), host)
        lines += ["", f"{name}: full resolution of (a), (b), (c) == the source (bits); the {n_lev - 1} overviews of (c) ({resampling}) == the numpy "
                  f"restatement; layout rules hold",
                  f"  (c): {rc['levels']} levels, {rc['tiles_stored']} of {rc['tiles']} tiles stored ({rb['tiles_stored']} of {rb['tiles']} in (b)), "
                  f"{rc['bytes_to_host'] / 1e6:.1f} MB device-to-host ((b): {rb['bytes_to_host'] / 1e6:.1f} MB; (a): {x.numel() * eb / 1e6:.1f} MB)",
                  f"  file sizes: (a) {size_a / 1e6:.2f} MB, (b) {size_b / 1e6:.2f} MB, (c) predictor None {size_c / 1e6:.2f} MB, (c) predictor "
                  f"'auto' {auto['bytes_written'] / 1e6:.2f} MB"]
        # ---- (a) / (b) / (c), host clock
        fns = (run_a, run_b, run_c)
        t = [[] for _ in fns]
        for _ in range(args.rounds):
            for i, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t[i].append(time.perf_counter() - t0)
        for nm, v in zip(("(a) write_tiff(x.cpu().numpy())", "(b) write_cog(overviews=(), sparse=False)", "(c) write_cog()"), t):
            lines.append(f"  {nm:46s}{fig(v, 1e3)} ms per file")
        lines.append(f"  every round of (c) {'lies below' if max(t[2]) < min(t[0]) else 'DOES NOT lie below'} every round of (a): "
                     f"max (c) {max(t[2]) * 1e3:.1f} ms, min (a) {min(t[0]) * 1e3:.1f} ms; mean (a) / mean (c) = {np.mean(t[0]) / np.mean(t[2]):.1f}")
        # ---- the kernels alone, device events
        x3 = x[None]
        levels = [x3] + cog.build_overviews(x3, n_lev - 1, resampling, nodata)
        flags = [cog.tile_flags(im, 128, nodata) for im in levels]
        slots = []
        for f in flags:
            keep = f == 0
            s = torch.where(keep, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
            slots.append((s, s.cpu().numpy(), int(keep.sum())))
        outs = [torch.empty((n, 128 * 128 * eb), dtype=torch.uint8, device="cuda") for _, _, n in slots]
        pred = 3 if eb == 4 else 2

        def k_pyramid():
            cog.build_overviews(x3, n_lev - 1, resampling, nodata)

        def k_flags():
            for im in levels:
                cog.tile_flags(im, 128, nodata)

        def k_pack(p):
            for im, (s, sh, n), o in zip(levels, slots, outs):
                cog.pack_tiles(im, 128, p, s, sh, n, out=o)

        kf = (k_pyramid, k_flags, lambda: k_pack(1), lambda: k_pack(pred))
        for fn in kf:
            fn()
        tk = [[] for _ in kf]
        for _ in range(args.rounds):
            for i, fn in enumerate(kf):
                tk[i].append(events(fn, args.reps))
        px = [int(im.shape[1]) * int(im.shape[2]) for im in levels]
        launches = -(-(n_lev - 1) // 3)
        pyr_bytes = eb * (sum(px[3 * i] for i in range(launches)) + sum(px[1:]))
        flag_bytes = eb * sum(px)
        pack_bytes = 2 * sum(n for _, _, n in slots) * 128 * 128 * eb

        def rate(nbytes, v):
            return f"{nbytes / 1e6:.1f} MB moved = {nbytes / 1e9 / float(np.mean(v)):.2f} TB/s"
        lines += [f"  sc_overview_reduce, {n_lev - 1} levels in {launches} launches        {fig(tk[0], 1e3)} us; {rate(pyr_bytes, tk[0])}",
                  f"  sc_tiff_tile_flags, {n_lev} levels                        {fig(tk[1], 1e3)} us; {rate(flag_bytes, tk[1])}",
                  f"  sc_tiff_pack_tiles, {n_lev} levels, predictor 1           {fig(tk[2], 1e3)} us; {rate(pack_bytes, tk[2])}",
                  f"  sc_tiff_pack_tiles, {n_lev} levels, predictor {pred}           {fig(tk[3], 1e3)} us; {rate(pack_bytes, tk[3])}",
                  "  (the access-pattern copy of this device reaches 4.25 / 4.70 TB/s; the pack figures include one blocking read-back of the "
                  "slot table per level)"]
        del levels, flags, slots, outs
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
