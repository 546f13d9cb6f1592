"""Time of whole-scene cloud masking (sentinel2.CDModel.predict_scene) on a Sentinel-2 tile against the same procedure staged with
stock torch ops, and of its two data-movement kernels on their own, in one process.

    python tools/bench_cdmodel_scene.py [--size 10980] [--rounds 6] [--reps 10] [--out profiles/cdmodel_scene.txt]

Case: seeded weights and BatchNorm statistics (the recipe of tools/bench_cdmodel.py), a seeded 13 x --size x --size uint16 scene of
digital numbers in [0, 10000) on the device, scale 1e-4.
  (a)  model.predict_scene(scene, tile, scale=1e-4) at tile 1024 and 2048: sc_scene_gather out of the uint16 scene, the network, the
       head writing every window's core into the (H, W) result (sc_head_conv_fwd_k_mosaic)
  (b)  the same windows (sentinel2.scene_windows) staged with torch: scene.float() * scale, F.pad(mode="reflect") to the padded scene,
       torch.stack of slices, net.predict_classes, slice copies of the cores into the (H, W) result
  (c)  sc_scene_gather of one batch of windows next to torch.stack of slices of the ALREADY padded float32 scene (the pad is not in
       this figure); sc_head_conv_fwd_k_mosaic on a seeded (batch, 16, wh, ww) tensor next to sc_head_conv_fwd_k (classes only)
       followed by the slice copies of the cores
(a) and (b) alternate in rounds of --reps calls after a warm-up call each (device events); likewise the forms of (c) after 3 warm-up
calls.  The figure is the mean over all rounds, the spread the minimum and maximum round.  Results are asserted equal before anything
is timed.  Peak memory: torch.cuda.max_memory_allocated over the calls of a form, the resident scene included.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from starcop_amd import _lib, sentinel2  # noqa: E402
from starcop_amd._lib import ACT_RELU, SC_CST, SRC_AFFINE, check, make_src, ptr, stream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10980)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tiles", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    S, K, SCALE = args.size, 4, 1e-4
    torch.manual_seed(0)
    model = sentinel2.CDModel(device="cuda")
    net = model.model
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
        net.segmentation_head[0].bias.copy_(torch.randn(K, generator=g) * 0.1)
    scene = torch.randint(0, 10000, (13, S, S), generator=torch.Generator(device="cuda").manual_seed(2), device="cuda",
                          dtype=torch.int32).to(torch.int16).view(torch.uint16)
    scene_i16 = scene.view(torch.int16)

    def batch_of(plan):
        return max(1, min(sentinel2.SCENE_BATCH_PIXELS // (plan.window[0] * plan.window[1]), plan.offsets.shape[0]))

    def padded(plan):
        x = scene_i16.to(torch.int32).float() * SCALE           # (DN < 32768: the int16 view holds the values)
        return F.pad(x[None], (plan.pad_cols[0], plan.pad_cols[1], plan.pad_rows[0], plan.pad_rows[1]), mode="reflect")[0]

    def torch_staged(tile):
        plan = sentinel2.scene_windows(S, S, tile)
        xp = padded(plan)
        wh, ww = plan.window
        out = torch.empty((S, S), dtype=torch.uint8, device="cuda")
        rows = list(zip(plan.offsets.tolist(), plan.cores.tolist(), plan.dests.tolist()))
        b = batch_of(plan)
        for k in range(0, len(rows), b):
            chunk = rows[k:k + b]
            cl = net.predict_classes(torch.stack([xp[:, r:r + wh, c:c + ww] for (r, c), _, _ in chunk]))
            for j, (_, (y0, y1, x0, x1), (dr, dc)) in enumerate(chunk):
                out[dr:dr + y1 - y0, dc:dc + x1 - x0] = cl[j, y0:y1, x0:x1]
        return out

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() / 2 ** 30

    def fig(v, unit=1.0):
        return f"{float(np.mean(v)) * unit:9.1f}   (rounds {min(v) * unit:.1f} .. {max(v) * unit:.1f})"

    lines = [f"CDModel.predict_scene, 13 x {S} x {S} uint16 scene (seeded DN in [0, 10000), scale 1e-4), precision {net.precision!r}; "
             f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
             f"{args.rounds} alternating rounds of {args.reps} calls after warm-up, device events; resident scene {scene.numel() * 2 / 2 ** 30:.2f} GiB"]
    # ---- (a) / (b): whole scene
    fns, names = [], []
    for tile in args.tiles:
        plan = sentinel2.scene_windows(S, S, tile)
        got = model.predict_scene(scene, tile=tile, scale=SCALE)
        want = torch_staged(tile)
        torch.cuda.synchronize()
        ndiff = int((got != want).sum())
        assert ndiff == 0, f"tile {tile}: predict_scene differs from the torch-staged procedure in {ndiff} pixels"
        counts = torch.bincount(got.flatten().long(), minlength=K).tolist()
        lines.append(f"tile {tile}: {plan.offsets.shape[0]} windows of {plan.window[0]} x {plan.window[1]}, batch {batch_of(plan)}; "
                     f"predict_scene == torch-staged in all {S * S} pixels (class counts {counts})")
        del got, want
        fns += [lambda tile=tile: model.predict_scene(scene, tile=tile, scale=SCALE), lambda tile=tile: torch_staged(tile)]
        names += [f"(a) predict_scene, tile {tile}", f"(b) torch-staged (float32 F.pad, slices, stitch), tile {tile}"]
    mem = [peak(fn) for fn in fns]
    t = [[] for _ in fns]
    for _ in range(args.rounds):
        for i, fn in enumerate(fns):
            t[i].append(events(fn, args.reps))
    for nm, v, m in zip(names, t, mem):
        lines.append(f"{nm:62s}{fig(v)} ms per call; peak {m:.2f} GiB allocated")
    for i, tile in enumerate(args.tiles):
        a, b = t[2 * i], t[2 * i + 1]
        lines.append(f"tile {tile}: rounds of (a) {'lie below' if max(a) < min(b) else 'OVERLAP with or lie above'} the rounds of (b)")
    best = args.tiles[int(np.argmin([float(np.mean(t[2 * i])) for i in range(len(args.tiles))]))]
    lines.append(f"faster tile of (a): {best}")
    # ---- (c): the two kernels on one batch of the first tile's plan
    plan = sentinel2.scene_windows(S, S, args.tiles[0])
    wh, ww = plan.window
    n = batch_of(plan)
    first = (plan.offsets.shape[0] // 2 // n) * n                      # an interior batch
    first = min(first, plan.offsets.shape[0] - n)
    table = sentinel2.scene_table(plan)
    table_dev = torch.from_numpy(table).cuda()
    xp = padded(plan)
    gout = torch.empty((n, 13, wh, ww), device="cuda")
    offs = plan.offsets[first:first + n].tolist()

    def run_gather():
        return sentinel2.scene_gather(scene_i16, (plan.pad_rows[0], plan.pad_cols[0]), table_dev, table, first, n, plan.window, SCALE, out=gout)

    def run_stack():
        return torch.stack([xp[:, r:r + wh, c:c + ww] for r, c in offs])

    assert torch.equal(run_gather(), run_stack()), "sc_scene_gather differs from its torch restatement"
    h_in = torch.randn(n, 16, wh, ww, generator=torch.Generator().manual_seed(3)).cuda()
    cst = torch.zeros(16, SC_CST, device="cuda")
    cst[:, 0], cst[:, 1] = 1.0, 0.1
    src_h = make_src(h_in, 16, SRC_AFFINE, act=ACT_RELU, cst=cst)
    w_head, b_head = net.segmentation_head[0].weight, net.segmentation_head[0].bias
    h_classes = torch.empty(n, wh, ww, dtype=torch.uint8, device="cuda")
    mos_a = torch.zeros((S, S), dtype=torch.uint8, device="cuda")
    mos_b = torch.zeros((S, S), dtype=torch.uint8, device="cuda")
    rows = list(zip(plan.cores[first:first + n].tolist(), plan.dests[first:first + n].tolist()))

    def run_mosaic():
        check(lib.sc_head_conv_fwd_k_mosaic(C.byref(src_h), ptr(w_head), ptr(b_head), ptr(mos_a), S, S, S, table_dev.data_ptr() + 32 * first,
                                            table.ctypes.data + 32 * first, n, 16, K, wh, ww, stream()))

    def run_classes_copies():
        check(lib.sc_head_conv_fwd_k(C.byref(src_h), ptr(w_head), ptr(b_head), None, ptr(h_classes), n, 16, K, wh, ww, stream()))
        for j, ((y0, y1, x0, x1), (dr, dc)) in enumerate(rows):
            mos_b[dr:dr + y1 - y0, dc:dc + x1 - x0] = h_classes[j, y0:y1, x0:x1]

    run_mosaic(); run_classes_copies()
    assert torch.equal(mos_a, mos_b), "the mosaic head differs from sc_head_conv_fwd_k followed by copies"
    core_px = sum((y1 - y0) * (x1 - x0) for (y0, y1, x0, x1), _ in rows)
    cfns = (run_gather, run_stack, run_mosaic, run_classes_copies)
    for fn in cfns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    tc = [[] for _ in cfns]
    for _ in range(args.rounds):
        for i, fn in enumerate(cfns):
            tc[i].append(events(fn, args.reps))
    gbytes_w, px = 4 * n * 13 * wh * ww, n * wh * ww
    lines += [
        f"(c) one batch of tile {args.tiles[0]}: {n} window(s) of {wh} x {ww}, rows {first}..{first + n - 1} of the plan; gather == torch.stack of "
        f"slices of the padded float32 scene, mosaic head == sc_head_conv_fwd_k + copies",
        f"(c) sc_scene_gather, uint16 -> float32 * scale                {fig(tc[0], 1e3)} us per call; {gbytes_w / 2e6:.1f} MB read + "
        f"{gbytes_w / 1e6:.1f} MB written = {1.5 * gbytes_w / 1e3 / float(np.mean(tc[0])) / 1e6:.2f} TB/s",
        f"(c) torch.stack of slices of the padded float32 scene         {fig(tc[1], 1e3)} us per call; {gbytes_w / 1e6:.1f} MB read + "
        f"{gbytes_w / 1e6:.1f} MB written = {2 * gbytes_w / 1e3 / float(np.mean(tc[1])) / 1e6:.2f} TB/s",
        f"(c) sc_head_conv_fwd_k_mosaic, 16 -> 4, cores only             {fig(tc[2], 1e3)} us per call; {core_px / 1e6:.2f} of {px / 1e6:.2f} Mpx are core",
        f"(c) sc_head_conv_fwd_k (classes) + slice copies of the cores  {fig(tc[3], 1e3)} us per call",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
