"""Time of whole-flight-line plume detection (ModelModule.predict_scene) against the same windows staged with stock torch ops, and of
its new kernels on one window, in one process.

    python tools/bench_aviris_scene.py [--rows 9000] [--cols 4000] [--rounds 6] [--reps 10] [--out profiles/aviris_scene.txt]

Case: seeded weights and BatchNorm statistics (the recipe of tools/bench_cdmodel.py), head bias = minus the median logit of the valid
core pixels of the fullest tile-1024 window (so that about half of the valid pixels lie above the threshold); a seeded
flight-line-like scene on the device: a --rows x --cols rectangle of fill (-9999) with a slanted valid strip
|x - (0.175 cols + 0.29 y)| < 0.1625 cols, mag1c ~ 600 N(0, 1) + 200 in a dense plane, radiance ~ U(0.5, 12) in ONE (rows, cols, 3)
buffer read in place, acquisition-date factor 1.037, mag1c clipped to [0, 10000].
  (a)  model.predict_scene(planes, fill, scales, clips, tile) with skip_empty (sc_scene_core_counts, then only windows whose core
       holds data: sc_scene_gather_planes, the network, sc_head_conv_fwd_mosaic_prob)
  (a') the same with skip_empty=False: every window is cut and run
  (b)  every window of the same plan staged with torch: where(x == fill, 0, x * s) / clamp per plane, F.pad(mode="reflect"),
       torch.stack of slices, the eval forward, masks_from_logits, slice copies of the cores, fill pixels -> nodata / 0
  (c)  one interior window: sc_scene_gather_planes next to torch.stack of slices of the ALREADY prepared and padded scene (neither
       the per-plane ops nor the pad are in that figure); sc_head_conv_fwd_mosaic_prob next to sc_head_conv_fwd + sc_threshold_masks
       + slice copies of the core; sc_scene_core_counts over the whole plan
(a), (a') and (b) alternate in rounds of --reps calls after a warm-up call each (device events); likewise the forms of (c) after 3
warm-up calls.  The figure is the mean over all rounds, the spread the minimum and maximum round.  Results are asserted equal (bits
of the probability, the mask) before anything is timed.  Peak memory: torch.cuda.max_memory_allocated over a call, the resident
scene included.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from starcop_amd import _lib, model_module as mm, sentinel2  # noqa: E402
from starcop_amd._lib import ACT_RELU, SC_CST, SRC_AFFINE, check, make_src, ptr, stream  # noqa: E402

FILL, FACTOR, NODATA = -9999.0, 1.037, -9999.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=9000)
    ap.add_argument("--cols", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tiles", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    H, W = args.rows, args.cols
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1)).to("cuda").eval()
    net = model.network
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
        net.segmentation_head[0].bias.zero_()
    gd = torch.Generator(device="cuda").manual_seed(2)
    yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    valid = (xx - (0.175 * W + 0.29 * yy)).abs() < 0.1625 * W
    fill_t = torch.tensor(FILL, device="cuda")
    mf = torch.where(valid, torch.randn((H, W), generator=gd, device="cuda") * 600.0 + 200.0, fill_t)
    rgb = torch.where(valid[:, :, None], torch.rand((H, W, 3), generator=gd, device="cuda") * 11.5 + 0.5, fill_t)
    planes = [mf, rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]]
    fills, scales, clips = [FILL] * 4, [None, FACTOR, FACTOR, FACTOR], [(0.0, 10000.0), None, None, None]
    del yy, xx
    with torch.no_grad():                                              # the head bias: minus the median logit of one window's valid core
        plan = sentinel2.scene_windows(H, W, 1024)
        table = sentinel2.scene_table(plan)
        table_dev = torch.from_numpy(table).cuda()
        i = int(sentinel2.scene_core_counts(planes[0], FILL, table_dev, table).argmax())
        x = sentinel2.scene_gather_planes(planes, (plan.pad_rows[0], plan.pad_cols[0]), table_dev, table, i, 1, plan.window, fills, scales, clips)
        (y0, y1, x0, x1), (dr, dc) = plan.cores[i].tolist(), plan.dests[i].tolist()
        z = model(x)[0, 0, y0:y1, x0:x1][valid[dr:dr + y1 - y0, dc:dc + x1 - x0]]
        net.segmentation_head[0].bias.fill_(-float(z.median()))
        del x, z

    def batch_of(plan, n=None):
        return max(1, min(sentinel2.SCENE_BATCH_PIXELS // (plan.window[0] * plan.window[1]), n if n is not None else plan.offsets.shape[0]))

    def prepared():
        out = []
        for p, s, c in zip(planes, scales, clips):
            v = torch.where(p == FILL, torch.zeros((), device="cuda"), p * s if s is not None else p)
            out.append(v.clamp(c[0], c[1]) if c is not None else v)
        return torch.stack(out)

    def padded(plan):
        return F.pad(prepared()[None], (plan.pad_cols[0], plan.pad_cols[1], plan.pad_rows[0], plan.pad_rows[1]), mode="reflect")[0]

    def torch_staged(tile):
        plan = sentinel2.scene_windows(H, W, tile)
        xp = padded(plan)
        wh, ww = plan.window
        prob = torch.empty((H, W), dtype=torch.float32, device="cuda")
        mask = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        rows = list(zip(plan.offsets.tolist(), plan.cores.tolist(), plan.dests.tolist()))
        b = batch_of(plan)
        for k in range(0, len(rows), b):
            chunk = rows[k:k + b]
            m = mm.masks_from_logits(model(torch.stack([xp[:, r:r + wh, c:c + ww] for (r, c), _, _ in chunk])))
            for j, (_, (y0, y1, x0, x1), (dr, dc)) in enumerate(chunk):
                if y1 > y0 and x1 > x0:
                    prob[dr:dr + y1 - y0, dc:dc + x1 - x0] = m["prediction"][j, 0, y0:y1, x0:x1]
                    mask[dr:dr + y1 - y0, dc:dc + x1 - x0] = m["pred_binary"][j, 0, y0:y1, x0:x1]
        hole = planes[0] == FILL
        return torch.where(hole, torch.tensor(NODATA, device="cuda"), prob), torch.where(hole, torch.zeros((), dtype=torch.uint8, device="cuda"), mask)

    def scene(tile, skip):
        return model.predict_scene(planes, fill_value=FILL, scales=scales, clips=clips, tile=tile, skip_empty=skip, nodata=NODATA)

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

    resident = (mf.numel() + rgb.numel()) * 4 / 2 ** 30
    lines = [f"ModelModule.predict_scene, {H} x {W} flight-line-like scene ({H * W / 1e6:.1f} Mpx, {100 * float(valid.float().mean()):.1f} % valid: a "
             f"slanted strip in a fill rectangle), 4 products, precision {net.precision!r}; "
             f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
             f"{args.rounds} alternating rounds of {args.reps} calls after warm-up, device events; resident scene {resident:.2f} GiB"]
    # ---- (a) / (a') / (b): whole scene
    fns, names, tiles_of = [], [], []
    for tile in args.tiles:
        plan = sentinel2.scene_windows(H, W, tile)
        a, a2 = scene(tile, True), scene(tile, False)
        wp, wm = torch_staged(tile)
        torch.cuda.synchronize()
        for nm, r in (("skip_empty", a), ("skip_empty=False", a2)):
            nd = int((r["prediction"].view(torch.int32) != wp.view(torch.int32)).sum()) + int((r["pred_binary"] != wm).sum())
            assert nd == 0, f"tile {tile}: predict_scene ({nm}) differs from the torch-staged procedure in {nd} values"
        plume = int(a["pred_binary"].sum())
        lines.append(f"tile {tile}: {a['windows']} windows of {plan.window[0]} x {plan.window[1]}, batch {batch_of(plan)}; {a['windows_run']} run with "
                     f"skip_empty, {a2['windows_run']} without; prediction (bits) and pred_binary == torch-staged in all {H * W} pixels "
                     f"({plume} plume pixels = {100 * plume / max(int(valid.sum()), 1):.1f} % of the valid ones)")
        del a, a2, wp, wm
        fns += [lambda tile=tile: scene(tile, True), lambda tile=tile: scene(tile, False), lambda tile=tile: torch_staged(tile)]
        names += [f"(a)  predict_scene, skip_empty, tile {tile}", f"(a') predict_scene, skip_empty=False, tile {tile}",
                  f"(b)  torch-staged (where/mul/clamp, F.pad, slices, stitch), tile {tile}"]
        tiles_of += [tile] * 3
    mem = [peak(fn) for fn in fns]
    t = [[] for _ in fns]
    for _ in range(args.rounds):
        for i, fn in enumerate(fns):
            t[i].append(events(fn, args.reps))
    for nm, v, m in zip(names, t, mem):
        lines.append(f"{nm:70s}{fig(v)} ms per scene; peak {m:.2f} GiB allocated")
    for i, tile in enumerate(args.tiles):
        a, a2, b = t[3 * i], t[3 * i + 1], t[3 * i + 2]
        lines.append(f"tile {tile}: rounds of (a) {'lie below' if max(a) < min(b) else 'OVERLAP with or lie above'} the rounds of (b); rounds of (a') "
                     f"{'lie below' if max(a2) < min(b) else 'OVERLAP with or lie above'} the rounds of (b)")
    best = args.tiles[int(np.argmin([float(np.mean(t[3 * i])) for i in range(len(args.tiles))]))]
    lines.append(f"faster tile of (a): {best} (sentinel2.SCENE_TILE = {sentinel2.SCENE_TILE})")
    # ---- (c): the kernels on one interior window of the first tile's plan
    plan = sentinel2.scene_windows(H, W, args.tiles[0])
    wh, ww = plan.window
    table = sentinel2.scene_table(plan)
    table_dev = torch.from_numpy(table).cuda()
    counts = sentinel2.scene_core_counts(planes[0], FILL, table_dev, table).cpu().numpy()
    first = int(np.argmax(counts))                                     # the window whose core holds the most data
    xp = padded(plan)
    gout = torch.empty((1, 4, wh, ww), device="cuda")
    r0, c0 = plan.offsets[first].tolist()

    def run_gather():
        return sentinel2.scene_gather_planes(planes, (plan.pad_rows[0], plan.pad_cols[0]), table_dev, table, first, 1, plan.window, fills, scales,
                                             clips, out=gout)

    def run_stack():
        return torch.stack([xp[:, r0:r0 + wh, c0:c0 + ww]])

    assert torch.equal(run_gather().view(torch.int32), run_stack().view(torch.int32)), "sc_scene_gather_planes differs from its torch restatement"
    h_in = torch.randn(1, 16, wh, ww, generator=torch.Generator().manual_seed(3)).cuda()
    cst = torch.zeros(16, SC_CST, device="cuda")
    cst[:, 0], cst[:, 1] = 1.0, 0.1
    src_h = make_src(h_in, 16, SRC_AFFINE, act=ACT_RELU, cst=cst)
    w_head, b_head = net.segmentation_head[0].weight, net.segmentation_head[0].bias
    logits = torch.empty(1, 1, wh, ww, device="cuda")
    pred = torch.empty(1, 1, wh, ww, device="cuda")
    pb = torch.empty(1, 1, wh, ww, dtype=torch.int64, device="cuda")
    prob_a, mask_a = torch.zeros((H, W), device="cuda"), torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    prob_b, mask_b = torch.zeros((H, W), device="cuda"), torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    (y0, y1, x0, x1), (dr, dc) = plan.cores[first].tolist(), plan.dests[first].tolist()
    fb = sentinel2.float_bits(FILL)

    def run_mosaic():
        check(lib.sc_head_conv_fwd_mosaic_prob(C.byref(src_h), ptr(w_head), ptr(b_head), ptr(prob_a), W, ptr(mask_a), W, H, W, ptr(planes[0]),
                                               planes[0].stride(0), planes[0].stride(1), fb, NODATA, table_dev.data_ptr() + 32 * first,
                                               table.ctypes.data + 32 * first, 1, 16, wh, ww, stream()))

    def run_head_copies():
        check(lib.sc_head_conv_fwd(C.byref(src_h), ptr(w_head), ptr(b_head), ptr(logits), 1, 16, wh, ww, stream()))
        check(lib.sc_threshold_masks(ptr(logits), None, 0, ptr(pred), ptr(pb), None, None, 1, wh * ww, stream()))
        hole = planes[0][dr:dr + y1 - y0, dc:dc + x1 - x0] == FILL
        prob_b[dr:dr + y1 - y0, dc:dc + x1 - x0] = torch.where(hole, torch.tensor(NODATA, device="cuda"), pred[0, 0, y0:y1, x0:x1])
        mask_b[dr:dr + y1 - y0, dc:dc + x1 - x0] = torch.where(hole, torch.zeros((), dtype=torch.int64, device="cuda"), pb[0, 0, y0:y1, x0:x1])

    def run_counts():
        return sentinel2.scene_core_counts(planes[0], FILL, table_dev, table)

    run_mosaic(); run_head_copies()
    assert torch.equal(prob_a.view(torch.int32), prob_b.view(torch.int32)) and torch.equal(mask_a, mask_b), \
        "the mosaic head differs from sc_head_conv_fwd + sc_threshold_masks + copies"
    cfns = (run_gather, run_stack, run_mosaic, run_head_copies, run_counts)
    for fn in cfns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    tc = [[] for _ in cfns]
    for _ in range(args.rounds):
        for i, fn in enumerate(cfns):
            tc[i].append(events(fn, args.reps))
    gbytes = 4 * 4 * wh * ww
    core_px = (y1 - y0) * (x1 - x0)
    lines += [
        f"(c) one window of tile {args.tiles[0]}: {wh} x {ww}, row {first} of the plan ({int(counts[first])} of its {core_px} core pixels are data); gather == "
        f"torch.stack of slices of the prepared, padded scene; mosaic head == sc_head_conv_fwd + sc_threshold_masks + copies",
        f"(c) sc_scene_gather_planes, 4 planes, fill / scale / clip        {fig(tc[0], 1e3)} us per call; {gbytes / 1e6:.1f} MB read + "
        f"{gbytes / 1e6:.1f} MB written = {2 * gbytes / 1e3 / float(np.mean(tc[0])) / 1e6:.2f} TB/s",
        f"(c) torch.stack of slices of the prepared, padded scene          {fig(tc[1], 1e3)} us per call; {gbytes / 1e6:.1f} MB read + "
        f"{gbytes / 1e6:.1f} MB written = {2 * gbytes / 1e3 / float(np.mean(tc[1])) / 1e6:.2f} TB/s",
        f"(c) sc_head_conv_fwd_mosaic_prob, 16 -> 1, core only, valid plane {fig(tc[2], 1e3)} us per call; {core_px / 1e6:.2f} of {wh * ww / 1e6:.2f} Mpx are core",
        f"(c) sc_head_conv_fwd + sc_threshold_masks + copies of the core   {fig(tc[3], 1e3)} us per call",
        f"(c) sc_scene_core_counts, {table.shape[0]} windows over the {H} x {W} plane        {fig(tc[4], 1e3)} us per call; {H * W * 4 / 1e6:.1f} MB read = "
        f"{H * W * 4 / 1e3 / float(np.mean(tc[4])) / 1e6:.2f} TB/s",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
