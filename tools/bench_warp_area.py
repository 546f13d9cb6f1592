"""Time of the footprint resampling of the warp (sc_warp_area) next to what users had before it, to a stock-torch restatement and to
its own other mapping, in one process.

    python tools/bench_warp_area.py [--rounds 6] [--reps 10] [--out profiles/warp_area.txt]

Case: a seeded 9000 x 4000 float32 scene of 5 m pixels, five planes (8 % no-data, 4 % NaN) and one uint8 mask, onto a 60 m grid, twice:
  aligned : source and destination in one UTM zone on a shared lattice (boxes of 12 x 12 source pixels, corners on integers)
  geo     : the source on a geographic grid of similar sampling, the destination the UTM grid warp.suggest_grid gives at 60 m
Per case, device events around --reps calls, --rounds alternating rounds after 3 warm-up calls each:
  average, five planes, the mapping the library picks (lane groups) | the same with the thread-per-pixel mapping forced -- the pair
  that sets the threshold between the mappings | sc_warp nearest onto the same grid: what users got before, and the lower bound on
  the projection cost | mode and max of the uint8 mask | (aligned only) stock torch: avg_pool2d of x * m and of m, divide, where.
Before anything is timed: the two mappings agree (max / mode bit-equal, average within 2 * 2^-24 * max|x|), and on the aligned case
the average equals the stock-torch restatement within its float32 accumulation (144 * 2^-24 * max|x|) with the same data pixels
(blocks with exactly half of their samples counting left out: the threshold itself).
Bytes by index arithmetic: every source pixel under the destination grid once per plane, plus the outputs, next to the 4.25 / 4.70
TB/s access-pattern copy of tools/membench/thin_pattern.hip.  The five planes (720 MB) exceed the 256 MiB Infinity Cache, the mask
(36 MB) does not: repeated calls on the mask are served from it.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from starcop_amd import _lib, warp  # noqa: E402
from starcop_amd._lib import check, stream  # noqa: E402

HS, WS, P, FILL, RES = 9000, 4000, 5, -9999.0, 60.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(9000)
    src = torch.randn((P, HS, WS), generator=g, device="cuda") * 300 + 200
    src.masked_fill_(torch.rand((P, HS, WS), generator=g, device="cuda") < 0.08, FILL)
    src.masked_fill_(torch.rand((P, HS, WS), generator=g, device="cuda") < 0.04, float("nan"))
    mask = (torch.rand((1, HS, WS), generator=g, device="cuda") * 4).to(torch.uint8) * 60 + 1        # four classes, no-data 0 absent
    fill_bits = int(np.array(FILL, dtype=np.float32).reshape(1).view(np.uint32)[0])
    vmax = float(src[torch.isfinite(src) & (src != FILL)].abs().max())
    px = 5.4e-4 / 12
    cases = {"aligned": ((600120.0, 5.0, 0.0, 3590460.0, 0.0, -5.0), 32613), "geo": ((-103.94127, px, 0.0, 32.45231, 0.0, -px), 4326)}
    lines = [f"footprint resampling, {HS} x {WS} source of 5 m pixels -> 60 m EPSG:32613 grid, {P} float32 planes ({src.nbytes / 1e6:.0f} MB, 8 % "
             f"no-data, 4 % NaN) and one uint8 mask ({mask.nbytes / 1e6:.0f} MB); {torch.cuda.get_device_name(0)} "
             f"({torch.cuda.get_device_properties(0).gcnArchName})",
             f"{args.rounds} alternating rounds of {args.reps} calls after 3 warm-up calls each, device events; min_coverage 0.5"]

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps          # ms per call

    for case, (src_gt, src_crs) in cases.items():
        (H, W), dst_gt = warp.suggest_grid((HS, WS), src_gt, src_crs, 32613, RES)
        inv = warp.invert_geotransform(src_gt)
        s_code, d_code = (0, 0) if src_crs == 32613 else (src_crs, 32613)
        out = torch.empty((P, H, W), dtype=torch.float32, device="cuda")
        out2 = torch.empty((P, H, W), dtype=torch.float32, device="cuda")
        out_mask = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
        out_mask2 = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")

        def area(t, dst, mode, variant=0):
            a = _lib.sc_warp_area_args()
            for i in range(6):
                a.dst_gt[i], a.src_inv[i] = dst_gt[i], inv[i]
            a.dst_crs, a.src_crs, a.out_h, a.out_w, a.src_h, a.src_w = d_code, s_code, H, W, HS, WS
            a.P, a.elem_bytes, a.mode, a.variant, a.min_coverage = t.shape[0], t.element_size(), mode, variant, 0.5
            for p in range(a.P):
                a.src[p] = t[p].data_ptr()
                a.row_stride[p], a.col_stride[p] = t.stride(1), t.stride(2)
                a.nodata_bits[p] = fill_bits if t.dtype == torch.float32 else 0
            a.out = dst.data_ptr()
            return lambda: check(lib.sc_warp_area(a, stream()))

        def nearest(t, dst):
            a = _lib.sc_warp_args()
            for i in range(6):
                a.dst_gt[i], a.src_inv[i] = dst_gt[i], inv[i]
            a.dst_crs, a.src_crs, a.out_h, a.out_w, a.src_h, a.src_w = d_code, s_code, H, W, HS, WS
            a.P, a.elem_bytes, a.resampling = t.shape[0], t.element_size(), _lib.WARP_NEAREST
            for p in range(a.P):
                a.src[p] = t[p].data_ptr()
                a.row_stride[p], a.col_stride[p] = t.stride(1), t.stride(2)
                a.nodata_bits[p] = fill_bits
            a.out = dst.data_ptr()
            return lambda: check(lib.sc_warp(a, stream()))

        def torch_average():
            m = (torch.isfinite(src) & (src != FILL)).float()
            num = F.avg_pool2d(torch.where(m > 0, src, torch.zeros_like(src))[None], 12)[0]
            den = F.avg_pool2d(m[None], 12)[0]
            return torch.where(den >= 0.5, num / den, torch.full_like(num, FILL)), den

        picked = warp.area_variant((H, W), dst_gt, 32613, src_gt, src_crs)
        fns = {"avg": area(src, out, _lib.WARP_AREA_AVERAGE), "avg_thread": area(src, out2, _lib.WARP_AREA_AVERAGE, _lib.WARP_AREA_THREAD),
               "nearest": nearest(src, out2), "mode": area(mask, out_mask, _lib.WARP_AREA_MODE), "max": area(mask, out_mask, _lib.WARP_AREA_MAX),
               "mode_thread": area(mask, out_mask2, _lib.WARP_AREA_MODE, _lib.WARP_AREA_THREAD)}
        # ---- checks first
        fns["avg"](); fns["avg_thread"]()
        data = out.view(torch.int32) != fill_bits - (1 << 32)
        assert torch.equal(data, out2.view(torch.int32) != fill_bits - (1 << 32)), "the mappings disagree on the data pixels"
        err_v = float((out - out2)[data].abs().max())
        assert err_v <= 2 * 2.0 ** -24 * vmax, err_v
        fns["mode"](); fns["mode_thread"]()
        assert torch.equal(out_mask, out_mask2), "mode: the mappings disagree"
        fns["max"](); area(mask, out_mask2, _lib.WARP_AREA_MAX, _lib.WARP_AREA_THREAD)()
        assert torch.equal(out_mask, out_mask2), "max: the mappings disagree"
        note = f"mappings agree: average within {err_v:.3g} (gate {2 * 2.0 ** -24 * vmax:.3g}), mode and max bit-equal"
        if case == "aligned":
            want, den = torch_average()
            hh, ww = want.shape[1:]
            fns["avg"]()
            got = out[:, :hh, :ww]
            keep = (den * 144).round() != 72                                # exactly half of a block counting: the threshold itself
            gd, wd = got.view(torch.int32) != fill_bits - (1 << 32), want.view(torch.int32) != fill_bits - (1 << 32)
            assert torch.equal(gd[keep], wd[keep]), "data pixels differ from the stock-torch restatement"
            err_t = float((got - want)[keep & gd].abs().max())
            assert err_t <= 144 * 2.0 ** -24 * vmax, err_t
            note += f"; average within {err_t:.3g} of the stock-torch restatement (gate {144 * 2.0 ** -24 * vmax:.3g}), same data pixels"
            del want, den, keep, gd, wd
            fns["torch"] = torch_average
        # ---- times
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(events(fn))
        mean = {k: float(np.mean(v)) for k, v in times.items()}

        def row(k):
            return f"{mean[k] * 1e3:10.1f} us per call   (rounds {min(times[k]) * 1e3:.1f} .. {max(times[k]) * 1e3:.1f})"
        boxes = warp.source_boxes((H, W), dst_gt, 32613, src_gt, src_crs)
        bw, bh = float((boxes[1] - boxes[0]).mean()), float((boxes[3] - boxes[2]).mean())
        u0, u1 = boxes[0].clamp(0, WS), boxes[1].clamp(0, WS)
        v0, v1 = boxes[2].clamp(0, HS), boxes[3].clamp(0, HS)
        under = float(((u1.max() - u0.min()) * (v1.max() - v0.min())))      # source pixels under the destination grid (its bounding box)
        under = min(under, HS * WS)
        b5, b1 = P * (under * 4 + H * W * 4), under + H * W
        lines += [
            "",
            f"{case}: source EPSG:{src_crs} -> {H} x {W} pixels, mean box {bw:.2f} x {bh:.2f} source pixels, the library picks `{picked}`; {note}",
            f"  average, {P} planes, lane groups                 {row('avg')}",
            f"  average, {P} planes, thread per pixel (forced)   {row('avg_thread')}   = {mean['avg_thread'] / mean['avg']:.2f} x lane groups",
            f"  sc_warp nearest, {P} planes, same grid           {row('nearest')}   average (lane groups) = {mean['avg'] / mean['nearest']:.2f} x this",
            f"  mode, uint8 mask, lane groups                   {row('mode')}",
            f"  mode, uint8 mask, thread per pixel (forced)     {row('mode_thread')}",
            f"  max, uint8 mask, lane groups                    {row('max')}",
        ]
        if "torch" in fns:
            lines.append(f"  stock torch (avg_pool2d of x*m and m, where)    {row('torch')}   = {mean['torch'] / mean['avg']:.2f} x lane groups")
        lines += [
            f"  bytes, {P} planes: {under * 4 * P / 1e6:.0f} MB read once + {P * H * W * 4 / 1e6:.1f} MB written = {b5 / 1e6:.0f} MB (beyond the 256 MiB "
            f"Infinity Cache) -> lane groups {b5 / (mean['avg'] * 1e-3) / 1e12:.2f} TB/s, {100 * b5 / (mean['avg'] * 1e-3) / 4.25e12:.0f} % / "
            f"{100 * b5 / (mean['avg'] * 1e-3) / 4.70e12:.0f} % of the 4.25 / 4.70 TB/s access-pattern copy; thread per pixel "
            f"{b5 / (mean['avg_thread'] * 1e-3) / 1e12:.2f} TB/s",
            f"  bytes, the mask: {b1 / 1e6:.0f} MB (inside the Infinity Cache: repeated calls do not reach HBM) -> mode {b1 / (mean['mode'] * 1e-3) / 1e12:.2f} "
            f"TB/s, max {b1 / (mean['max'] * 1e-3) / 1e12:.2f} TB/s",
        ]
        del out, out2, out_mask, out_mask2, boxes
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
