"""Time of one mosaic (sc_mosaic) next to the path a user had before it -- one sc_warp per scene onto the common grid and a chain of
torch.where -- in one process.

    python tools/bench_mosaic.py [--rounds 6] [--reps 10] [--out profiles/mosaic.txt]

Case: six seeded 2000 x 2300 geographic grids with an EMIT-like pixel (5.42e-4 degrees, ~60 m), two across-track by three
along-track with 15 % overlap each way, composed onto their mosaic.union_grid in the UTM zone of the centre at 60 m; five float32
planes (8 % no-data holes), rule "max" on plane 0, nearest.
  (a)  sc_mosaic: the library call alone (device events; outputs and the device table allocated once, boxes computed once)
  (b)  the sequential path: six sc_warp calls (library calls alone, outputs allocated once) onto the same grid and the composite
       with stock torch ops: per scene valid = key != no-data and not NaN, take = valid & (first | key > best), torch.where
  (c)  one sc_warp coordinates-only call (P = 0) of scene 0 onto the same grid: the unit of projection work
(a) and (b) alternate in rounds of --reps calls after 3 warm-up calls each; the figure is the mean over all rounds, the spread the
minimum and maximum round.  Before anything is timed the planes of (a) and (b) are asserted bit-equal.  Also printed: the wall
time of mosaic.mosaic (Python side included: boxes, table, allocation), the share of (tile, scene) pairs and of tiles the cull
skips, and the bytes the algorithm has to move.
"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from starcop_amd import _lib, warp  # noqa: E402
from starcop_amd import mosaic as M  # noqa: E402
from starcop_amd._lib import check, stream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    Hs, Ws, P, N, fill = 2000, 2300, 5, 6, -9999.0
    px = 0.000542232520256367
    lon_w, lat_n = -106.18127, 34.01731
    grids = [(lon_w + i * 0.85 * Ws * px, px, 0.0, lat_n - j * 0.85 * Hs * px, 0.0, -px) for j in range(3) for i in range(2)]
    dst_crs = warp.utm_crs_for(lon_w + 0.925 * Ws * px, lat_n - 1.35 * Hs * px)
    (H, W), dst_gt = M.union_grid([((Hs, Ws), g, 4326) for g in grids], dst_crs, 60.0)
    srcs_np = []
    for s in range(N):
        rng = np.random.default_rng(3000 + s)
        a = (rng.standard_normal((P, Hs, Ws)) * 300 + 200).astype(np.float32)
        a[rng.random((P, Hs, Ws)) < 0.08] = fill
        srcs_np.append(a)
    srcs = [torch.from_numpy(a).cuda() for a in srcs_np]
    del srcs_np

    def case(H, W):
        fill_bits = int(np.array([fill], dtype=np.float32).view(np.uint32)[0])
        boxes = [M.footprint_box((Hs, Ws), g, 4326, dst_gt, dst_crs, (H, W)) for g in grids]
        invs = [warp.invert_geotransform(g) for g in grids]

        # ---- (a) one sc_mosaic call
        table = (_lib.sc_mosaic_source * N)()
        for s in range(N):
            q = table[s]
            for i in range(6):
                q.src_inv[i] = invs[s][i]
            q.src_crs, q.src_h, q.src_w = 4326, Hs, Ws
            for i in range(4):
                q.box[i] = boxes[s][i]
            for p in range(P):
                q.src[p] = srcs[s][p].data_ptr()
                q.row_stride[p], q.col_stride[p] = srcs[s].stride(1), srcs[s].stride(2)
        out_a = torch.empty((P, H, W), dtype=torch.float32, device="cuda")
        dev_table = torch.empty(ctypes.sizeof(table), dtype=torch.uint8, device="cuda")
        ma = _lib.sc_mosaic_args()
        for i in range(6):
            ma.dst_gt[i] = dst_gt[i]
        ma.dst_crs, ma.out_h, ma.out_w, ma.N, ma.P, ma.elem_bytes = dst_crs, H, W, N, P, 4
        ma.rule, ma.key_plane, ma.resampling, ma.flags = _lib.MOSAIC_MAX, 0, _lib.WARP_NEAREST, _lib.MOSAIC_KEY_FLOAT
        for p in range(P):
            ma.nodata_bits[p] = fill_bits
        ma.sources, ma.table, ma.out = ctypes.cast(table, ctypes.POINTER(_lib.sc_mosaic_source)), dev_table.data_ptr(), out_a.data_ptr()

        def run_a():
            check(lib.sc_mosaic(ma, stream()))

        # ---- (b) six sc_warp calls and the composite
        warped = [torch.empty((P, H, W), dtype=torch.float32, device="cuda") for _ in range(N)]
        coords = torch.empty((2, H, W), dtype=torch.float64, device="cuda")

        def warp_args(s, planes, dst, uv=None):
            a = _lib.sc_warp_args()
            for i in range(6):
                a.dst_gt[i], a.src_inv[i] = dst_gt[i], invs[s][i]
            a.dst_crs, a.src_crs, a.out_h, a.out_w, a.src_h, a.src_w = dst_crs, 4326, H, W, Hs, Ws
            a.P, a.elem_bytes, a.resampling = planes, 4, _lib.WARP_NEAREST
            for p in range(planes):
                a.src[p] = srcs[s][p].data_ptr()
                a.row_stride[p], a.col_stride[p] = srcs[s].stride(1), srcs[s].stride(2)
                a.nodata_bits[p] = fill_bits
            a.out = dst.data_ptr() if planes else None
            a.coords = uv.data_ptr() if uv is not None else None
            return a
        wa = [warp_args(s, P, warped[s]) for s in range(N)]
        a_uv = warp_args(0, 0, None, coords)
        fill_t = torch.tensor(fill, dtype=torch.float32, device="cuda")

        def run_b():
            out = best = has = None
            for s in range(N):
                check(lib.sc_warp(wa[s], stream()))
                w = warped[s]
                k = w[0]
                valid = (k != fill_t) & ~torch.isnan(k)
                if out is None:
                    out, best, has = torch.where(valid, w, fill_t), k, valid
                    continue
                take = valid & (~has | (k > best))
                out, best, has = torch.where(take, w, out), torch.where(take, k, best), has | valid
            return out

        def run_uv():
            check(lib.sc_warp(a_uv, stream()))

        def events(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.reps          # ms per call

        run_a()
        out_b = run_b()
        torch.cuda.synchronize()
        assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)), "sc_mosaic disagrees with the sequential path"
        del out_b
        sources = [(srcs[s], grids[s], 4326) for s in range(N)]
        res, index, count = M.mosaic(sources, dst_gt, dst_crs, (H, W), "max", 0, "nearest", fill, return_index=True, return_count=True)
        assert torch.equal(res.view(torch.int32), out_a.view(torch.int32))
        index, count = index.cpu().numpy(), count.cpu().numpy()
        del res

        fns = {"mosaic": run_a, "seq": run_b, "uv": run_uv}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(events(fn))
        mean = {k: float(np.mean(v)) for k, v in times.items()}
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.reps):
            M.mosaic(sources, dst_gt, dst_crs, (H, W), "max", 0, "nearest", fill)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3 / args.reps

        def row(k):
            return f"{mean[k] * 1e3:9.1f} us per call   (rounds {min(times[k]) * 1e3:.1f} .. {max(times[k]) * 1e3:.1f})"
        vec = W % 4 == 0
        th, tw = (16, 64) if vec else (4, 64)
        ty, tx = -(-H // th), -(-W // tw)
        r0, c0 = np.arange(ty)[:, None] * th, np.arange(tx)[None, :] * tw
        live = np.stack([(b[0] < r0 + th) & (b[1] > r0) & (b[2] < c0 + tw) & (b[3] > c0) for b in boxes])
        pairs, empty = float(1.0 - live.mean()), float((~live.any(axis=0)).mean())
        inside = int(count.sum())                       # every plane is dense but for the holes: valid ~ 92 % of inside
        moved_a = P * H * W * 4 + inside * 4 + int((index >= 0).sum()) * (P - 1) * 4
        moved_b = N * P * H * W * 4 + (N - 1) * (3 * P + 2) * H * W * 4
        below = max(times["mosaic"]) < min(times["seq"])
        lines = [
            f"mosaic, {N} geographic grids of {Hs} x {Ws} ({px:.6g} degrees; 2 across x 3 along, 15 % overlap) -> {H} x {W} EPSG:{dst_crs} grid "
            f"at 60 m, {P} float32 planes per scene ({N * P * Hs * Ws * 4 / 1e6:.0f} MB, 8 % no-data), rule max on plane 0, "
            f"nearest; {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
            f"{args.rounds} alternating rounds of {args.reps} calls after 3 warm-up calls each, device events; (a) and (b) asserted bit-equal first; "
            f"{100.0 * (index >= 0).mean():.1f} % of the pixels have a winner, {100.0 * (count >= 2).mean():.1f} % lie in an overlap",
            f"(a) sc_mosaic, one launch ({'4 pixels' if vec else '1 pixel'} per thread)          {row('mosaic')}",
            f"(b) {N} x sc_warp + torch.where composite               {row('seq')}   (b) / (a) = {mean['seq'] / mean['mosaic']:.2f}",
            f"(c) one sc_warp coordinates-only call onto this grid   {row('uv')}   (a) = {mean['mosaic'] / mean['uv']:.2f} of these, (b) = "
            f"{mean['seq'] / mean['uv']:.2f}",
            f"every round of (a) below every round of (b): {'yes' if below else 'NO'}",
            f"mosaic.mosaic, Python side included (boxes, table, allocation), host clock around {args.reps} calls and a synchronise: "
            f"{wall * 1e3:.1f} us per call",
            f"cull: tiles of {th} x {tw} pixels, {ty * tx} tiles; {100.0 * pairs:.1f} % of the (tile, scene) pairs are skipped, "
            f"{100.0 * empty:.1f} % of the tiles meet no box and project nothing",
            f"bytes the algorithm moves: (a) {moved_a / 1e6:.0f} MB ({P} planes written, the key element of every valid scene and the other "
            f"{P - 1} planes of the winner read) -> {moved_a / (mean['mosaic'] * 1e-3) / 1e12:.2f} TB/s; (b) at least {moved_b / 1e6:.0f} MB "
            f"({N} x {P} full-grid intermediates written, and per composite step the intermediate, the running result and the masks read "
            f"and the result written)",
        ]
        return lines

    W4 = -(-W // 4) * 4                              # the same grid widened to whole 4-pixel vectors: the 16-byte store variant
    lines = case(H, W) + (["", f"the same with the grid widened by {W4 - W} columns to a multiple of 4:"] + case(H, W4) if W4 != W else [])
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
