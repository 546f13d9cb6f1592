"""Time of burning the plume outlines of one orthorectified granule back into a label image (sc_rasterize_polygons /
plumes.rasterize_polygons) next to the same operator from stock torch ops and to the numpy restatement of tests/rasterize_util.py,
in one process.

    python tools/bench_rasterize.py [--rows 2000] [--cols 2300] [--blobs 300] [--rounds 6] [--out profiles/rasterize.txt]

  (a)  sc_rasterize_polygons alone on a prebuilt, uploaded table: the clearing of the image and the burn launch (the plume ids
       are 1..P, so there is no value-mapping launch, as in the call below)
  (a') plumes.rasterize_polygons as it is called: the host flattening of the rings, the one upload, the launches
  (b)  stock torch ops on the device, per polygon a broadcast crossing count over its box: (rows, edges) crossing tests and
       abscissae, (rows, edges, columns) comparisons summed over the edges, parity, masked assignment; the per-polygon edge
       tensors are uploaded once, outside the timed region
  (c)  the restatement (numpy, row by row) on the host, one run: a stated baseline, not a like-for-like comparison
(a), (a') and (b) alternate in rounds of 10 calls after 10 warm-up calls each (device events; (a') and (b) include their host
time); the figure is the mean over all rounds, the spread the minimum and maximum round.  All results are asserted equal to the
label image the outlines were traced from, and to (c), before anything is timed.  The mask is the seeded one of
tools/bench_component_stats.py.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rasterize_util as R  # noqa: E402
from bench_component_stats import scene  # noqa: E402
from starcop_amd import _lib, mask_creation, plumes  # noqa: E402

GT = (500000.0, 5.0, 0.0, 4100000.0, 0.0, -5.0)


def torch_plan(edges, table, dev):
    """per polygon: its edges on the device, its box and the pixel centres of the box"""
    plan = []
    for e0, e1, r0, r1, c0, c1, _, _ in table.tolist():
        if r1 <= r0 or e1 <= e0:
            plan.append(None)
            continue
        e = torch.from_numpy(edges[e0:e1]).to(dev)
        plan.append((e[:, 0], e[:, 1], e[:, 2], e[:, 3], (r0, r1, c0, c1),
                     torch.arange(r0, r1, device=dev, dtype=torch.float64)[:, None] + 0.5,
                     torch.arange(c0, c1, device=dev, dtype=torch.float64) + 0.5))
    return plan


def torch_rasterize(plan, values, shape, dev):
    out = torch.zeros(shape, dtype=torch.int32, device=dev)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    for item, v in zip(plan, values):
        if item is None:
            continue
        x0, y0, x1, y1, (r0, r1, c0, c1), yc, cc = item
        cross = (y0 <= yc) != (y1 <= yc)                                   # (rows, edges)
        xs = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0)                      # eager ops: each rounded on its own
        xs = torch.where(cross, xs, inf)
        odd = ((xs[:, :, None] <= cc).sum(1) & 1).bool()                   # (rows, columns)
        box = out[r0:r1, c0:c1]
        box[odd] = int(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--cols", type=int, default=2300)
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    H, W = args.rows, args.cols
    mask, _, _ = scene(H, W, args.blobs, seed=20002300)
    d_mask = torch.from_numpy(mask).cuda()
    labels, n = mask_creation.connected_components(d_mask)
    dev = labels.device
    polys = plumes.plume_outlines(d_mask, geotransform=GT)
    keys = list(polys)
    assert len(keys) == n
    rings = [polys[k] for k in keys]
    ids = np.array([k[1] for k in keys], dtype=np.int32)

    t = time.perf_counter()
    want = R.raster_ref([R.to_pixel(r, GT) for r in rings], ids, H, W)
    cpu = (time.perf_counter() - t) * 1e3
    print(f"restatement done: {cpu:.0f} ms", flush=True)
    assert np.array_equal(want, labels.cpu().numpy()), "the restatement does not give the label image back"

    edges, table = plumes.polygon_edges(rings, (H, W), GT)
    assert np.array_equal(ids, np.arange(1, n + 1))
    ops = plumes.rasterize_upload(edges, table, None)
    out_a = torch.empty((H, W), dtype=torch.int32, device=dev)
    plan = torch_plan(edges, table, dev)

    def run_a():
        return plumes.rasterize_launch(ops, (H, W), out=out_a)

    def run_call():
        return plumes.rasterize_polygons(polys, (H, W), geotransform=GT)

    def run_b():
        return torch_rasterize(plan, ids, (H, W), dev)

    def events(fn, reps=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    for name, got in (("sc_rasterize_polygons", run_a()), ("rasterize_polygons", run_call()), ("torch restatement", run_b())):
        assert torch.equal(got, labels), f"{name}: disagrees with the label image"
    print("results equal", flush=True)
    for fn in (run_a, run_call, run_b):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ta, tc, tb, tl = [], [], [], []
    for _ in range(args.rounds):
        ta.append(events(run_a))
        tc.append(events(run_call))
        tb.append(events(run_b))
    for _ in range(args.rounds):                                          # (a) again in windows long enough to time: 1000 calls each
        tl.append(events(run_a, reps=1000))

    rows = (table[:, 3] - table[:, 2]).astype(np.int64)
    nedge = (table[:, 1] - table[:, 0]).astype(np.int64)
    cols = (table[:, 5] - table[:, 4]).astype(np.int64)
    jobs, E = int(rows.sum()), len(edges)
    covered = int((want != 0).sum())
    # bytes by index arithmetic: the image cleared, every job reads its polygon's edges (32 B each, cache hits after the first row)
    # and its descriptor, every covered pixel is one 4-byte atomic (read + write)
    moved = H * W * 4 + int((rows * nedge).sum()) * 32 + jobs * 32 + covered * 8
    ma, mb, mc, ml = float(np.mean(ta)), float(np.mean(tb)), float(np.mean(tc)), float(np.mean(tl))
    lines = [
        f"polygon burn, {H} x {W} image, the outlines of its {n} components (connectivity 2) burnt back: {E} edges, {jobs} (polygon, row) "
        f"jobs, boxes of up to {int(rows.max())} rows x {int(cols.max())} columns, {covered} covered pixels; {torch.cuda.get_device_name(0)} "
        f"({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; the results of (a), (a') and (b) equal the "
        f"label image the outlines came from and the numpy restatement",
        f"(a)  sc_rasterize_polygons on an uploaded table: clear + one burn launch {ma:9.3f} ms per call   (rounds {min(ta):.3f} .. {max(ta):.3f})",
        f"(a)  the same in {args.rounds} rounds of 1000 calls (a round of 10 such calls is a window of a fraction of a millisecond) {ml:9.4f} ms per call   "
        f"(rounds {min(tl):.4f} .. {max(tl):.4f})",
        f"(a') plumes.rasterize_polygons as called (host flattening of {len(rings)} ring lists, one upload, the launches) {mc:9.3f} ms per call   "
        f"(rounds {min(tc):.3f} .. {max(tc):.3f})",
        f"(b)  stock torch ops, per polygon a broadcast crossing count over its box {mb:9.3f} ms per call   (rounds {min(tb):.3f} .. {max(tb):.3f})   "
        f"(b) / (a, long rounds) = {mb / ml:.0f}, (b) / (a') = {mb / mc:.2f}",
        f"(c)  numpy restatement on the host, row by row, one run {cpu:9.1f} ms   (c) / (a') = {cpu / mc:.0f}",
        f"(a)  bytes by index arithmetic: {moved / 1e6:.1f} MB per call ({H * W * 4 / 1e6:.1f} MB of it the clearing of the whole image)"
        f" -> {moved / (ml * 1e-3) / 1e12:.3f} TB/s at the long-round time, next to the 4.25 / 4.70 TB/s of the access-pattern copies",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
