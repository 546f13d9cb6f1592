"""Time of the radial profiles of one orthorectified granule (sc_component_radial / plumes.component_radial) next to the two ways
to get the same numbers without it, in one process.

    python tools/bench_quantify.py [--rows 2000] [--cols 2300] [--blobs 300] [--bins 30] [--rounds 6] [--out profiles/quantify.txt]

On the seeded plume mask of tools/bench_component_stats.py, K radii of 1 .. K pixels, origins at the mag1c maximum:
  (k)  sc_component_radial: the library call alone (labels, boxes, origins, outputs and workspace allocated once; 3 launches)
  (a)  relabel + sc_component_stats: every foreground pixel gets the pseudo-component plume * (K+1) + bin (stock torch ops: the
       origin of its plume gathered, d2, torch.bucketize, a scatter into a zeroed image), then one sc_component_stats call over
       M * (K+1) rows; timed as a whole, and the sc_component_stats call alone on the relabelled image ((a'), the relabelling
       left out)
  (b)  stock torch ops: the same keys, then torch.bincount(key, weights=) for the fp64 sums and torch.bincount for the counts,
       over the foreground pixels only (their index list is built once, outside the timed region)
(k), (a), (a') and (b) alternate in rounds of 10 calls after 10 warm-up calls each; device events; the figure is the mean over all
rounds, the spread the minimum and maximum round.  Before anything is timed the counts are asserted equal and the sums to lie
within 2 * (n - 1) * 2^-53 * sum|v| of each other per bin (three different summation orders of float64).  Bytes of (k), by index
arithmetic: the labels and the plane of every bounding box once, the item records written and read.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_component_stats import scene  # noqa: E402
from starcop_amd import _lib, mask_creation, plumes  # noqa: E402
from starcop_amd._lib import check, ptr, stream  # noqa: E402

COPY_TBS = (4.25, 4.70)          # this project's access-pattern copy with 4-byte / 16-byte accesses (tools/membench/thin_pattern.hip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--cols", type=int, default=2300)
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("--bins", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    t_start = time.perf_counter()
    H, W, K = args.rows, args.cols, args.bins
    mask, mag, _ = scene(H, W, args.blobs, seed=20002300)
    plane = torch.from_numpy(mag).cuda()
    labels, n = mask_creation.connected_components(torch.from_numpy(mask).cuda())
    counts = torch.tensor([n], dtype=torch.int32, device="cuda")
    st = plumes.component_stats(labels, counts, [plane], M=n)
    origins = plumes.origins_from_argmax(st, W)
    radii = [float(j) for j in range(1, K + 1)]
    edge2 = [int(np.floor(r * r)) for r in radii]
    K1 = K + 1

    # ---- (k): the call as plumes.component_radial makes it, with everything allocated once
    first = plumes.component_radial(labels, counts, st, origins, radii, plane, M=n)
    out = {f: torch.empty_like(first[f]) for f in plumes.RADIAL_FIELDS}
    a = _lib.sc_cradial_args()
    a.labels, a.counts, a.N, a.H, a.W, a.M, a.K = labels.data_ptr(), counts.data_ptr(), 1, H, W, n, K
    a.row_min, a.row_max, a.col_min, a.col_max = (st[f].data_ptr() for f in ("row_min", "row_max", "col_min", "col_max"))
    a.origin, a.plane, a.plane_stride = origins.data_ptr(), plane.data_ptr(), H * W
    for j, e in enumerate(edge2):
        a.edge2[j] = e
    for f, t in out.items():
        setattr(a, f, t.data_ptr())
    wb = lib.sc_component_radial_workspace_bytes(1, H, W, n, K)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")

    def run_k():
        check(lib.sc_component_radial(a, ptr(work), wb, stream()))

    # ---- the keys of (a) and (b): plume * (K+1) + bin + 1, 0 for the background and for plumes without an origin
    # over the foreground pixels only (their indices are built once, outside the timed region, as (k)'s boxes are): 4.2 M background
    # pixels under one key would serialise bincount's fp64 atomics on one address and time that instead
    idx = torch.nonzero(labels.reshape(-1) > 0).reshape(-1)
    lab = labels.reshape(-1)[idx].long()
    rows, cols = idx // W, idx % W
    org = origins[0].long()
    edges_t = torch.tensor(edge2, dtype=torch.int64, device="cuda")
    flat = plane.reshape(-1)[idx]

    def keys():
        o = org[lab - 1]
        d2 = (rows - o[:, 0]) ** 2 + (cols - o[:, 1]) ** 2
        return torch.where(o[:, 0] >= 0, (lab - 1) * K1 + torch.bucketize(d2, edges_t) + 1, 0)

    # ---- (a): sc_component_stats over the relabelled image
    M2 = n * K1
    counts2 = torch.tensor([M2], dtype=torch.int32, device="cuda")
    out2 = {f: torch.empty((1, M2), dtype=plumes._DTYPES.get(f, torch.int64), device="cuda") for f in plumes.COMPONENT_FIELDS}
    out2.update({f: torch.empty((1, M2, 1), dtype=plumes._DTYPES.get(f, torch.int64), device="cuda") for f in plumes.PLANE_FIELDS})
    pseudo = torch.empty((H, W), dtype=torch.int32, device="cuda")
    b = _lib.sc_cstats_args()
    b.labels, b.counts, b.N, b.H, b.W, b.M, b.P = pseudo.data_ptr(), counts2.data_ptr(), 1, H, W, M2, 1
    b.plane[0], b.plane_stride[0] = plane.data_ptr(), H * W
    for f, t in out2.items():
        setattr(b, f, t.data_ptr())
    wb2 = lib.sc_component_stats_workspace_bytes(1, H, W, M2, 1)
    work2 = torch.empty(wb2, dtype=torch.uint8, device="cuda")

    def run_a_stats():
        check(lib.sc_component_stats(b, ptr(work2), wb2, stream()))

    def run_a():
        pseudo.zero_()
        pseudo.view(-1)[idx] = keys().int()
        run_a_stats()

    # ---- (b): bincount
    def run_b():
        key = keys()
        fin = torch.isfinite(flat)
        s = torch.bincount(key, weights=torch.where(fin, flat, 0).double(), minlength=M2 + 1)[1:]
        c = torch.bincount(key[fin], minlength=M2 + 1)[1:]
        return c.reshape(n, K1), s.reshape(n, K1)

    def events(fn, reps=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    def say(what):
        torch.cuda.synchronize()
        print(f"[{time.perf_counter() - t_start:7.1f} s] {what}", flush=True)

    # ---- equal first
    run_k()
    say("(k) ran")
    run_a()
    say("(a) ran")
    cb, sb = run_b()
    say("(b) ran")
    for f in plumes.RADIAL_FIELDS:
        assert torch.equal(out[f].view(torch.int64), first[f].view(torch.int64)), f"{f}: two calls differ"
    ck, sk = out["bin_count"][0], out["bin_sum"][0]
    ca, sa = out2["n_finite"][0, :, 0].reshape(n, K1), out2["sum"][0, :, 0].reshape(n, K1)
    fin = torch.isfinite(flat)
    sabs = torch.bincount(keys(), weights=torch.where(fin, flat, 0).abs().double(), minlength=M2 + 1)[1:].reshape(n, K1)
    assert torch.equal(ck, ca) and torch.equal(ck, cb), "bin counts differ"
    tol = 2.0 * (ck - 1).clamp(min=0).double() * 2.0 ** -53 * sabs
    for name, s in (("relabel + sc_component_stats", sa), ("bincount", sb)):
        assert bool(((sk - s).abs() <= tol).all()), f"{name}: bin sums differ from sc_component_radial beyond the bound"
    assert int(ck.sum()) == int(st["n_finite"][0, :, 0].sum()), "the bins do not hold every finite pixel"

    runs = (run_k, run_a, run_a_stats, run_b)
    for fn in runs:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    say("warm-up done")
    times = [[] for _ in runs]
    for _ in range(args.rounds):
        for t, fn in zip(times, runs):
            t.append(events(fn))
    say("rounds done")
    tk, ta, tas, tb = times
    for _ in range(3):
        plumes.component_radial(labels, counts, st, origins, radii, plane, M=n)
    api = events(lambda: plumes.component_radial(labels, counts, st, origins, radii, plane, M=n))

    host = {f: st[f][0].cpu().numpy().astype(np.int64) for f in ("row_min", "row_max", "col_min", "col_max", "area")}
    box_px = int(((host["row_max"] - host["row_min"] + 1) * (host["col_max"] - host["col_min"] + 1))[host["area"] > 0].sum())
    fg = int(host["area"].sum())
    heights = (host["row_max"] - host["row_min"] + 1)[host["area"] > 0]
    extra = (H * W + 511) // 512                   # the plan of the call: bands of bh rows, at most n + extra of them
    bh = int(min(max(-(-int(heights.sum()) // extra), 4), max(H, 4)))
    items = int((-(-heights // bh)).sum()) + int((host["area"] == 0).sum())
    rec = items * (32 + 16 * K1)
    moved = box_px * 8 + 2 * rec + n * (K1 * 16 + 32)
    mk = float(np.mean(tk))
    below = max(tk) < min(ta)
    lines = [
        f"radial profiles per component, {H} x {W} label image, {n} components ({fg} foreground pixels, bounding boxes {box_px} pixels), "
        f"K = {K} radii of 1 .. {K} pixels, one float32 plane (1 % NaN), origins at its maximum; {torch.cuda.get_device_name(0)} "
        f"({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; bin counts equal, bin sums within "
        f"2 (n - 1) 2^-53 sum|v| of each other, two calls of (k) identical bytes",
        f"(k) sc_component_radial (library call, 3 launches) {mk:9.3f} ms per call   (rounds {min(tk):.3f} .. {max(tk):.3f})",
        f"(k) through plumes.component_radial (edges, checks, allocations; device events, 10 calls) {api:9.3f} ms per call",
        f"(a) relabel (torch ops) + sc_component_stats over {M2} rows {np.mean(ta):9.3f} ms per call   (rounds {min(ta):.3f} .. {max(ta):.3f})"
        f"   (a) / (k) = {np.mean(ta) / mk:.1f}",
        f"(a') sc_component_stats over {M2} rows alone, the image relabelled beforehand {np.mean(tas):9.3f} ms per call   "
        f"(rounds {min(tas):.3f} .. {max(tas):.3f})   (a') / (k) = {np.mean(tas) / mk:.1f}",
        f"(b) stock torch ops (keys + bincount(weights=) + bincount) {np.mean(tb):9.3f} ms per call   (rounds {min(tb):.3f} .. {max(tb):.3f})"
        f"   (b) / (k) = {np.mean(tb) / mk:.1f}",
        f"every round of (k) below every round of (a): {'yes' if below else 'NO'};  below every round of (a'): "
        f"{'yes' if max(tk) < min(tas) else 'NO'};  below every round of (b): {'yes' if max(tk) < min(tb) else 'NO'}",
        f"(k) bytes: labels and plane of the boxes {box_px * 8 / 1e6:.1f} MB + {items} item records (bands of {bh} rows) "
        f"written and read {2 * rec / 1e6:.1f} MB + outputs {n * (K1 * 16 + 32) / 1e6:.2f} MB = {moved / 1e6:.1f} MB per call -> "
        f"{moved / (mk * 1e-3) / 1e12:.3f} TB/s, {moved / (mk * 1e-3) / 1e12 / COPY_TBS[0]:.3f} / {moved / (mk * 1e-3) / 1e12 / COPY_TBS[1]:.3f} of the "
        f"{COPY_TBS[0]} / {COPY_TBS[1]} TB/s access-pattern copy",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
