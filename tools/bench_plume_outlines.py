"""Time of the plume outlines of one orthorectified granule (sc_component_outlines / plumes.plume_outlines) next to the same
operator from stock torch ops and to the sequential restatement of tests/outlines_util.py, in one process.

    python tools/bench_plume_outlines.py [--rows 2000] [--cols 2300] [--blobs 300] [--bernoulli P] [--rounds 6] [--out profiles/plume_outlines.txt]

  (a)  the library stages with the scans and the sort between them (device events; every buffer allocated once, the edge, ring and
       vertex counts known: no read-back), plumes.component_outlines as it is called (its two read-backs included) and
       plumes.plume_outlines end to end (labelling, tracing, the read-back of the rings, the polygons; host clock + synchronise)
  (b)  stock torch ops on the device: shifted-label comparisons for the sides, nonzero for the edge list, a 4-plane id map for the
       successors, the same (smallest id, distance) pointer doubling as m = where(m[j] < m, ..), j = j[j] rounds, scatter_add_ for
       the areas, sort of the ring keys, index_put for the ring order, boolean indexing for the corners; its constant tensors are
       built once, outside the timed region
  (c)  the restatement (pure Python over numpy arrays) on the host, one run: a stated baseline, not a like-for-like comparison
(a) and (b) alternate in rounds of 10 calls after 10 warm-up calls each; the figure is the mean over all rounds, the spread the
minimum and maximum round.  The four result tensors of (a) and (b) are asserted equal to (c) before anything is timed.  The mask
is the seeded one of tools/bench_component_stats.py.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import outlines_util as U  # noqa: E402
from bench_component_stats import scene  # noqa: E402
from starcop_amd import _lib, mask_creation, plumes  # noqa: E402
from starcop_amd._lib import check, stream  # noqa: E402

FIELDS = plumes.OUTLINE_FIELDS


def torch_plan(H, W, dev):
    return {"step_r": torch.tensor([0, 1, 0, -1], device=dev), "step_c": torch.tensor([1, 0, -1, 0], device=dev),
            "idmap": torch.empty(H * W * 4, dtype=torch.int64, device=dev)}


def torch_outlines(L, connectivity, plan):
    """the four tensors of component_outlines(collinear=False) from stock torch ops"""
    H, W = L.shape
    dev = L.device
    P = torch.nn.functional.pad(L, (1, 1, 1, 1))
    fg = L > 0
    sides = torch.stack([fg & (P[:-2, 1:-1] != L), fg & (P[1:-1, 2:] != L), fg & (P[2:, 1:-1] != L), fg & (P[1:-1, :-2] != L)], -1)
    code = torch.nonzero(sides.reshape(-1))[:, 0]               # edge order: raster order of the pixel, then top, right, bottom, left
    E = code.numel()
    ids = torch.arange(E, device=dev)
    idmap = plan["idmap"]
    idmap[code] = ids
    pix, d = code // 4, code % 4
    r0, c0 = pix // W + (d >= 2), pix % W + ((d == 1) | (d == 2))
    r1, c1 = r0 + plan["step_r"][d], c0 + plan["step_c"][d]
    k = L.reshape(-1)[pix]
    nw, ne, sw, se = P[r1, c1], P[r1, c1 + 1], P[r1 + 1, c1], P[r1 + 1, c1 + 1]
    can = torch.stack([(se == k) & (ne != k), (sw == k) & (se != k), (nw == k) & (sw != k), (ne == k) & (nw != k)], 1)
    first, last = ((d + 3) % 4, (d + 1) % 4) if connectivity == 2 else ((d + 1) % 4, (d + 3) % 4)
    nd = torch.where(can.gather(1, first[:, None])[:, 0], first, torch.where(can.gather(1, d[:, None])[:, 0], d, last))
    succ = idmap[((r1 - (nd >= 2).long()) * W + c1 - ((nd == 1) | (nd == 2)).long()) * 4 + nd]
    m, off, j = ids, torch.zeros_like(ids), succ
    t = 0
    while True:                                                  # ceil(log2 E) + 1 rounds, as the library
        take = m[j] < m
        off = torch.where(take, off[j] + (1 << t), off)
        m = torch.where(take, m[j], m)
        j = j[j]
        t += 1
        if (1 << (t - 1)) >= E:
            break
    area2 = torch.zeros(E, dtype=torch.int64, device=dev).scatter_add_(0, m, c0 * r1 - c1 * r0)
    head = torch.nonzero(m == ids)[:, 0]
    key = torch.sort((k[head].long() << 33) | ((area2[head] < 0).long() << 32) | head).values
    head = key & 0xffffffff
    R = head.numel()
    ring_len = off[succ[head]] + 1
    ring_start = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    ring_start[1:] = torch.cumsum(ring_len, 0)
    rank = torch.empty(E, dtype=torch.int64, device=dev)
    rank[head] = torch.arange(R, device=dev)
    q = rank[m]
    at = ring_start[q] + torch.where(off == 0, 0, ring_len[q] - off)
    keep = torch.empty(E, dtype=torch.bool, device=dev)
    keep[succ] = d[succ] != d
    ordered = torch.empty((E, 2), dtype=torch.int32, device=dev)
    ordered[at] = torch.stack([r0, c0], 1).int()
    okeep = torch.empty(E, dtype=torch.bool, device=dev)
    okeep[at] = keep
    kp = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(okeep, 0)])
    return {"vertices": ordered[okeep], "ring_offsets": kp[ring_start], "ring_label": (key >> 33).int(), "ring_area2": area2[head]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--cols", type=int, default=2300)
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("--bernoulli", type=float, default=None, help="a Bernoulli(p) mask instead of the blobs")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    H, W = args.rows, args.cols
    if args.bernoulli is not None:                               # a noise mask: many edges, long rings
        mask = np.random.default_rng(20002300).random((H, W)) < args.bernoulli
    else:
        mask, _, _ = scene(H, W, args.blobs, seed=20002300)
    d_mask = torch.from_numpy(mask).cuda()
    labels, n = mask_creation.connected_components(d_mask)
    lab_h = labels.cpu().numpy()

    t = time.perf_counter()
    want = U.outlines_ref(lab_h, 2)
    cpu = (time.perf_counter() - t) * 1e3
    print(f"restatement done: {want['n_edges']} edges, {cpu:.0f} ms", flush=True)
    E, R, V = want["n_edges"], want["ring_label"].size, want["vertices"].shape[0]
    T = lib.sc_component_outlines_rounds(E)

    dev = labels.device
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)      # noqa: E731
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)      # noqa: E731
    wb = lib.sc_component_outlines_workspace_bytes(H, W, E)
    buf = {"cnt": i32(H * W), "prefix": i32(H * W), "work": torch.empty(wb, dtype=torch.uint8, device=dev), "keys": i64(E), "stats": i32(2),
           "ring_label": i32(R), "ring_area2": i64(R), "ring_len": i64(R), "ring_start": torch.zeros(R + 1, dtype=torch.int64, device=dev),
           "ordered": i32(2 * E), "ordered_keep": i32(E), "keep_prefix": i32(E), "vertices": torch.empty((V, 2), dtype=torch.int32, device=dev),
           "ring_offsets": i64(R + 1), "sorted_keys": i64(E)}
    a = _lib.sc_outline_args()
    a.labels, a.H, a.W, a.connectivity, a.E, a.R, a.V, a.work_bytes = labels.data_ptr(), H, W, 2, E, R, V, wb
    for f, tns in buf.items():
        setattr(a, f, tns.data_ptr())

    def run_a():
        check(lib.sc_component_outlines(a, _lib.OUTLINE_COUNT, stream()))
        torch.cumsum(buf["cnt"], 0, dtype=torch.int32, out=buf["prefix"])
        check(lib.sc_component_outlines(a, _lib.OUTLINE_TRACE, stream()))
        torch.sort(buf["keys"], out=(buf["sorted_keys"], run_a.order))
        check(lib.sc_component_outlines(a, _lib.OUTLINE_RINGS, stream()))
        torch.cumsum(buf["ring_len"], 0, out=buf["ring_start"][1:])
        check(lib.sc_component_outlines(a, _lib.OUTLINE_SCATTER, stream()))
        torch.cumsum(buf["ordered_keep"], 0, dtype=torch.int32, out=buf["keep_prefix"])
        check(lib.sc_component_outlines(a, _lib.OUTLINE_COMPACT, stream()))
    run_a.order = i64(E)

    plan = torch_plan(H, W, dev)

    def run_b():
        return torch_outlines(labels, 2, plan)

    def run_call():
        return plumes.component_outlines(labels, n)

    def events(fn, reps=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    run_a()
    tb_out = run_b()
    call_out = run_call()
    torch.cuda.synchronize()
    assert buf["stats"].tolist() == [R, V]
    for name, got in (("staged library call", buf), ("component_outlines", call_out), ("torch restatement", tb_out)):
        for f in FIELDS:
            assert np.array_equal(got[f].cpu().numpy(), want[f]), f"{name}: {f} disagrees with the restatement"
    print("results equal", flush=True)
    for fn in (run_a, run_b, run_call):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(args.rounds):
        ta.append(events(run_a))
        tb.append(events(run_b))
        tc.append(events(run_call))
    for _ in range(3):
        plumes.plume_outlines(d_mask)
    t = time.perf_counter()
    for _ in range(20):
        polys = plumes.plume_outlines(d_mask)
    torch.cuda.synchronize()
    e2e = (time.perf_counter() - t) / 20 * 1e3
    assert len(polys) == n

    # bytes the stages read and write, by their index arithmetic (neighbour loads of the labels counted once: they hit the cache)
    px = H * W * (4 + 4) + H * W * 8 + H * W * 12                         # count, scan of cnt, emit reads labels + cnt + prefix
    per_edge = 24 + T * (12 + 12 + 12) + (8 + 4 + 4 + 4 + 1 + 8) + (8 + 8) + 3 * 16 + (8 + 4 + 1 + 12) + (12 + 8) + 8
    moved = px + E * per_edge
    ma, mb, mc = float(np.mean(ta)), float(np.mean(tb)), float(np.mean(tc))
    lines = [
        f"plume outlines, {H} x {W} label image ({'blobs' if args.bernoulli is None else f'Bernoulli p = {args.bernoulli}'}), {n} components, connectivity 2: {E} edges, {R} rings ({int((want['ring_area2'] < 0).sum())} holes), "
        f"longest ring {want['longest']} edges, {V} corner vertices, {T} pointer-doubling rounds; {torch.cuda.get_device_name(0)} "
        f"({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; the four result tensors of (a) and (b) equal "
        f"the sequential restatement",
        f"(a) sc_component_outlines, 5 stages + 3 scans + 1 sort, {T + 7} kernel launches of its own, no read-back {ma:9.3f} ms per call   (rounds {min(ta):.3f} .. {max(ta):.3f})",
        f"(a) plumes.component_outlines (allocations and its two read-backs included) {mc:9.3f} ms per call   (rounds {min(tc):.3f} .. {max(tc):.3f})",
        f"(b) stock torch ops (shifted comparisons, nonzero, id map, where / gather doubling rounds, scatter_add_, sort) {mb:9.3f} ms per call   "
        f"(rounds {min(tb):.3f} .. {max(tb):.3f})   (b) / (a) = {mb / ma:.2f}, (b) / component_outlines = {mb / mc:.2f}",
        f"(a) end to end, plumes.plume_outlines: labelling + tracing + read-back + polygons (host clock, 20 calls) {e2e:9.3f} ms per call",
        f"(c) sequential restatement on the host (pure Python over numpy), one run {cpu:9.1f} ms   (c) / (a) = {cpu / ma:.0f}",
        f"(a) bytes by index arithmetic: per-pixel passes {px / 1e6:.1f} MB + {per_edge} B x {E} edges = {moved / 1e6:.1f} MB per call -> "
        f"{moved / (ma * 1e-3) / 1e12:.3f} TB/s",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
