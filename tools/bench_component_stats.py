"""Time of the per-component statistics of one orthorectified granule (sc_component_stats / plumes.plume_table) next to a
restatement with stock torch ops and to the scipy oracle, in one process.

    python tools/bench_component_stats.py [--rows 2000] [--cols 2300] [--blobs 300] [--rounds 6] [--out profiles/component_stats.txt]

  (a)  sc_component_stats: the library call alone (device events; labels, outputs and workspace allocated once), and
       plumes.plume_table end to end (labelling, the call, read-back, the DataFrame; host clock + synchronise)
  (b)  stock torch ops on the device, keyed by label: scatter_add_ for the counts, the coordinate sums and the fp64 sums,
       scatter_reduce_ (amin / amax) for the boxes, the first pixel, max, min and argmax -- floating-point atomics, one launch per
       statistic and plane; its index tensors are built once, outside the timed region, as (a)'s workspace is
  (c)  the oracle of tests/plumes_util.py (scipy.ndimage + math.fsum per component), the components dealt to 16 threads: a stated
       baseline, not a like-for-like comparison
(a) and (b) alternate in rounds of 10 calls after 10 warm-up calls each; the figure is the mean over all rounds, the spread the
minimum and maximum round.  The results are asserted equal before anything is timed.  Bytes: the box pass of (a) reads every label
once (its neighbour loads hit the cache), the walk reads the labels of every bounding box once and the planes and the mask where
the label matches.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import plumes_util as U  # noqa: E402
from starcop_amd import _lib, mask_creation, plumes  # noqa: E402
from starcop_amd._lib import check, ptr, stream  # noqa: E402


def scene(H, W, blobs, seed):
    """a seeded plume-like mask: ``blobs`` ellipses of 3 .. 40 pixels half-axis plus 0.01 % single pixels; two planes"""
    rng = np.random.default_rng(seed)
    mask = rng.random((H, W)) < 1e-4
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(blobs):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        a, b = rng.integers(3, 41, 2)
        y0, y1, x0, x1 = max(cy - a, 0), min(cy + a + 1, H), max(cx - b, 0), min(cx + b + 1, W)
        mask[y0:y1, x0:x1] |= ((yy[y0:y1, x0:x1] - cy) / a) ** 2 + ((xx[y0:y1, x0:x1] - cx) / b) ** 2 <= 1.0
    mag = (rng.standard_normal((H, W)) * 300 + np.where(mask, 600.0, 0.0)).astype(np.float32)
    mag[rng.random((H, W)) < 0.01] = np.nan                      # no-data pixels
    prob = rng.random((H, W)).astype(np.float32)
    return mask, mag, prob


def torch_plan(labels, W):
    dev = labels.device
    lab = labels.reshape(-1).long()
    idx = torch.arange(lab.numel(), device=dev)
    return lab, idx, idx // W, idx % W


def torch_component_stats(plan, n, planes, other):
    """-> the columns of sc_component_stats for one image from stock torch ops (row 0 is the background and is dropped)"""
    lab, idx, rows, cols = plan
    dev = lab.device
    big = torch.iinfo(torch.int64).max

    def sadd(src, dtype=torch.int64):
        return torch.zeros(n + 1, dtype=dtype, device=dev).scatter_add_(0, lab, src.to(dtype))[1:]

    def sred(src, how, init):
        return torch.full((n + 1,), init, dtype=src.dtype, device=dev).scatter_reduce_(0, lab, src, how, include_self=True)[1:]
    out = {"area": sadd(torch.ones_like(lab)), "sum_row": sadd(rows), "sum_col": sadd(cols), "n_other": sadd(other.reshape(-1) != 0),
           "row_min": sred(rows, "amin", big), "row_max": sred(rows, "amax", -1), "col_min": sred(cols, "amin", big),
           "col_max": sred(cols, "amax", -1), "first_pixel": sred(idx, "amin", big)}
    per = {f: [] for f in U.PLANE_FIELDS}
    for p in planes:
        v = p.reshape(-1)
        fin = torch.isfinite(v)
        nf = sadd(fin)
        none = nf == 0                                           # no finite value: NaN, NaN, -1
        per["n_finite"].append(nf)
        per["sum"].append(sadd(torch.where(fin, v, 0).double(), torch.float64))
        mx = torch.full((n + 1,), -float("inf"), device=dev).scatter_reduce_(0, lab, torch.where(fin, v, -float("inf")), "amax")
        per["max"].append(torch.where(none, float("nan"), mx[1:]))
        per["min"].append(torch.where(none, float("nan"), sred(torch.where(fin, v, float("inf")), "amin", float("inf"))))
        per["argmax"].append(torch.where(none, -1, sred(torch.where(fin & (v == mx[lab]), idx, big), "amin", big)))
    out.update({f: torch.stack(c, 1) for f, c in per.items()})
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
    lib = _lib.load()
    H, W = args.rows, args.cols
    mask, mag, prob = scene(H, W, args.blobs, seed=20002300)
    other = (np.random.default_rng(1).random((H, W)) < 0.5).astype(np.uint8)
    d_mask, d_other = torch.from_numpy(mask).cuda(), torch.from_numpy(other).cuda()
    d_planes = [torch.from_numpy(mag).cuda(), torch.from_numpy(prob).cuda()]
    labels, n = mask_creation.connected_components(d_mask)
    lab_h = labels.cpu().numpy()
    counts = torch.tensor([n], dtype=torch.int32, device="cuda")
    P = len(d_planes)

    # (c) first: the oracle is also what (a) and (b) are checked against before their times mean anything
    t = time.perf_counter()

    def part(j):                                                 # components j, j + 16, ..: relabelled 1 .. so each thread walks its own
        ks = np.arange(j + 1, n + 1, 16)
        remap = np.zeros(n + 1, dtype=np.int64)
        remap[ks] = np.arange(1, ks.size + 1)
        return ks, U.oracle_stats(remap[lab_h], ks.size, [mag, prob], other)
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(part, range(16)))
    cpu = (time.perf_counter() - t) * 1e3
    want = {f: np.zeros((n,) + parts[0][1][f].shape[1:], dtype=parts[0][1][f].dtype) for f in parts[0][1]}
    for ks, st in parts:
        for f in st:
            want[f][ks - 1] = st[f]

    out = {f: torch.empty((1, n), dtype=plumes._DTYPES.get(f, torch.int64), device="cuda") for f in plumes.COMPONENT_FIELDS}
    out.update({f: torch.empty((1, n, P), dtype=plumes._DTYPES.get(f, torch.int64), device="cuda") for f in plumes.PLANE_FIELDS})
    a = _lib.sc_cstats_args()
    a.labels, a.counts, a.N, a.H, a.W, a.M, a.P = labels.data_ptr(), counts.data_ptr(), 1, H, W, n, P
    for q, p in enumerate(d_planes):
        a.plane[q], a.plane_stride[q] = p.data_ptr(), H * W
    a.other, a.other_stride = d_other.data_ptr(), H * W
    for f, tns in out.items():
        setattr(a, f, tns.data_ptr())
    wb = lib.sc_component_stats_workspace_bytes(1, H, W, n, P)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")

    def run_a():
        check(lib.sc_component_stats(a, ptr(work), wb, stream()))

    plan = torch_plan(labels, W)

    def run_b():
        return torch_component_stats(plan, n, d_planes, d_other)

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
    torch.cuda.synchronize()
    tol = want["area"][:, None] * 2.0 ** -50 * want["sum_abs"]
    for name, got in (("sc_component_stats", {f: v[0] for f, v in out.items()}), ("torch restatement", tb_out)):
        for f in plumes.COMPONENT_FIELDS + ("n_finite", "argmax", "max", "min"):
            assert np.array_equal(got[f].cpu().numpy(), want[f], equal_nan=True), f"{name}: {f} disagrees with the oracle"
        assert (np.abs(got["sum"].cpu().numpy() - want["sum"]) <= tol).all(), f"{name}: sum disagrees with the oracle"
    for _ in range(10):
        run_a()
    for _ in range(10):
        run_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(events(run_a))
        tb.append(events(run_b))
    for _ in range(3):
        plumes.plume_table(d_mask, mag1c=d_planes[0], prob=d_planes[1], label_mask=d_other)
    t = time.perf_counter()
    for _ in range(20):
        table = plumes.plume_table(d_mask, mag1c=d_planes[0], prob=d_planes[1], label_mask=d_other)
    torch.cuda.synchronize()
    e2e = (time.perf_counter() - t) / 20 * 1e3
    assert len(table) == n

    box_px = int(((want["row_max"] - want["row_min"] + 1) * (want["col_max"] - want["col_min"] + 1)).sum())
    fg = int(want["area"].sum())
    moved = H * W * 4 + box_px * 4 + fg * (4 * P + 1)
    ma, mb = float(np.mean(ta)), float(np.mean(tb))
    lines = [
        f"per-component statistics, {H} x {W} label image, {n} components ({fg} foreground pixels, bounding boxes {box_px} pixels), "
        f"{P} float32 planes (1 % NaN in the first) and a uint8 mask; {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; (a) and (b) equal the scipy oracle in every "
        f"integer column, max, min and argmax, and their fp64 sums lie within area * 2^-50 * sum|x| of math.fsum",
        f"(a) sc_component_stats (library call, 5 launches) {ma:9.3f} ms per call   (rounds {min(ta):.3f} .. {max(ta):.3f})",
        f"(b) stock torch ops (scatter_add_ / scatter_reduce_ by label) {mb:9.3f} ms per call   (rounds {min(tb):.3f} .. {max(tb):.3f})   (b) / (a) = {mb / ma:.1f}",
        f"(a) end to end, plumes.plume_table: labelling + statistics + read-back + DataFrame (host clock, 20 calls) {e2e:9.3f} ms per call",
        f"(c) scipy oracle (find_objects + fsum per component, 16 threads), one run {cpu:9.1f} ms   (c) / (a) = {cpu / ma:.0f}",
        f"(a) bytes: labels once {H * W * 4 / 1e6:.1f} MB + labels of the boxes {box_px * 4 / 1e6:.1f} MB + planes and mask of the foreground "
        f"{fg * (4 * P + 1) / 1e6:.1f} MB = {moved / 1e6:.1f} MB per call -> {moved / (ma * 1e-3) / 1e12:.3f} TB/s",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
