"""Time of the mag1c window statistics of one flight line (sc_window_stats / sampling.window_stats) next to a restatement with
stock torch ops and to the CPU oracle loop, in one process.

    python tools/bench_window_stats.py [--rows 16384] [--cols 668] [--rounds 6] [--out profiles/window_stats.txt]

  (a)  sc_window_stats: the library call alone (device events; windows, outputs and workspace allocated once), and
       sampling.window_stats end to end (upload of the window list, the call, read-back, the DataFrame; host clock + synchronise)
  (b)  stock torch ops on the device: gather the windows of one shape into (n, h*w), replace what is not in the value set by +inf,
       torch.sort along the window, count, the ranks and numpy's float32 interpolation as tensor ops -- batched, no host round trip
       per window (a stronger baseline than a per-window loop); its index tensors and constants are built once, outside the
       timed region, as (a)'s window list and workspace are
  (c)  the CPU oracle loop of tests/winstats_util.py (the reference's numpy calls per window) on a pool of 16 threads: a stated
       baseline, not a like-for-like comparison
(a) and (b) alternate in rounds of 10 calls after 10 warm-up calls each; the figure is the mean over all rounds, the spread the
minimum and maximum round.  Bytes: every pass of (a) loads each window once, so a call issues 3 x (sum of window sizes) x 4 bytes
of loads out of a scene of rows x cols x 4 bytes that stays cache resident.
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

import winstats_util as U  # noqa: E402
from starcop_amd import _lib, sampling  # noqa: E402
from starcop_amd._lib import check, ptr, stream  # noqa: E402

PASSES = 3


def torch_plan(wins, dev):
    """index tensors of the restatement, built once per window list (outside any timed region): per window shape the row / column
    gather indices and the positions of its windows in the list"""
    groups = {}
    for i, (r, c, h, w) in enumerate(wins):
        groups.setdefault((h, w), []).append(i)
    plan = []
    for (h, w), idx in groups.items():
        r0 = torch.tensor([wins[i][0] for i in idx], device=dev)
        c0 = torch.tensor([wins[i][1] for i in idx], device=dev)
        rr = (r0[:, None] + torch.arange(h, device=dev)[None, :])[:, :, None]
        cc = (c0[:, None] + torch.arange(w, device=dev)[None, :])[:, None, :]
        plan.append((h, w, rr, cc, torch.tensor(idx, device=dev)))
    q32 = [torch.tensor(float(np.float32(q) / np.float32(100)), dtype=torch.float32, device=dev) for q in (1, 5, 95, 99)]
    consts = {"q32": q32, "inf": torch.tensor(float("inf"), device=dev), "zero": torch.zeros((), device=dev)}
    return plan, consts


def torch_window_stats(scene, plan, consts, n, fill, clip=10_000.):
    """-> (count int64 [n], sum float64 [n], stats float32 [n][7]) in window order, stock torch ops only, no host copies"""
    dev = scene.device
    count = torch.empty(n, dtype=torch.int64, device=dev)
    total = torch.empty(n, dtype=torch.float64, device=dev)
    stats = torch.empty((n, 7), dtype=torch.float32, device=dev)
    for h, w, rr, cc, ii in plan:
        v = scene[rr, cc].reshape(ii.numel(), h * w)
        ok = v >= 0
        if fill is not None:
            ok &= v != fill
        key = torch.where(ok, v.clamp(max=clip), consts["inf"])
        srt = torch.sort(key, dim=1).values
        cnt = ok.sum(1)
        out = torch.empty((ii.numel(), 7), dtype=torch.float32, device=dev)
        last = (cnt - 1).clamp(min=0)
        out[:, 0] = srt.gather(1, last[:, None])[:, 0]
        out[:, 1] = srt[:, 0]
        for j, q32 in zip((2, 3, 5, 6), consts["q32"]):
            # the quantile was rounded on the host: a device division by a scalar may multiply by the rounded reciprocal instead
            vi = (cnt - 1).to(torch.float32) * q32
            lo = vi.floor()
            t = vi - lo
            lo = lo.long().clamp(min=0)
            a = srt.gather(1, lo[:, None])[:, 0]
            b = srt.gather(1, torch.minimum(lo + 1, last)[:, None])[:, 0]
            d = b - a
            out[:, j] = torch.where(t >= .5, b - d * (1 - t), a + d * t)
        a = srt.gather(1, ((cnt - 1) // 2).clamp(min=0)[:, None])[:, 0]
        b = srt.gather(1, (cnt // 2).clamp(max=h * w - 1)[:, None])[:, 0]
        out[:, 4] = (a + b) / 2
        count[ii] = cnt
        total[ii] = torch.where(ok, key, consts["zero"]).double().sum(1)
        stats[ii] = out
    return count, total, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--cols", type=int, default=668)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    fill = -9999.
    scene_np = U.flightline_scene(H=args.rows, W=args.cols, seed=16384668)
    scene = torch.from_numpy(scene_np).cuda()
    wins = U.windows_flightline(scene_np.shape)
    n = len(wins)
    wins_np = np.array(wins, dtype=np.int32)
    wins_d = torch.from_numpy(wins_np).cuda()
    count = torch.empty(n, dtype=torch.int64, device="cuda")
    sum_mean = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    stats = torch.empty((n, 7), dtype=torch.float32, device="cuda")
    wb = lib.sc_window_stats_workspace_bytes(n)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    a = _lib.sc_winstats_args()
    a.x, a.row_stride, a.H, a.W = scene.data_ptr(), scene.stride(0), args.rows, args.cols
    a.has_fill, a.fill, a.clip_max, a.n_win = 1, fill, 10_000., n
    a.windows, a.windows_host = wins_d.data_ptr(), wins_np.ctypes.data
    a.count, a.sum_mean, a.stats = count.data_ptr(), sum_mean.data_ptr(), stats.data_ptr()

    def run_a():
        check(lib.sc_window_stats(a, ptr(work), wb, stream()))

    plan, consts = torch_plan(wins, scene.device)

    def run_b():
        return torch_window_stats(scene, plan, consts, n, fill)

    def events(fn, reps=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    # (c) first: the CPU oracle on 16 threads is also what (a) and (b) are checked against before their times mean anything
    chunks = [wins[i::16] for i in range(16)]
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(lambda ws: U.oracle_rows(scene_np, ws, fill=fill), chunks))
    cpu = (time.perf_counter() - t) * 1e3
    by = {(r["window_row_off"], r["window_col_off"]): r for p in parts for r in p}
    assert len(by) == n, "a window of the benchmark scene is empty"
    want = np.array([[by[(w[0], w[1])][c] for c in U.F32_COLUMNS] for w in wins], dtype=np.float32)
    want_count = np.array([by[(w[0], w[1])]["count"] for w in wins])
    run_a()
    cb, sb, stb = run_b()
    torch.cuda.synchronize()
    assert np.array_equal(count.cpu().numpy(), want_count) and np.array_equal(U.bits(stats.cpu().numpy()), U.bits(want)), \
        "sc_window_stats disagrees with the CPU oracle"
    differ = int((U.bits(stb.cpu().numpy()) != U.bits(want)).sum())
    assert np.array_equal(cb.cpu().numpy(), want_count), "torch restatement: counts disagree with the CPU oracle"
    assert ((sum_mean[:, 0] - sb).abs() <= 1e-12 * sb).all()
    for _ in range(10):
        run_a()
    for _ in range(10):
        run_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(events(run_a))
        tb.append(events(run_b))
    # end to end through the Python surface
    for _ in range(3):
        sampling.window_stats(scene, fill_value=fill)
    t = time.perf_counter()
    for _ in range(20):
        table = sampling.window_stats(scene, fill_value=fill)
    torch.cuda.synchronize()
    e2e = (time.perf_counter() - t) / 20 * 1e3
    assert len(table) == n

    win_bytes = int(sum(w[2] * w[3] for w in wins)) * 4
    ma, mb = float(np.mean(ta)), float(np.mean(tb))
    lines = [
        f"mag1c window statistics, {args.rows} x {args.cols} float32 scene ({scene_np.nbytes / 1e6:.1f} MB), {n} windows of 512 x 512 at "
        f"overlap 256 ({win_bytes / 1e6:.1f} MB of window pixels), fill -9999, clip 10000; {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; (a) is bit-equal to the CPU oracle in all "
        f"{stats.numel()} float32 statistics and the counts, (b) in {stats.numel() - differ} of them and the counts",
        f"(a) sc_window_stats (library call)        {ma:9.3f} ms per call   (rounds {min(ta):.3f} .. {max(ta):.3f})",
        f"(b) stock torch ops (gather, sort, index) {mb:9.3f} ms per call   (rounds {min(tb):.3f} .. {max(tb):.3f})   (b) / (a) = {mb / ma:.1f}",
        f"(a) end to end, sampling.window_stats -> DataFrame (host clock, 20 calls) {e2e:9.3f} ms per call",
        f"(c) CPU oracle loop (numpy per window, 16 threads), one run {cpu:9.1f} ms   (c) / (a) = {cpu / ma:.0f}",
        f"(a) loads issued: {PASSES} passes x {win_bytes / 1e6:.1f} MB = {PASSES * win_bytes / 1e6:.1f} MB per call -> "
        f"{PASSES * win_bytes / (ma * 1e-3) / 1e12:.2f} TB/s of window loads; scene bytes x passes = "
        f"{PASSES * scene_np.nbytes / 1e6:.1f} MB -> {PASSES * scene_np.nbytes / (ma * 1e-3) / 1e12:.2f} TB/s",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
