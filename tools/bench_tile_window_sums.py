"""Time and memory of the label sums behind the tiled training table: sc_tile_window_sums next to the float64 integral image that
``ResidentTileSet.tiled_table`` used before it, in one process.

    python tools/bench_tile_window_sums.py [--tiles 256] [--size 512] [--rounds 6] [--out profiles/tile_window_sums.txt]

Input: ``tiles`` seeded {0, 1} float32 label tiles of size x size and the training grid create_windows((size, size), (128, 128),
(64, 64)) (49 windows at 512).
  (a)  sc_tile_window_sums: the library call alone (window table uploaded and the (M, K) output allocated once)
  (b)  the integral image with stock torch ops: labels.double(), two cumsums into a zero-padded (M, H+1, W+1) float64 array and
       four fancy-indexed look-ups per window; its index tensors are built once, outside the timed region
(a) and (b) alternate in rounds of 10 calls after 10 warm-up calls each (device events); the figure is the mean over all rounds,
the spread the minimum and maximum round.  The two results are asserted equal before anything is timed.  Memory: the growth of
torch.cuda.max_memory_allocated over one call of datamodule.tile_window_sums (which allocates its table and output) and over one
call of (b).  Bytes of (a): every label element once (the tile) and once per window that covers it (what the kernel requests).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from starcop_amd import _lib, datamodule as dm  # noqa: E402
from starcop_amd._lib import check, ptr, stream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    M, S = args.tiles, args.size
    rng = np.random.default_rng(256512)
    lab = torch.from_numpy((rng.random((M, S, S), dtype=np.float32) < np.float32(0.2)).astype(np.float32)).cuda()
    wins = dm.create_windows((S, S), (128, 128), (64, 64))
    K = len(wins)
    win = np.ascontiguousarray(np.asarray(wins, dtype=np.int32))
    win_d = torch.from_numpy(win).cuda()
    out = torch.empty((M, K), dtype=torch.float64, device="cuda")

    def run_a():
        check(lib.sc_tile_window_sums(ptr(lab), M, S, S, ptr(win_d), win.ctypes.data, K, ptr(out), stream()))

    r = torch.tensor([w[0] for w in wins], device="cuda")
    c = torch.tensor([w[1] for w in wins], device="cuda")
    k = torch.arange(K, device="cuda")

    def run_b():
        ii = torch.zeros((M, S + 1, S + 1), dtype=torch.float64, device="cuda")
        ii[:, 1:, 1:] = lab.double().cumsum(1).cumsum(2)
        return ii[:, r + 128][:, k, c + 128] - ii[:, r][:, k, c + 128] - ii[:, r + 128][:, k, c] + ii[:, r][:, k, c]

    def events(fn, reps=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    def growth(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del res
        return peak

    run_a()
    want = run_b()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "sc_tile_window_sums disagrees with the integral image"
    assert torch.equal(dm.tile_window_sums(lab, wins), want)
    del want
    mem_a = growth(lambda: dm.tile_window_sums(lab, wins))
    mem_b = growth(run_b)
    for _ in range(10):
        run_a()
    for _ in range(10):
        run_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(events(run_a))
        tb.append(events(run_b))
    ma, mb = float(np.mean(ta)), float(np.mean(tb))
    tile_bytes = M * S * S * 4
    req_bytes = M * sum(h * w for (_, _, h, w) in wins) * 4
    lines = [
        f"label sums of the training windows: {M} tiles of {S} x {S} float32 {{0, 1}} labels ({tile_bytes / 1e6:.0f} MB), {K} windows of "
        f"128 x 128 at stride 64; {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; (a) and (b) are equal in all {M * K} sums",
        f"(a) sc_tile_window_sums, 1 launch                     {ma:9.3f} ms per call   (rounds {min(ta):.3f} .. {max(ta):.3f})",
        f"(b) float64 integral image with stock torch ops       {mb:9.3f} ms per call   (rounds {min(tb):.3f} .. {max(tb):.3f})   (b) / (a) = {mb / ma:.1f}",
        f"(a) bytes per call: {tile_bytes / 1e6:.1f} MB of labels, each read once per covering window = {req_bytes / 1e6:.1f} MB requested -> "
        f"{tile_bytes / (ma * 1e-3) / 1e12:.2f} TB/s of distinct bytes, {req_bytes / (ma * 1e-3) / 1e12:.2f} TB/s of requested bytes",
        f"peak device memory above the resident labels, one call: (a) {mem_a} bytes (the (M, K) float64 output is {M * K * 8}, the window "
        f"table {K * 16}; the allocator rounds each to 512)   (b) {mem_b} bytes = {mem_b / 1e9:.2f} GB",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
