"""Time of the anti-aliased downscale (sc_resize_aa through resample.resize_antialiased) of a flight line's 13 simulated Sentinel-2
bands from 5 m to 20 m with the sigmas of their own sampling distances, next to a stock-torch restatement in the same process and to
scipy on 16 processes.

    python tools/bench_resize.py [--lines 16384] [--samples 668] [--rounds 6] [--calls 10] [--out profiles/resize.txt]

Scene: seeded 13 x lines x samples float32 in [0, 100).  The results are checked first: the kernel against scipy's float64
gaussian_filter + zoom (the operator's definition, tests/resize_util.py; gate 4 * 2^-24 * max|x|), the torch restatement against the
same at 1e-4 relative.  Timing: device events around `calls` calls, `rounds` alternating rounds (kernel, torch, kernel, ..) after a
warm-up; the median round is reported with the range.  Bytes moved = the input read once + the float32 intermediate written and read
+ the output written; the rate is quoted next to the 4.25 / 4.70 TB/s of this project's access-pattern copy
(tools/membench/thin_pattern.hip).  scipy runs before the device is touched, one plane per process, float32 in and out."""
import argparse
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import resize_util as R  # noqa: E402

BANDS = ["B1", "B2", "B3", "B4", "B5", "B6", "B7", "B8", "B8A", "B9", "B10", "B11", "B12"]
_SCENE = None


def _scipy_plane(job):
    p, shape, sigma, dtype = job
    import scipy.ndimage as ndi
    x = _SCENE[p].astype(dtype)
    f = ndi.gaussian_filter(x, sigma, mode="constant", cval=0.0) if sigma > 0 else x
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return ndi.zoom(f, (shape[0] / x.shape[0], shape[1] / x.shape[1]), order=1, mode="constant", cval=0.0, grid_mode=True)


def main():
    global _SCENE
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=668)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    P, H, W = len(BANDS), args.lines, args.samples
    rng = np.random.default_rng(0)
    _SCENE = (rng.random((P, H, W), dtype=np.float32) * 100).astype(np.float32)

    from starcop_amd import aviris, resample                       # imports torch; the device is not touched before the pool has gone
    sig = aviris.sentinel_2_sigmas(BANDS, 5.0)
    shape = resample.output_shape_for((H, W), 5.0, 20.0)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
    say(f"scene {P} x {H} x {W} float32, 5 m -> 20 m = {shape[0]} x {shape[1]}, sigmas " + " ".join(f"{s:g}" for s in sig))

    ctx = multiprocessing.get_context("fork")
    with ctx.Pool(min(args.procs, P)) as pool:
        t0 = time.perf_counter()
        want = np.stack(pool.map(_scipy_plane, [(p, shape, float(sig[p]), np.float64) for p in range(P)]))
        t64 = time.perf_counter() - t0
        t0 = time.perf_counter()
        pool.map(_scipy_plane, [(p, shape, float(sig[p]), np.float32) for p in range(P)])
        t32 = time.perf_counter() - t0

    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(_SCENE).cuda()

    def hip():
        return resample.resize_antialiased(x, shape, sigma=sig, mode="constant", cval=0.0)

    groups = [(float(s), torch.tensor(np.flatnonzero(sig == s), device="cuda")) for s in np.unique(sig)]
    kernels = {s: torch.from_numpy(resample.gaussian_kernel(s)[0].astype(np.float32)).cuda() for s, _ in groups}
    out_t = torch.empty((P,) + shape, dtype=torch.float32, device="cuda")

    def stock():
        for s, idx in groups:
            v = x[idx][:, None]                                    # (n, 1, H, W)
            g = kernels[s]
            r = g.numel() // 2
            v = F.conv2d(v, g.view(1, 1, -1, 1), padding=(r, 0))
            v = F.conv2d(v, g.view(1, 1, 1, -1), padding=(0, r))
            out_t[idx] = F.interpolate(v, size=shape, mode="bilinear", align_corners=False)[:, 0]
        return out_t

    got = hip().cpu().numpy()
    M = float(_SCENE.max())
    worst = float(np.abs(got.astype(np.float64) - want).max())
    assert worst <= 4.0 * R.ULP * M, f"kernel differs from the scipy float64 oracle by {worst / (R.ULP * M):.2f} x 2^-24 M"
    say(f"checked: kernel vs scipy float64 oracle, worst {worst / (R.ULP * M):.3f} x 2^-24 M (gate 4)")
    rel = float(np.abs(stock().cpu().numpy().astype(np.float64) - want).max()) / M
    assert rel <= 1e-4, f"torch restatement differs from the oracle by {rel:.2e} of max|x|"
    say(f"checked: torch restatement vs the same oracle, worst {rel:.2e} of max|x| (gate 1e-4)")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls                    # ms per call

    for fn in (hip, stock):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    th, ts = [], []
    for _ in range(args.rounds):
        th.append(timed(hip))
        ts.append(timed(stock))
    nbytes = 4 * P * (H * W + 2 * shape[0] * W + shape[0] * shape[1])
    mh, ms = float(np.median(th)), float(np.median(ts))
    say(f"sc_resize_aa (2 launches, {P} planes): {mh:.3f} ms per call (rounds {min(th):.3f}-{max(th):.3f}), "
                 f"{nbytes / 1e6:.0f} MB moved, {nbytes / mh / 1e9:.2f} TB/s (access-pattern copy: 4.25 / 4.70 TB/s)")
    say(f"stock torch (conv2d x 2 + interpolate per sigma group): {ms:.3f} ms per call (rounds {min(ts):.3f}-{max(ts):.3f}), "
                 f"{ms / mh:.1f} x the kernel")
    say(f"scipy, one plane per process on {min(args.procs, P)} processes: float32 {t32 * 1e3:.0f} ms, float64 {t64 * 1e3:.0f} ms "
                 f"for the {P} planes ({t32 * 1e3 / mh:.0f} x the kernel at float32)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
