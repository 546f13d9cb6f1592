"""Stage times of the Sanchez-Garcia MLR ratio (sc_mlr_*) at batch 16 x 512^2, k = 5 and 9, both registry divisions, each next
to its algorithmic byte floor at ~6 TB/s of achievable HBM bandwidth.  Device-event timing after warm-up.

    python tools/bench_mlr.py [--batch 16] [--size 512] [--reps 50]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from starcop_amd import _lib, features  # noqa: E402
from starcop_amd._lib import check, ptr, stream  # noqa: E402

HBM = 6.0e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    B, H = args.batch, args.size
    n = H * H
    rng = np.random.default_rng(0)
    plane = B * n * 4
    rows = []
    for k in (5, 9):
        alb = rng.uniform(0.1, 0.3, size=(B, 1, H, H)).astype(np.float32)
        x = torch.from_numpy(alb * rng.uniform(0.6, 1.4, size=(1, k + 1, 1, 1)).astype(np.float32)
                             + 0.02 * rng.standard_normal((B, k + 1, H, H)).astype(np.float32)).to("cuda")   # (B, k+1, H, W)
        a, keep, _ = features._mlr_operands([x[:, j] for j in range(k)], x[:, k])
        wb = lib.sc_mlr_workspace_bytes(B, n, k)
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        coef = torch.empty((B, k + 1), dtype=torch.float64, device="cuda")
        r = torch.empty((B, n), dtype=torch.float32, device="cuda")
        out = torch.empty((B, n), dtype=torch.float32, device="cuda")
        tdense = x[:, k].contiguous()
        tw = lib.sc_trimmed_sum_workspace_bytes(B)
        twork = torch.empty(tw, dtype=torch.uint8, device="cuda")
        sums = torch.empty(B, dtype=torch.float64, device="cuda")
        ar = C.byref(a)
        check(lib.sc_mlr_fit(ar, ptr(coef), ptr(work), wb, stream()))
        check(lib.sc_mlr_predict(ar, ptr(coef), ptr(r), stream()))
        stages = [
            ("moments", lambda: check(lib.sc_mlr_moments(ar, ptr(work), wb, stream())), (k + 1) * plane),
            ("solve", lambda: check(lib.sc_mlr_solve(ar, ptr(coef), ptr(work), wb, stream())), 0),
            ("predict", lambda: check(lib.sc_mlr_predict(ar, ptr(coef), ptr(r), stream())), (k + 1) * plane),
            ("trimmed sums (t, r)", lambda: (check(lib.sc_trimmed_sums(ptr(tdense), B, n, 5.0, ptr(sums), ptr(twork), tw, stream())),
                                             check(lib.sc_trimmed_sums(ptr(r), B, n, 5.0, ptr(sums), ptr(twork), tw, stream()))),
             2 * plane),
            ("ratio c_matched (incl. trimmed sums)",
             lambda: check(lib.sc_mlr_ratio(ar, ptr(coef), ptr(r), _lib.MLR_C_MATCHED, 0, ptr(out), ptr(work), wb, stream())),
             5 * plane),
            ("ratio simple_plus (2 passes, r fused)",
             lambda: check(lib.sc_mlr_ratio(ar, ptr(coef), None, _lib.MLR_SIMPLE_PLUS, 0, ptr(out), ptr(work), wb, stream())),
             (2 * (k + 1) + 1) * plane),
            ("end to end c_matched_outliers", lambda: features.ratio_MLR_local([x[:, j] for j in range(k)], x[:, k]),
             ((k + 1) + (k + 2) + 5) * plane),
            ("end to end simple_plus", lambda: features.ratio_MLR_local([x[:, j] for j in range(k)], x[:, k], division="simple_plus"),
             ((k + 1) + 2 * (k + 1) + 1) * plane),
        ]
        for name, fn, nbytes in stages:
            us = timed(fn, args.reps)
            floor = nbytes / HBM * 1e6
            rows.append((k, name, us, floor))
            print(f"k={k}  {name:40s} {us:9.1f} us   floor {floor:7.1f} us  ({nbytes / 1e6:6.1f} MB)", flush=True)
        del keep
    print(f"\n| k | stage (batch {B} x {H}^2) | time (us) | byte floor at 6 TB/s (us) |\n|---|---|---|---|")
    for k, name, us, floor in rows:
        print(f"| {k} | {name} | {us:.1f} | {floor:.1f} |")


if __name__ == "__main__":
    main()
