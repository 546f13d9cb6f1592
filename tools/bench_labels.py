"""Times of the plume label mask (sc_proposed_mask) and of connected-component labelling (sc_connected_components) next to
their byte floors at ~6 TB/s of achievable HBM bandwidth, and scipy's CPU time for the same work.  Device-event timing after
warm-up (the library calls only: no allocation, no host copies inside the timed loop).

    python tools/bench_labels.py [--reps 30]

Byte floors: proposed_mask reads mag1c (4 B/px) and alpha (1 B/px) and writes the mask (1 B/px): 6 B/px;
connected_components reads the mask (1 B/px) and writes int32 labels (4 B/px): 5 B/px.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import labels_util as lu  # noqa: E402
from starcop_amd import _lib  # noqa: E402
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


def cpu_ms(fn, reps=2):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    from scipy import ndimage
    rng = np.random.default_rng(0)
    rows = []

    for B, H, W in [(16, 512, 512), (1, 1280, 1242), (1, 700, 8000)]:
        fields = [lu.plume_field(rng, H, W, blobs=max(4, (H * W) // 30000)) for _ in range(B)]
        mag = torch.from_numpy(np.stack([f[0] for f in fields])).cuda()          # (B, 1, H, W)
        rgba_np = np.stack([f[1] for f in fields])
        rgba = torch.from_numpy(rgba_np).cuda()                                   # (B, 4, H, W): alpha read in place
        out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
        wb = lib.sc_label_workspace_bytes(B, H, W)
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        alpha = rgba[:, 3]

        def run():
            check(lib.sc_proposed_mask(ptr(mag), H * W, ptr(alpha), 4 * H * W, 200.0, _lib.SE_CROSS, ptr(out), ptr(work), wb,
                                       B, H, W, stream()))
        us = timed(run, args.reps)
        px = B * H * W
        cpu = cpu_ms(lambda: [lu.proposed_mask(rgba_np[i], f[0]) for i, f in enumerate(fields)])
        rows.append((f"proposed_mask {B} x {H} x {W}", us, 6 * px / HBM * 1e6, 6 * px, cpu))

    for conn, dens in ((2, 0.41), (1, 0.59)):
        for B, H, W in [(16, 512, 512), (1, 700, 8000)]:
            m_np = rng.uniform(size=(B, H, W)) < dens
            m = torch.from_numpy(m_np.astype(np.uint8)).cuda()
            lab = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
            cnt = torch.empty(B, dtype=torch.int32, device="cuda")
            wb = lib.sc_label_workspace_bytes(B, H, W)
            work = torch.empty(wb, dtype=torch.uint8, device="cuda")

            def run():
                check(lib.sc_connected_components(ptr(m), conn, ptr(lab), ptr(cnt), ptr(work), wb, B, H, W, stream()))
            us = timed(run, args.reps)
            px = B * H * W
            st = np.ones((3, 3)) if conn == 2 else None
            cpu = cpu_ms(lambda: [ndimage.label(m_np[i], structure=st) for i in range(B)])
            rows.append((f"connected_components conn={conn} density {dens} {B} x {H} x {W}", us, 5 * px / HBM * 1e6, 5 * px, cpu))

    for name, us, floor, nbytes, cpu in rows:
        print(f"{name:58s} {us:9.1f} us   floor {floor:7.1f} us  ({nbytes / 1e6:6.1f} MB)   scipy {cpu:8.1f} ms", flush=True)
    print("\n| call | time (us) | byte floor at 6 TB/s (us) | x floor | scipy CPU (ms) |\n|---|---|---|---|---|")
    for name, us, floor, nbytes, cpu in rows:
        print(f"| {name} | {us:.1f} | {floor:.1f} | {us / floor:.1f} | {cpu:.1f} |")


if __name__ == "__main__":
    main()
