"""Time of one GLT orthorectification call (sc_glt_ortho / ortho.georeference) next to a restatement with stock torch ops and to
the numpy oracle, in one process.

    python tools/bench_glt_ortho.py [--planes 5] [--rounds 6] [--reps 200] [--out profiles/glt_ortho.txt]

Case: the realistic swath of tests/ortho_util.py (1280 x 1242 source -> 2000 x 2300 grid, rotated strip with a no-data border and
repeated source pixels), P float32 planes.
  (a)  sc_glt_ortho: the library call alone (device events; GLT on the device, output and counter allocated once), and
       ortho.georeference end to end with check=True (allocation, the call, the counter read-back; host clock + synchronise)
  (b)  stock torch ops on the device: where(valid, src[:, iy, ix], fill) with the mask and the clamped index tensors built once,
       outside the timed region, as (a)'s device GLT is
  (c)  the numpy oracle, one plane per thread of a pool of 16: a stated baseline, not a like-for-like comparison
(a) and (b) alternate in rounds of --reps calls (a timed window of tens of milliseconds) after 10 warm-up calls each; the figure
is the mean over all rounds, the spread the minimum and maximum round.  Bytes: the floor of the operation is the output written once plus the two GLT planes read once; the
source pixels read on top of it are counted once each (the gather's cache lines are fetched more than once in practice).
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

import ortho_util as U  # noqa: E402
from starcop_amd import _lib, ortho  # noqa: E402
from starcop_amd._lib import check, stream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    P, fill = args.planes, -9999.0
    rows, cols = 1280, 1242
    gx_np, gy_np = U.swath_glt(rows, cols)
    Ho, Wo = gx_np.shape
    rng = np.random.default_rng(1280)
    src_np = rng.standard_normal((P, rows, cols)).astype(np.float32)
    src = torch.from_numpy(src_np).cuda()
    gx, gy = torch.from_numpy(gx_np).cuda(), torch.from_numpy(gy_np).cuda()
    out = torch.empty((P, Ho, Wo), dtype=torch.float32, device="cuda")
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = _lib.sc_ortho_args()
    a.glt_x, a.glt_y, a.out_h, a.out_w, a.rows, a.cols = gx.data_ptr(), gy.data_ptr(), Ho, Wo, rows, cols
    a.P, a.elem_bytes, a.absolute = P, 4, 0
    fill_bits = int(np.array(fill, dtype=np.float32).reshape(1).view(np.uint32)[0])
    for p in range(P):
        a.src[p] = src[p].data_ptr()
        a.row_stride[p], a.col_stride[p] = src.stride(1), src.stride(2)
        a.fill_bits[p] = fill_bits
    a.out, a.oob_count = out.data_ptr(), oob.data_ptr()

    def run_a():
        check(lib.sc_glt_ortho(a, stream()))

    valid = (gx != 0) & (gy != 0)
    iy, ix = (gy.long() - 1).clamp_(min=0), (gx.long() - 1).clamp_(min=0)
    fill_t = torch.tensor(fill, dtype=torch.float32, device="cuda")

    def run_b():
        return torch.where(valid, src[:, iy, ix], fill_t)

    def events(fn, reps=args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    # (c) first: the oracle is also what (a) and (b) are checked against before their times mean anything
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        want = np.stack(list(ex.map(lambda p: U.oracle(src_np[p], gx_np, gy_np, fill), range(P))))
    cpu = (time.perf_counter() - t) * 1e3
    run_a()
    got_b = run_b()
    torch.cuda.synchronize()
    assert int(oob.item()) == 0
    assert U.same_bytes(out.cpu().numpy(), want), "sc_glt_ortho disagrees with the numpy oracle"
    assert U.same_bytes(got_b.cpu().numpy(), want), "torch restatement disagrees with the numpy oracle"
    del got_b
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
        ortho.georeference(src, gx, gy, fill_value_default=fill)
    t = time.perf_counter()
    for _ in range(20):
        res = ortho.georeference(src, gx, gy, fill_value_default=fill)
    torch.cuda.synchronize()
    e2e = (time.perf_counter() - t) / 20 * 1e3
    assert U.same_bytes(res.cpu().numpy(), want)

    n_valid = int(valid.sum().item())
    floor = out.numel() * 4 + 2 * gx.numel() * 4
    src_once = P * min(n_valid, rows * cols) * 4
    ma, mb = float(np.mean(ta)), float(np.mean(tb))
    lines = [
        f"GLT orthorectification, {P} float32 planes of a {rows} x {cols} swath ({src_np.nbytes / 1e6:.1f} MB) -> {Ho} x {Wo} grid, "
        f"{n_valid} of {Ho * Wo} pixels with data ({100.0 * n_valid / (Ho * Wo):.1f} %), fill -9999; "
        f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of {args.reps} calls after 10 warm-up calls each, device events; (a) and (b) are bit-equal to the numpy "
        f"oracle in all {out.numel()} values",
        f"(a) sc_glt_ortho (library call, one launch)      {ma * 1e3:9.1f} us per call   (rounds {min(ta) * 1e3:.1f} .. {max(ta) * 1e3:.1f})",
        f"(b) stock torch ops (index, where)              {mb * 1e3:9.1f} us per call   (rounds {min(tb) * 1e3:.1f} .. {max(tb) * 1e3:.1f})   "
        f"(b) / (a) = {mb / ma:.2f}",
        f"(a) end to end, ortho.georeference with check=True (host clock, 20 calls) {e2e * 1e3:9.1f} us per call",
        f"(c) numpy oracle, one plane per thread (16 threads), one run {cpu:9.1f} ms   (c) / (a) = {cpu / ma:.0f}",
        f"bytes: output written {out.numel() * 4 / 1e6:.1f} MB + GLT read {2 * gx.numel() * 4 / 1e6:.1f} MB = floor {floor / 1e6:.1f} MB -> "
        f"(a) {floor / (ma * 1e-3) / 1e12:.2f} TB/s against the floor; with every source pixel once (+{src_once / 1e6:.1f} MB) "
        f"{(floor + src_once) / (ma * 1e-3) / 1e12:.2f} TB/s",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
