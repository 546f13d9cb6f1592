"""Time of cutting the sampled windows of one flight line (sc_window_cut) next to a restatement with stock torch ops and to the
numpy restatement, in one process.

    python tools/bench_window_cut.py [--rows 16384] [--cols 668] [--rounds 6] [--out profiles/window_cut.txt]

Input: a seeded rows x cols flight line of 29 float32 planes (mag1c: nodata -> 0 and a clip; 16 simulated bands: nodata, the
float32 multiply and a clip to [0, 2]; 12 AVIRIS bands: nodata and the multiply) plus a chunky uint8 (rows, cols, 4) label_rgba, and
24 windows of 512 x 512 of which some hang over the edges of the flight line.
  (a)  sc_window_cut: the library call alone, one launch for the 29 float32 planes and one for the four uint8 planes (device
       events; window tables and outputs allocated once).  The call reads its device window table back before the launch (192 bytes
       here), which is inside the time
  (b)  stock torch ops on the device: one advanced-indexing gather of all planes and windows with clamped indices, torch.where for
       what the flight line does not hold and for nodata, the multiply and torch.clamp on the planes that have them -- batched, no
       host round trip; its index tensors and constants are built once, outside the timed region
  (c)  the numpy restatement of tests/window_cut_util.py on a pool of 16 threads: a stated baseline, not like for like
(a) and (b) alternate in rounds of 10 calls after 10 warm-up calls each; the figure is the mean over all rounds, the spread the
minimum and maximum round.  The three results are asserted equal before anything is timed.  Bytes per call: every output element
is written once and every element of the flight line under a window is read once per window that holds it.
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

import window_cut_util as U  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import check, stream  # noqa: E402

NF, HW = 29, 512
FILL = -9999.0


def plane_ops(k):
    """(scale, clip) of float32 plane k: 0 mag1c, 1..16 simulated bands, 17..28 AVIRIS bands"""
    if k == 0:
        return None, (0.0, 10000.0)
    if k <= 16:
        return 3.2 / 100 / (0.08 + 0.11 * k), (0.0, 2.0)
    return 3.2, None


def windows(rows, cols, n=24):
    """n windows of HW x HW spread over the flight line: the first and last hang over its upper / lower edge, every third one over
    its left or right edge, the column offsets take every residue mod 4"""
    offs = []
    for i in range(n):
        r = -HW // 3 + i * (rows - HW // 3) // (n - 1)
        c = (0, cols - HW, -37, cols - HW + 90, 41, 78)[i % 6] + i % 4
        offs.append((r, c))
    return offs


def fill_args(a, planes, offs_d, offs, scene, out, ops):
    a.scene_rows, a.scene_cols, a.out_h, a.out_w = scene[0], scene[1], HW, HW
    a.P, a.elem_bytes, a.n_win = len(planes), planes[0].element_size(), offs.shape[0]
    a.win_off, a.win_off_host = offs_d.data_ptr(), offs.ctypes.data
    for k, t in enumerate(planes):
        a.src[k] = t.data_ptr()
        a.row_stride[k], a.col_stride[k] = t.stride()
        a.rows[k], a.cols[k] = t.shape
        scale, clip = ops[k]
        a.ops[k] = (_lib.WCUT_FILL if t.dtype == torch.float32 else 0) | (_lib.WCUT_SCALE if scale is not None else 0) | \
                   (_lib.WCUT_CLIP if clip is not None else 0)
        a.fill_bits[k] = int(np.array(FILL, np.float32).view(np.uint32)) if t.dtype == torch.float32 else 0
        if scale is not None:
            a.scale[k] = float(np.float32(scale))
        if clip is not None:
            a.clip_lo[k], a.clip_hi[k] = clip
    a.out = out.data_ptr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--cols", type=int, default=668)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    H, W = args.rows, args.cols
    rng = np.random.default_rng(16384668)
    cube_np = rng.random((NF, H, W), dtype=np.float32) * np.float32(40)
    cube_np[0] *= np.float32(400)
    holes = rng.random((H, W)) < .03
    cube_np[:, holes] = np.float32(FILL)
    rgba_np = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    offs = np.array(windows(H, W), dtype=np.int32)
    n = offs.shape[0]
    cube, rgba, offs_d = torch.from_numpy(cube_np).cuda(), torch.from_numpy(rgba_np).cuda(), torch.from_numpy(offs).cuda()
    ops_f = [plane_ops(k) for k in range(NF)]
    out_f = torch.empty((n, NF, HW, HW), dtype=torch.float32, device="cuda")
    out_u = torch.empty((n, 4, HW, HW), dtype=torch.uint8, device="cuda")
    af, au = _lib.sc_wcut_args(), _lib.sc_wcut_args()
    fill_args(af, [cube[k] for k in range(NF)], offs_d, offs, (H, W), out_f, ops_f)
    fill_args(au, [rgba[:, :, k] for k in range(4)], offs_d, offs, (H, W), out_u, [(None, None)] * 4)

    def run_a():
        check(lib.sc_window_cut(af, stream()))
        check(lib.sc_window_cut(au, stream()))

    # (b): built once
    ar = torch.arange(HW, device="cuda")
    rr, cc = offs_d[:, 0, None].long() + ar, offs_d[:, 1, None].long() + ar                  # (n, HW)
    inside = ((rr >= 0) & (rr < H))[:, None, :, None] & ((cc >= 0) & (cc < W))[:, None, None, :]
    rr_c, cc_c = rr.clamp(0, H - 1)[:, None, :, None], cc.clamp(0, W - 1)[:, None, None, :]
    pf, pu = torch.arange(NF, device="cuda")[None, :, None, None], torch.arange(4, device="cuda")[None, :, None, None]
    scales = torch.tensor([np.float32(s if s is not None else 1.0) for s, _ in ops_f], dtype=torch.float32, device="cuda")[None, :, None, None]
    zero_f, zero_u = torch.zeros((), device="cuda"), torch.zeros((), dtype=torch.uint8, device="cuda")
    rgba_planes = rgba.permute(2, 0, 1)                                                       # a view: (4, H, W)

    def run_b():
        v = cube[pf, rr_c, cc_c]
        v = torch.where(inside & (v != FILL), v, zero_f)
        v[:, 1:] *= scales[:, 1:]
        v[:, 0].clamp_(0.0, 10000.0)
        v[:, 1:17].clamp_(0.0, 2.0)
        u = torch.where(inside, rgba_planes[pu, rr_c, cc_c], zero_u)
        return v, u

    def events(fn, reps=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    # (c) first: it is also what (a) and (b) are checked against before their times mean anything
    def cpu_window(i):
        win = (int(offs[i, 0]), int(offs[i, 1]), HW, HW)
        f = np.stack([U.cut(cube_np[k], win, (0, 0), FILL, *ops_f[k]) for k in range(NF)])
        u = np.stack([U.cut(rgba_np[:, :, k], win) for k in range(4)])
        return f, u
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(cpu_window, range(n)))
    cpu = (time.perf_counter() - t) * 1e3
    want_f, want_u = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    del parts
    run_a()
    vb, ub = run_b()
    torch.cuda.synchronize()
    assert U.equal(out_f.cpu().numpy(), want_f) and U.equal(out_u.cpu().numpy(), want_u), "sc_window_cut disagrees with the numpy restatement"
    assert U.equal(vb.cpu().numpy(), want_f) and U.equal(ub.cpu().numpy(), want_u), "the torch restatement disagrees with the numpy restatement"
    del vb, ub, want_f, want_u
    for _ in range(10):
        run_a()
    for _ in range(10):
        run_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(events(run_a))
        tb.append(events(run_b))

    held = sum(max(0, min(r + HW, H) - max(r, 0)) * max(0, min(c + HW, W) - max(c, 0)) for r, c in offs.tolist())
    written = n * HW * HW * (NF * 4 + 4)
    read = held * (NF * 4 + 4)
    ma, mb = float(np.mean(ta)), float(np.mean(tb))
    lines = [
        f"window cutting, {H} x {W} flight line: {NF} float32 planes ({cube_np.nbytes / 1e6:.0f} MB) + chunky uint8 label_rgba "
        f"({rgba_np.nbytes / 1e6:.0f} MB), {n} windows of {HW} x {HW} ({held / (n * HW * HW) * 100:.0f} % of their pixels on the flight line); "
        f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; (a), (b) and (c) are equal in all "
        f"{n * (NF + 4) * HW * HW} elements",
        f"(a) sc_window_cut, 2 launches (float32, uint8)  {ma:9.3f} ms per call   (rounds {min(ta):.3f} .. {max(ta):.3f})",
        f"(b) stock torch ops (gather, where, mul, clamp) {mb:9.3f} ms per call   (rounds {min(tb):.3f} .. {max(tb):.3f})   (b) / (a) = {mb / ma:.1f}",
        f"(c) numpy restatement, 16 threads, one run      {cpu:9.1f} ms   (c) / (a) = {cpu / ma:.0f}",
        f"(a) bytes per call: {written / 1e6:.1f} MB written + {read / 1e6:.1f} MB read = {(written + read) / 1e6:.1f} MB -> "
        f"{(written + read) / (ma * 1e-3) / 1e12:.2f} TB/s   ((b) at the same byte count: {(written + read) / (mb * 1e-3) / 1e12:.2f} TB/s)",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
