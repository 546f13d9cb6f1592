"""Time of the exact order statistics per labelled component (sc_component_quantiles / plumes.component_quantiles,
component_median_mad) next to the same numbers from stock torch ops and from numpy, in one process.

    python tools/bench_component_quantiles.py [--rounds 6] [--out profiles/component_quantiles.txt]

Three label images, one float32 plane each (both signs, 1 % NaN):
  rings   the background rings (ring_px=16, gap_px=2) of the seeded 2000 x 2300 plume mask of tools/bench_component_stats.py:
          large, sparse, interleaved segments
  plumes  the plume labels of that mask: compact segments
  noise   the 1000 x 1000 Bernoulli-0.62 mask of tools/bench_plume_outlines.py: tens of thousands of components of a few pixels
Timed per image:
  (a1) sc_component_quantiles for ("median",), (a3) for (5, "median", 95): the library call alone (labels, outputs and workspace
       allocated once)
  (b)  plumes.component_median_mad: two calls through the Python layer, its allocations included
  (c1) / (c3) the numbers of (a1) / (a3) from stock torch ops: the monotone keys of the labelled finite pixels, ONE torch.sort of the
       composite keys label * 2^32 + key, indexing at the ranks and the float32 interpolation; the pixel index list, the segment
       starts and the ranks are built once, outside the timed region.  The MAD is not restated this way (it would be a second sort)
  (d)  numpy: np.percentile / np.median per component on the float32 values, the pixels grouped by one stable argsort; one run
(a1), (a3), (b), (c1), (c3) alternate in rounds of 10 calls after 10 warm-up calls each; device events; the figure is the mean over
all rounds, the spread the minimum and maximum round.  Every result is asserted equal to (d) before anything is timed (a zero may
have either sign).  Bytes of (a), by index arithmetic: both gather passes read every label and the plane where the label names a
row, the scatter writes a key per member, the small path reads its keys once, the large path four times; 12 bytes of state and the
outputs per row.
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
Q1, Q3 = ("median",), (5, "median", 95)


def numpy_rows(lab, n, plane, q):
    """np.percentile / np.median per component, the labelled pixels grouped by one stable argsort -> (n_finite (n,), (n, Q))"""
    lab, plane = lab.reshape(-1), plane.reshape(-1)
    idx = np.flatnonzero((lab >= 1) & (lab <= n))
    order = np.argsort(lab[idx], kind="stable")
    vals, bounds = plane[idx[order]], np.searchsorted(lab[idx[order]], np.arange(1, n + 2))
    nf, out = np.zeros(n, np.int64), np.full((n, len(q)), np.nan, np.float32)
    for k in range(n):
        t = vals[bounds[k]:bounds[k + 1]]
        t = t[np.isfinite(t)]
        nf[k] = t.size
        if t.size:
            out[k] = [np.median(t) if isinstance(v, str) else np.percentile(t, v) for v in q]
    return nf, out


class TorchSort:
    """(c): the order statistics from one torch.sort of composite keys; everything that does not depend on the values of the call is
    built here"""

    def __init__(self, labels, n, plane, q):
        lab, flat = labels.reshape(-1), plane.reshape(-1)
        self.flat = flat
        self.idx = torch.nonzero((lab >= 1) & (lab <= n) & torch.isfinite(flat)).reshape(-1)
        self.hi = lab[self.idx].long() << 32
        cnt = torch.bincount(lab[self.idx].long(), minlength=n + 1)[1:]
        start = torch.cumsum(cnt, 0) - cnt
        self.cnt, self.some = cnt, cnt > 0
        last = (cnt - 1).clamp(min=0)
        lo, hi, g, self.median = [], [], [], []
        for v in q:
            if isinstance(v, str):
                lo.append(last // 2), hi.append(cnt // 2), g.append(torch.zeros(n, device=lab.device)), self.median.append(True)
                continue
            vi = last.float() * float(np.float32(v) / np.float32(100))
            f = torch.floor(vi)
            a = torch.minimum(f.long(), last)
            lo.append(a), hi.append(torch.minimum(a + 1, last)), g.append(torch.where(cnt > 1, vi - f, 0.0)), self.median.append(False)
        self.lo = (torch.stack(lo, 1) + start[:, None]).clamp(max=max(self.idx.numel() - 1, 0))
        self.hi_r = (torch.stack(hi, 1) + start[:, None]).clamp(max=max(self.idx.numel() - 1, 0))
        self.g = torch.stack(g, 1)
        self.is_median = torch.tensor(self.median, device=lab.device)[None, :]

    def __call__(self):
        u = self.flat[self.idx].view(torch.int32).long() & 0xffffffff
        key = torch.where(u >= 0x80000000, u ^ 0xffffffff, u | 0x80000000)
        s = torch.sort(self.hi | key).values & 0xffffffff

        def value(k):                                # key -> float bits (as a signed 32-bit pattern) -> float32
            u = torch.where(k >= 0x80000000, k - 0x80000000, 0xffffffff - k)
            return torch.where(u >= 0x80000000, u - 0x100000000, u).to(torch.int32).view(torch.float32)
        a, b = value(s[self.lo]), value(s[self.hi_r])
        d = b - a
        lerp = torch.where(self.g >= 0.5, b - d * (1.0 - self.g), a + d * self.g)
        out = torch.where(self.is_median, (a + b) / 2.0, lerp)
        return torch.where(self.some[:, None], out, float("nan"))


def same(got, want):
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def bench_case(name, labels, n, plane, rounds, lib, say):
    H, W = labels.shape
    counts = torch.tensor([n], dtype=torch.int32, device="cuda")
    lab_h, plane_h = labels.cpu().numpy(), plane.cpu().numpy()
    t0 = time.perf_counter()
    nf3, want3 = numpy_rows(lab_h, n, plane_h, Q3)
    t_np = time.perf_counter() - t0
    _, want1 = numpy_rows(lab_h, n, plane_h, Q1)
    med = want1[:, 0]
    flat, labf = plane_h.reshape(-1), lab_h.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        dev_abs = np.where((labf >= 1) & (labf <= n), np.abs(flat - med[np.clip(labf, 1, max(n, 1)) - 1]), np.nan).astype(np.float32)
    _, want_mad = numpy_rows(lab_h, n, dev_abs.reshape(H, W), Q1)
    say(f"{name}: numpy reference done ({t_np:.1f} s for {Q3})")

    calls = {}
    for q in (Q1, Q3):
        out = {"n_finite": torch.empty((1, n), dtype=torch.int64, device="cuda"),
               "quantile": torch.empty((1, n, len(q)), dtype=torch.float32, device="cuda")}
        a = _lib.sc_cquant_args()
        a.labels, a.counts, a.N, a.H, a.W, a.M, a.Q = labels.data_ptr(), counts.data_ptr(), 1, H, W, n, len(q)
        a.plane, a.plane_stride, a.n_finite, a.quantile = plane.data_ptr(), H * W, out["n_finite"].data_ptr(), out["quantile"].data_ptr()
        for j, f in enumerate(plumes.quantile_fractions(q, "bench")):
            a.q[j] = float(f)
        wb = lib.sc_component_quantiles_workspace_bytes(1, H, W, n, len(q))
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        calls[q] = (a, work, wb, out)

    def run_a(q):
        a, work, wb, _ = calls[q]
        check(lib.sc_component_quantiles(a, ptr(work), wb, stream()))

    def run_b():
        return plumes.component_median_mad(labels, counts, plane, M=n)
    c1, c3 = TorchSort(labels, n, plane, Q1), TorchSort(labels, n, plane, Q3)

    # ---- equal first
    for q, want in ((Q1, want1), (Q3, want3)):
        run_a(q)
        first = {f: t.clone() for f, t in calls[q][3].items()}
        run_a(q)
        torch.cuda.synchronize()
        out = calls[q][3]
        assert all(torch.equal(first[f].view(torch.int32 if f == "quantile" else torch.int64),
                               out[f].view(torch.int32 if f == "quantile" else torch.int64)) for f in out), "two calls differ"
        assert np.array_equal(out["n_finite"][0].cpu().numpy(), nf3), f"{name}: n_finite differs from numpy"
        assert same(out["quantile"][0].cpu().numpy(), want), f"{name}: {q} differs from numpy"
    mm = run_b()
    assert same(mm["median"][0].cpu().numpy(), want1[:, 0]) and same(mm["mad"][0].cpu().numpy(), want_mad[:, 0]), f"{name}: median / MAD differ"
    assert same(c1().cpu().numpy(), want1) and same(c3().cpu().numpy(), want3), f"{name}: the torch.sort restatement differs from numpy"
    say(f"{name}: all results equal numpy")

    def events(fn, reps=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    runs = (lambda: run_a(Q1), lambda: run_a(Q3), run_b, c1, c3)
    for fn in runs:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in runs]
    for _ in range(rounds):
        for t, fn in zip(times, runs):
            t.append(events(fn))
    ta1, ta3, tb, tc1, tc3 = times
    say(f"{name}: rounds done")

    labelled = int(((labf >= 1) & (labf <= n)).sum())
    members = int(nf3.sum())
    large = int(nf3[nf3 > _lib.CQUANT_SMALL_MAX].sum())
    wb3 = calls[Q3][2]

    def moved(Q):
        return 2 * (4 * H * W + 4 * labelled) + 4 * members + 4 * (members - large) + 16 * large + n * (12 + 8 + 4 * Q)

    def line(tag, what, t, ref=None, Q=None):
        s = f"({tag}) {what} {np.mean(t):9.3f} ms per call   (rounds {min(t):.3f} .. {max(t):.3f})"
        if ref is not None:
            s += f"   / ({ref[0]}) = {np.mean(t) / np.mean(ref[1]):.2f}"
        if Q is not None:
            r = moved(Q) / (np.mean(t) * 1e-3) / 1e12
            s += f"   {moved(Q) / 1e6:.1f} MB -> {r:.3f} TB/s, {r / COPY_TBS[0]:.3f} / {r / COPY_TBS[1]:.3f} of the {COPY_TBS[0]} / {COPY_TBS[1]} TB/s copy"
        return s
    return [
        f"[{name}] {H} x {W} label image, {n} rows, {labelled} labelled pixels, {members} members (finite), the largest segment "
        f"{int(nf3.max()) if n else 0}, {int((nf3 > _lib.CQUANT_SMALL_MAX).sum())} segments above SC_CQUANT_SMALL_MAX = {_lib.CQUANT_SMALL_MAX} "
        f"holding {large} keys; workspace {wb3 / 1e6:.1f} MB",
        line("a1", "sc_component_quantiles (\"median\",)", ta1, Q=1),
        line("a3", "sc_component_quantiles (5, \"median\", 95)", ta3, Q=3),
        line("b", "plumes.component_median_mad (two calls, allocations included)", tb),
        line("c1", "torch.sort of composite keys, (\"median\",)", tc1, ref=("a1", ta1)),
        line("c3", "torch.sort of composite keys, (5, \"median\", 95)", tc3, ref=("a3", ta3)),
        f"(d) numpy per component (grouped by one argsort), (5, \"median\", 95), one run {t_np * 1e3:9.1f} ms",
        f"every round of (a1) below every round of (c1): {'yes' if max(ta1) < min(tc1) else 'NO'};  "
        f"every round of (a3) below every round of (c3): {'yes' if max(ta3) < min(tc3) else 'NO'}",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--cases", default="rings,plumes,noise")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    t_start = time.perf_counter()

    def say(what):
        torch.cuda.synchronize()
        print(f"[{time.perf_counter() - t_start:7.1f} s] {what}", flush=True)
    want = args.cases.split(",")
    lines = [f"exact order statistics per labelled component; {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); "
             f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; every result asserted equal to "
             f"numpy's np.percentile / np.median (float32, a zero of either sign) before timing, two calls identical bytes"]
    if "rings" in want or "plumes" in want:
        H, W = 2000, 2300
        mask, mag, _ = scene(H, W, 300, seed=20002300)
        plane = torch.from_numpy(mag).cuda()
        labels, n = mask_creation.connected_components(torch.from_numpy(mask).cuda())
        n = int(n)
        if "rings" in want:
            rings = plumes.background_rings(labels, 16, 2).contiguous()
            lines += bench_case("rings 16 / 2 of the plume mask", rings, n, plane, args.rounds, lib, say)
        if "plumes" in want:
            lines += bench_case("plume labels", labels.contiguous(), n, plane, args.rounds, lib, say)
    if "noise" in want:
        rng = np.random.default_rng(20002300)
        mask = rng.random((1000, 1000)) < 0.62
        mag = (rng.standard_normal((1000, 1000)) * 300).astype(np.float32)
        mag[rng.random((1000, 1000)) < 0.01] = np.nan
        for conn in (2, 1):                          # 2 is what tools/bench_plume_outlines.py labels it with
            labels, n = mask_creation.connected_components(torch.from_numpy(mask).cuda(), connectivity=conn)
            lines += bench_case(f"Bernoulli-0.62 noise 1000 x 1000, connectivity {conn}", labels.contiguous(), int(n),
                                torch.from_numpy(mag).cuda(), args.rounds, lib, say)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
