"""Time of the distance transform and the disc morphology (sc_edt / starcop_amd.morphology) next to restatements with stock torch
ops in the same process and to scipy.ndimage on the CPU.

    python tools/bench_morphology.py [--case plume|tile|both] [--rounds 6] [--reps 10] [--restatement plume|none] [--out profiles/morphology.txt]

  plume  the seeded 2000 x 2300 plume mask of tools/bench_component_stats.py (scene(..., seed=20002300))
  tile   a 10980 x 10980 class-map-like mask: smooth seeded noise thresholded at its 80th percentile (blobs, about 20 % set)
Rows: the unbounded transform (the envelope row pass), dilate at radius 3 and 16, opening at radius 1, remove_small_objects(8);
(b) the same operators from stock torch ops -- F.conv2d of the float mask with the disc kernel > 0 (exact for binary images:
the sums are small integers), the sieve by bincount and indexing over the same labelling; (c) scipy.ndimage, one run each.
(a) and (b) alternate in rounds of ``reps`` calls after as many warm-up calls, device events; the figure is the mean over the
rounds, the spread the fastest and slowest round.  Every result is asserted equal to the oracle before anything is timed.
On the plume mask, both row passes forced at cap radii 4 .. 64: the table SC_EDT_WINDOW_MAX_R is read from.
Bytes per call by index arithmetic (mask once, the band words and carries, g written and read, the transposed result written
and read for the envelope, the output); the envelope's stack traffic depends on the image and is not counted.
Every step prints a line as it begins.  (b) runs on the plume mask only (``--restatement none``: nowhere); the tile rows are
(a) and (c)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from scipy import ndimage  # noqa: E402

import morphology_util as U  # noqa: E402
from bench_component_stats import scene  # noqa: E402
from starcop_amd import _lib, mask_creation, morphology as mo  # noqa: E402

torch.set_num_threads(min(16, torch.get_num_threads()))


def tile_mask(n=10980, seed=10980):
    rng = np.random.default_rng(seed)
    k = 16
    low = ndimage.gaussian_filter(rng.standard_normal((n // k + 2, n // k + 2)).astype(np.float32), 1.5)
    up = ndimage.zoom(low, k, order=1)[:n, :n]
    return (up > np.quantile(up[::7, ::7], 0.8)).astype(np.uint8)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, rounds, reps):
    """[fn, ...] -> [[ms per call of every round], ...], the functions taking turns round by round"""
    for fn in fns:
        for _ in range(reps):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(events(fn, reps))
    return times


T0 = time.perf_counter()


def progress(what):
    """one line per step as it begins, so that a log shows where a long run is"""
    print(f"[{time.perf_counter() - T0:7.1f} s] {what}", flush=True)


def fmt(t):
    return f"{np.mean(t):9.3f} ms   (rounds {min(t):.3f} .. {max(t):.3f})"


def disc_kernel(r):
    return torch.from_numpy(U.disc(r).astype(np.float32)).cuda()[None, None]


def torch_dilate(mf, kern):
    return (F.conv2d(mf, kern, padding=kern.shape[-1] // 2) > 0).to(torch.uint8)


def torch_erode(mf, kern):                                   # no unset pixel under the disc; the zero padding is "outside is set"
    return (F.conv2d(1.0 - mf, kern, padding=kern.shape[-1] // 2) == 0).to(torch.uint8)


def torch_sieve(mask, min_area):
    labels, _ = mask_creation.connected_components(mask)
    keep = torch.bincount(labels.reshape(-1)) >= min_area
    keep[0] = False
    return keep[labels.long()].to(torch.uint8)


def edt_bytes(px, variant, out_bytes):
    tables = px / 64.0 * (3 * 8 + 2 * 2 * 4)                 # band words written once and read twice, carries written and read
    if variant == "window":
        return px * (1 + 2 + 2 + out_bytes) + tables
    return px * (1 + 2 + 2 + 4 + 4 + out_bytes) + tables


def run_case(name, mask, args, lines, variants_table):
    H, W = mask.shape
    px = H * W
    restate = args.restatement == name
    d = torch.from_numpy(mask).cuda()
    mf = d.float()[None, None]
    lines.append(f"--- {name}: {H} x {W} uint8 mask, {100.0 * mask.mean():.1f} % set")
    # oracles first (their one run is the scipy row), and every device result is checked before it is timed
    progress(f"{name}: scipy distance_transform_edt")
    t = time.perf_counter()
    d2 = U.d2_scipy(mask != 0)
    cpu = {"edt": (time.perf_counter() - t) * 1e3}
    progress(f"{name}: unbounded transform against the oracle")
    got = mo.distance_transform(d, squared=True, variant="envelope")
    torch.cuda.synchronize()
    progress(f"{name}: float32 distances against the oracle")
    assert np.array_equal(got.cpu().numpy(), d2.astype(np.int32)), "unbounded transform disagrees with scipy"
    dist = mo.distance_transform(d, pixel_size=5.0)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), U.dist_f32(d2, 5.0).view(np.uint32)), "float32 distances disagree"
    del got, dist
    rows = []
    for r in (3, 16):
        want = torch.from_numpy((d2 <= int(np.floor(r * r))).astype(np.uint8)).cuda()
        kern = disc_kernel(r)
        progress(f"{name}: dilate radius {r} against the oracle")
        assert torch.equal(mo.dilate(d, r), want), f"dilate {r} disagrees with the oracle"
        same = None
        if restate:
            progress(f"{name}: conv2d dilation radius {r} against the oracle")
            try:
                same = torch.equal(torch_dilate(mf, kern)[0, 0], want)
            except torch.cuda.OutOfMemoryError:              # reported by the timing loop below
                pass
        assert same is not False, f"conv2d dilation {r} disagrees with the oracle"
        rows.append((f"dilate radius {r}", (lambda r=r: mo.dilate(d, r)), (lambda kern=kern: torch_dilate(mf, kern)), f"dilate{r}"))
        if r == 3 or name == "plume":
            progress(f"{name}: scipy binary_dilation radius {r}")
            t = time.perf_counter()
            ref = ndimage.binary_dilation(mask != 0, U.disc(r))
            cpu[f"dilate{r}"] = (time.perf_counter() - t) * 1e3
            assert np.array_equal(ref, want.cpu().numpy() != 0)
        del want
    k1 = disc_kernel(1)

    def torch_opening():
        return torch_dilate(torch_erode(mf, k1).float(), k1)
    progress(f"{name}: opening against scipy")
    t = time.perf_counter()
    ref = ndimage.binary_dilation(ndimage.binary_erosion(mask != 0, U.disc(1), border_value=1), U.disc(1))
    cpu["opening1"] = (time.perf_counter() - t) * 1e3
    want = torch.from_numpy(ref.astype(np.uint8)).cuda()
    assert torch.equal(mo.opening(d, 1), want), "opening disagrees with scipy"
    if restate:
        progress(f"{name}: conv2d opening against scipy")
        assert torch.equal(torch_opening()[0, 0], want), "conv2d opening disagrees with scipy"
    rows.append(("opening radius 1", lambda: mo.opening(d, 1), torch_opening, "opening1"))
    progress(f"{name}: sieve against scipy")
    t = time.perf_counter()
    ref = U.sieve(mask, 8)
    cpu["sieve8"] = (time.perf_counter() - t) * 1e3
    want = torch.from_numpy(ref).cuda()
    assert torch.equal(mo.remove_small_objects(d, 8), want), "sieve disagrees with scipy"
    if restate:
        progress(f"{name}: bincount sieve against scipy")
        assert torch.equal(torch_sieve(d, 8), want), "bincount sieve disagrees with scipy"
    rows.append(("remove_small_objects(8)", lambda: mo.remove_small_objects(d, 8), lambda: torch_sieve(d, 8), "sieve8"))
    del want, ref

    progress(f"{name}: timing the unbounded transform")
    (te,) = alternate([lambda: mo.distance_transform(d, squared=True, variant="envelope")], args.rounds, args.reps)
    b = edt_bytes(px, "envelope", 4)
    lines.append(f"unbounded transform (envelope, int32 out)   (a) {fmt(te)}   {b / 1e6:.1f} MB -> {b / (np.mean(te) * 1e-3) / 1e12:.3f} TB/s"
                 f"   (c) scipy distance_transform_edt {cpu['edt']:.0f} ms = {cpu['edt'] / np.mean(te):.0f} x (a)")
    print(lines[-1], flush=True)
    for label, fa, fb, key in rows:
        progress(f"{name}: timing {label}")
        if not restate:
            (ta,) = alternate([fa], args.rounds, args.reps)
            line = f"{label:26s} (a) {fmt(ta)}   (b) not run"
        else:
            try:
                ta, tb = alternate([fa, fb], args.rounds, args.reps)
                below = "every round of (a) below every round of (b)" if max(ta) < min(tb) else "NOT every round of (a) below every round of (b)"
                line = f"{label:26s} (a) {fmt(ta)}   (b) torch {fmt(tb)}   (b) / (a) = {np.mean(tb) / np.mean(ta):.2f}: {below}"
            except torch.cuda.OutOfMemoryError as e:         # the restatement may not fit: say so, time (a) alone
                torch.cuda.synchronize()
                (ta,) = alternate([fa], args.rounds, args.reps)
                line = f"{label:26s} (a) {fmt(ta)}   (b) torch failed: {str(e).splitlines()[0][:80]}"
        if key.startswith("dilate"):
            b = edt_bytes(px, "window", 1)
            line += f"   (a) {b / 1e6:.1f} MB -> {b / (np.mean(ta) * 1e-3) / 1e12:.3f} TB/s"
        if key in cpu:
            line += f"   (c) scipy {cpu[key]:.0f} ms"
        lines.append(line)
        print(line, flush=True)
    if variants_table:
        lines.append(f"row passes forced, capped int32 transform of the {name} mask (max_distance = radius): window | envelope")
        for r in (4, 8, 16, 32, 64):
            if r > mo.WINDOW_MAX_R:
                lines.append(f"  radius {r:3d}: the window is refused above SC_EDT_WINDOW_MAX_R = {mo.WINDOW_MAX_R}")
                continue
            want = torch.from_numpy(U.capped(d2, r * r).astype(np.int32)).cuda()
            fw = lambda r=r: mo.distance_transform(d, max_distance=r, squared=True, variant="window")      # noqa: E731
            fe = lambda r=r: mo.distance_transform(d, max_distance=r, squared=True, variant="envelope")    # noqa: E731
            assert torch.equal(fw(), want) and torch.equal(fe(), want), f"capped transform at {r} disagrees with the oracle"
            tw, tv = alternate([fw, fe], args.rounds, args.reps)
            verdict = "window below envelope in every round" if max(tw) < min(tv) else "NOT every round of window below every round of envelope"
            lines.append(f"  radius {r:3d}: window {fmt(tw)} | envelope {fmt(tv)} | {verdict}")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both", choices=("plume", "tile", "both"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--restatement", default="plume", choices=("plume", "none"), help="where the stock torch ops (b) run too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lines = [f"distance transform and disc morphology; {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); "
             f"{args.rounds} alternating rounds of {args.reps} calls after {args.reps} warm-up calls each, device events; every result equal to its "
             "oracle before it is timed; rates next to the 4.25 / 4.70 TB/s of the access-pattern copy (4- / 16-byte accesses)"]
    if args.case in ("plume", "both"):
        run_case("plume", scene(2000, 2300, 300, seed=20002300)[0].astype(np.uint8), args, lines, True)
    if args.case in ("tile", "both"):
        run_case("tile", tile_mask(), args, lines, False)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
